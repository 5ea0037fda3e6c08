#!/usr/bin/env python3
"""Golden vectors for VITS2 monotonic alignment search: the `with torch.no_grad():` block of SynthesizerTrn.forward
(vits2/models.py:1224-1254) and monotonic_align/core.pyx, produced by the reference's own code on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_align.py <path to the reference's vits2 directory>

The reference ships core.pyx uncompiled.  This script copies it into a temporary directory, compiles it there with Cython's
pyximport and calls maximum_path_c as the reference's wrapper does (monotonic_align/__init__.py:6-19: fp32 copy of neg_cent, zeroed
int32 path, t_t_max = mask.sum(1)[:, 0], t_s_max = mask.sum(2)[:, 0]).  Nothing compiled and no reference text is written here.

Writes tests/golden/align_small.npz + align_meta.json:
  model/{x, x_lengths, y, y_lengths, sid, noise}   one SynthesizerTrn.forward call (reduced dims, 3 speakers, ragged lengths, every
                                      parameter randomised, the zero-initialised `post` convs included); noise: the posterior's draw
  model/{z, z_p, m_p, logs_p, neg_cent, t_y, t_x, frame_token, w}   what the call computed up to `w = attn.sum(2)`; the path is kept
                                      as frame_token [B, T_y] int16 (-1 at padded frames)
  ragged/{neg_cent, t_y, t_x, frame_token}   a random ragged batch
  alone/<name>/{neg_cent, frame_token}   stand-alone cases (tests/test_align_host.alone_cases): integer costs (int8) and multiples
                                      of 1 / 64 (int16, x 64), t_x in (1, 2, 63, 64, 65, 129), t_y = t_x and t_y >> t_x
and in the meta JSON the seeds and checksums of the model's weights (tests/test_align_host.align_net redraws them), and the error
of the reference's fp32 torch-CPU neg_cent against an fp64 evaluation of the same lines (max abs error / max |value|) at the fixture's
dims and at C = 192, 600 x 150 on tests/test_align_host.neg_cent_inputs: the bar of the GPU test is 4 x these."""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

TMP = tempfile.mkdtemp(prefix="mas_ref_")
shutil.copy(os.path.join(REF, "monotonic_align", "core.pyx"), os.path.join(TMP, "refcore.pyx"))
import pyximport  # noqa: E402

pyximport.install(language_level=3, build_dir=os.path.join(TMP, "_build"), inplace=False)
sys.path.insert(0, TMP)
import refcore  # noqa: E402  (the reference's core.pyx, compiled outside the repository)


def maximum_path(neg_cent, mask):
    """The reference's wrapper, call for call."""
    device, dtype = neg_cent.device, neg_cent.dtype
    neg_cent = neg_cent.data.cpu().numpy().astype(np.float32)
    path = np.zeros(neg_cent.shape, dtype=np.int32)
    t_t_max = mask.sum(1)[:, 0].data.cpu().numpy().astype(np.int32)
    t_s_max = mask.sum(2)[:, 0].data.cpu().numpy().astype(np.int32)
    refcore.maximum_path_c(path, neg_cent, t_t_max, t_s_max)
    return torch.from_numpy(path).to(device=device, dtype=dtype)


stub = types.ModuleType("monotonic_align")
stub.maximum_path = maximum_path
sys.modules["monotonic_align"] = stub
sys.path.insert(0, REF)
import models  # noqa: E402

from test_align_host import alone_cases, alone_costs, checksum, neg_cent_inputs, neg_cent_torch, rel_err  # noqa: E402
from test_duration_host import randomize  # noqa: E402

NET = dict(n_vocab=23, spec_channels=16, segment_size=32, inter_channels=16, hidden_channels=32, filter_channels=48, n_heads=2, n_layers=2,
           kernel_size=3, p_dropout=0.1, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
           upsample_rates=[4, 2], upsample_initial_channel=32, upsample_kernel_sizes=[8, 4], use_transformer_flows=True,
           transformer_flow_type="pre_conv")
PARTS = ("enc_p", "enc_q", "flow", "emb_g")
out = {}


def frame_token(path, t_y):
    """[B, T_y, T_x] 0 / 1 -> [B, T_y] int16, -1 at padded frames; checks one token per frame inside the lengths, none outside."""
    path = path.numpy() if isinstance(path, torch.Tensor) else path
    ft = path.argmax(2).astype(np.int16)
    for b, ty in enumerate(t_y):
        assert (path[b, :ty].sum(1) == 1).all() and path[b, ty:].sum() == 0
        ft[b, ty:] = -1
    return ft


class Stop(Exception):
    pass


def model_case(meta, seed=90):
    torch.manual_seed(seed)
    net = models.SynthesizerTrn(**NET, n_speakers=3, gin_channels=4).eval()
    seeds = {part: 1000 * seed + len(part) for part in PARTS}
    for part in PARTS:
        randomize(getattr(net, part), seeds[part])
    B, T_x, T_y = 4, 9, 31
    x_lengths, y_lengths = torch.tensor([9, 6, 3, 1]), torch.tensor([31, 17, 3, 8])
    x = torch.randint(0, NET["n_vocab"], (B, T_x))
    y = torch.randn(B, NET["spec_channels"], T_y)
    sid = torch.tensor([0, 2, 1, 1])
    got = {}
    real_mp, real_rl = stub.maximum_path, torch.randn_like

    def recording_maximum_path(neg_cent, mask):
        got["neg_cent"], got["mask"] = neg_cent.clone(), mask.clone()
        got["path"] = real_mp(neg_cent, mask)
        raise Stop  # (the rest of forward - segment slicing, the generator - is not part of the fixture)

    def randn_like(*a, **k):
        got.setdefault("draws", []).append(real_rl(*a, **k))
        return got["draws"][-1].clone()

    hooks = [net.enc_p.register_forward_hook(lambda m, i, o: got.update(m_p=o[1], logs_p=o[2])),
             net.enc_q.register_forward_hook(lambda m, i, o: got.update(z=o[0])),
             net.flow.register_forward_hook(lambda m, i, o: got.update(z_p=o))]
    stub.maximum_path, torch.randn_like = recording_maximum_path, randn_like
    try:
        with torch.no_grad():
            net(x, x_lengths, y, y_lengths, sid=sid)
    except Stop:
        pass
    finally:
        stub.maximum_path, torch.randn_like = real_mp, real_rl
        for h in hooks:
            h.remove()
    assert len(got["draws"]) == 1
    t_y = got["mask"].sum(1)[:, 0].int().numpy()
    t_x = got["mask"].sum(2)[:, 0].int().numpy()
    assert t_y.tolist() == y_lengths.tolist() and t_x.tolist() == x_lengths.tolist()
    rec = dict(x=x, x_lengths=x_lengths, y=y, y_lengths=y_lengths, sid=sid, noise=got["draws"][0], z=got["z"], z_p=got["z_p"], m_p=got["m_p"],
               logs_p=got["logs_p"], neg_cent=got["neg_cent"], w=got["path"].unsqueeze(1).sum(2))
    for k, v in rec.items():
        out[f"model/{k}"] = v.numpy()
    out["model/t_y"], out["model/t_x"] = t_y, t_x
    out["model/frame_token"] = frame_token(got["path"], t_y)
    # the restated formula in fp32 is the reference's arithmetic: the same bits on this host
    assert torch.equal(neg_cent_torch(got["z_p"], got["m_p"], got["logs_p"]), got["neg_cent"])
    meta["model"] = dict(n_speakers=3, gin_channels=4, seeds=seeds, checksums={part: checksum(getattr(net, part)) for part in PARTS},
                         B=B, T_x=T_x, T_y=T_y)
    return got


def run_alone(nc, t_y, t_x):
    B, T_y, T_x = nc.shape
    mask = (torch.arange(T_y)[None, :, None] < torch.tensor(t_y)[:, None, None]) & (torch.arange(T_x)[None, None, :] < torch.tensor(t_x)[:, None, None])
    return maximum_path(torch.from_numpy(nc), mask.float())


def main():
    meta = {"net": NET}
    got = model_case(meta)
    rng = np.random.default_rng(0)
    nc = (rng.standard_normal((6, 40, 17)) * 5).astype(np.float32)
    t_y, t_x = np.array([40, 33, 17, 20, 40, 25], np.int32), np.array([17, 10, 17, 1, 3, 12], np.int32)
    out.update({"ragged/neg_cent": nc, "ragged/t_y": t_y, "ragged/t_x": t_x, "ragged/frame_token": frame_token(run_alone(nc, t_y, t_x), t_y)})
    meta["alone"] = []
    for name, ty, tx in alone_cases():
        c = alone_costs(name, ty, tx)
        out[f"alone/{name}/neg_cent"] = c.astype(np.int8) if name.startswith("int") else np.round(c * 64).astype(np.int16)
        out[f"alone/{name}/frame_token"] = frame_token(run_alone(c[None], [ty], [tx]), [ty])[0]
        meta["alone"].append([name, ty, tx])
    # the reference's own fp32 error against fp64, which sets the bar of the GPU test
    z_p, m_p, logs_p = neg_cent_inputs(11, 2, 192, 600, 150)
    meta["neg_cent_cpu_f32_err"] = {
        "golden": rel_err(got["neg_cent"], neg_cent_torch(got["z_p"].double(), got["m_p"].double(), got["logs_p"].double())),
        "c192_600x150": rel_err(neg_cent_torch(z_p, m_p, logs_p), neg_cent_torch(z_p.double(), m_p.double(), logs_p.double())),
        "inputs": "test_align_host.neg_cent_inputs(11, 2, 192, 600, 150)", "torch": torch.__version__, "threads": torch.get_num_threads()}
    np.savez_compressed(os.path.join(HERE, "align_small.npz"), **out)
    with open(os.path.join(HERE, "align_meta.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in meta.items()) + "\n}\n")
    print(os.path.getsize(os.path.join(HERE, "align_small.npz")), "bytes", meta["neg_cent_cpu_f32_err"])
    shutil.rmtree(TMP, ignore_errors=True)


if __name__ == "__main__":
    main()
