#!/usr/bin/env python3
"""Golden vectors for VITS2 voice conversion (vits2/models.py:1328-1336): the PosteriorEncoder (models.py:858-897), the forward direction
of ResidualCouplingTransformersBlock (models.py:803-806 over :506-526) and one whole SynthesizerTrn.voice_conversion call, produced by the
reference's own models.py on CPU.  models.py imports monotonic_align at module level, which inference never uses: a stub stands in.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vc.py <path to the reference's vits2 directory>

Writes tests/golden/vc_small.npz + vc_meta.json (reduced dims, no reference source):
  post{S}_{gin}/w/<key>               PosteriorEncoder(S, 8, 16, 5, 1, 3, gin) state dicts, S in (16, 13), gin in (0, 8), weights randomised
  post{S}/y, post{S}/lengths          y [3, S, 11] (lengths 11, 6, 1), unmasked past the lengths (the reference masks after pre)
  post/g8, post/noise                 speaker rows [3, 8, 1] and the draw torch.randn_like(m) [3, 8, 11] (recorded)
  post{S}_{gin}/{z, m, logs, x_mask}  the reference's outputs
  flow/w/<key>, flow/{x, x_mask, g, out}   ResidualCouplingTransformersBlock(16, 16, 5, 1, 2, 4, gin 8, pre_conv) forward with g
  vc/{y, lengths, sid_src, sid_tgt, noise, o_hat, y_mask, z, z_p, z_hat}   one voice_conversion call of a SynthesizerTrn with
                                      n_speakers = 3 and upsampling [4, 2] (noise: its posterior draw, recorded)
and in the meta JSON the seeds and checksums of that model's enc_q / flow / dec / emb_g weights (tests/test_vc_host.py redraws them with
test_duration_host.randomize), the dims, and the state-dict key / shape list of PosteriorEncoder at the ModelConfig dims."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = sys.argv[1]
sys.path.insert(0, REF)
sys.modules.setdefault("monotonic_align", types.ModuleType("monotonic_align"))  # (imported by models.py, unused by inference)
import models  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_duration_host import randomize  # noqa: E402  (the fixtures' weight rule, shared with the duration fixtures)

NET = dict(n_vocab=23, spec_channels=16, segment_size=32, inter_channels=16, hidden_channels=32, filter_channels=48, n_heads=2, n_layers=2,
           kernel_size=3, p_dropout=0.1, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
           upsample_rates=[4, 2], upsample_initial_channel=32, upsample_kernel_sizes=[8, 4], use_transformer_flows=True,
           transformer_flow_type="pre_conv")
PARTS = ("enc_q", "flow", "dec", "emb_g")
POST = dict(inter=8, hidden=16, kernel=5, n_layers=3)
FLOW = dict(channels=16, hidden=16, kernel=5, n_layers=2, n_flows=4, gin=8)
out = {}


def save_sd(prefix, mod):
    for k, v in mod.state_dict().items():
        out[f"{prefix}/w/{k}"] = v.detach().numpy().copy()


def checksum(mod):
    """[tensors, elements, sum, sum |v|, sum over tensors of (index + 1) * sum]: a state dict's keys, shapes, values and order."""
    vs = [v.double() for v in mod.state_dict().values()]
    return [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
            float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]


class Recorder:
    """Records what torch.randn_like returns inside models.py (the posterior's draw)."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self._randn_like = torch.randn_like

        def randn_like(*a, **k):
            r = self._randn_like(*a, **k)
            self.draws.append(r.clone())
            return r

        torch.randn_like = randn_like
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._randn_like


def posterior(meta):
    torch.manual_seed(5)
    B, T = 3, 11
    lengths = torch.tensor([11, 6, 1])
    g = torch.randn(B, 8, 1)
    noise = torch.randn(B, POST["inter"], T)
    out.update({"post/g8": g.numpy(), "post/noise": noise.numpy()})
    for S in (16, 13):
        y = torch.randn(B, S, T)
        out.update({f"post{S}/y": y.numpy(), f"post{S}/lengths": lengths.numpy()})
        for gin in (0, 8):
            enc = randomize(models.PosteriorEncoder(S, POST["inter"], POST["hidden"], POST["kernel"], 1, POST["n_layers"], gin_channels=gin).eval(),
                            100 + S + gin)
            save_sd(f"post{S}_{gin}", enc)
            real = torch.randn_like
            with torch.no_grad():
                torch.randn_like = lambda *a, **k: noise.clone()  # the recorded draw
                try:
                    z, m, logs, x_mask = enc(y, lengths, g=g if gin else None)
                finally:
                    torch.randn_like = real
            for k, v in dict(z=z, m=m, logs=logs, x_mask=x_mask).items():
                out[f"post{S}_{gin}/{k}"] = v.numpy()
    meta["post"] = dict(POST, B=B, T=T, lengths=lengths.tolist(), spec=[16, 13], gin=[0, 8])


def flow_forward(meta):
    torch.manual_seed(6)
    B, T = 3, 10
    lengths = torch.tensor([10, 7, 2])
    x_mask = (torch.arange(T)[None, :] < lengths[:, None]).unsqueeze(1).float()
    x = torch.randn(B, FLOW["channels"], T) * x_mask
    g = torch.randn(B, FLOW["gin"], 1)
    fl = randomize(models.ResidualCouplingTransformersBlock(FLOW["channels"], FLOW["hidden"], FLOW["kernel"], 1, FLOW["n_layers"], FLOW["n_flows"],
                                                            gin_channels=FLOW["gin"], use_transformer_flows=True,
                                                            transformer_flow_type="pre_conv").eval(), 200)
    with torch.no_grad():
        y = fl(x, x_mask, g=g)
    save_sd("flow", fl)
    out.update({"flow/x": x.numpy(), "flow/x_mask": x_mask.numpy(), "flow/g": g.numpy(), "flow/out": y.numpy()})
    meta["flow"] = dict(FLOW, B=B, T=T, lengths=lengths.tolist())


def vc_case(meta, seed=70):
    torch.manual_seed(seed)
    net = models.SynthesizerTrn(**NET, n_speakers=3, gin_channels=4).eval()
    net.n_speakers = 3  # (voice_conversion asserts on self.n_speakers, which SynthesizerTrn.__init__ never stores)
    seeds = {part: 1000 * seed + len(part) for part in PARTS}
    for part in PARTS:
        randomize(getattr(net, part), seeds[part])
    B, T = 3, 9
    y = torch.randn(B, NET["spec_channels"], T)
    lengths = torch.tensor([9, 5, 2])
    sid_src, sid_tgt = torch.tensor([0, 2, 1]), torch.tensor([1, 0, 1])
    with torch.no_grad(), Recorder() as rec:
        o_hat, y_mask, (z, z_p, z_hat) = net.voice_conversion(y, lengths, sid_src, sid_tgt)
    assert len(rec.draws) == 1, len(rec.draws)
    rec_out = dict(y=y, lengths=lengths, sid_src=sid_src, sid_tgt=sid_tgt, noise=rec.draws[0], o_hat=o_hat, y_mask=y_mask, z=z, z_p=z_p, z_hat=z_hat)
    for k, v in rec_out.items():
        out[f"vc/{k}"] = v.numpy()
    meta["vc"] = dict(n_speakers=3, gin_channels=4, seeds=seeds, checksums={part: checksum(getattr(net, part)) for part in PARTS})


def main():
    meta = {"net": NET}
    posterior(meta)
    flow_forward(meta)
    vc_case(meta)
    pe = models.PosteriorEncoder(80, 192, 192, 5, 1, 16, gin_channels=256)
    meta["fulldims_post_state_dict"] = [[k, list(v.shape)] for k, v in pe.state_dict().items()]
    np.savez_compressed(os.path.join(HERE, "vc_small.npz"), **out)
    lines = []
    for k, v in meta.items():
        if k.startswith("fulldims_"):
            lines.append(f" {json.dumps(k)}: [\n  " + ",\n  ".join(json.dumps(r) for r in v) + "\n ]")
        else:
            lines.append(f" {json.dumps(k)}: {json.dumps(v)}")
    with open(os.path.join(HERE, "vc_meta.json"), "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(os.path.getsize(os.path.join(HERE, "vc_small.npz")), "bytes")


if __name__ == "__main__":
    main()
