#!/usr/bin/env python3
"""Golden vectors for the VITS2 duration likelihood: StochasticDurationPredictor.forward(x, x_mask, w, g=g) (vits2/models.py:78-125)
and SynthesizerTrn.forward up to l_length (models.py:1214-1267), produced by the reference's own models.py on CPU in eval mode.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_durnll.py <path to the reference's vits2 directory>

monotonic_align is the reference's core.pyx compiled by pyximport in a temporary directory, as make_golden_align.py does (imported
from there: nothing compiled and no reference text is written here).

Writes tests/golden/durnll_small.npz + durnll_meta.json:
  case/x, case/x_mask, case/g4, case/w, case/e_q    x [3, 32, 9] (lengths 9, 5, 1; padded frames zero), speaker rows, integer
                                      durations 1 - 12 [3, 1, 9] (zero at padded tokens), the recorded draw torch.randn(3, 2, 9)
  sdp{0,4}/nll, sdp{0,4}/z            the reference's nll [3] and its z after the flows [3, 2, 9] of StochasticDurationPredictor(32, 192,
                                      3, 0.5, 4, gin), weights by make_golden_duration.randomize (seed in the meta file; the tests
                                      redraw them and check the recorded checksum)
  sdp{0,4}/nll64, sdp{0,4}/z64        the same from the same module after .double() (what the tests' fp64 restatement must reproduce)
  model_{sdp,dp,sdp_g}/{x, x_lengths, y, y_lengths, sid, e_post, e_q, e_w, l_length, attn, logw, logw_, hidden_x}
                                      one SynthesizerTrn.forward call at make_golden_align.py's dims with a stochastic / a plain
                                      duration predictor / speakers, every draw recorded (e_post: the posterior encoder's)
and in the meta JSON the seeds and checksums of every weight, and the yardstick of the GPU tests' bar: the error of the reference's
own fp32 CPU nll against the same module in fp64, max |a - b| / (0.1 + |b|), at the fixture dims and at C = 192, T = 150 with lengths
150 / 149 / 64 / 2.  The weights are redrawn (next seed) until it is <= 2.5e-5: the GPU bar of 1e-4 is then at least 4 x the
reference's own error, the convention of align_meta.json.  For the C = 192 case with speakers, which the tests compare z on as well,
the weights are also redrawn until the reference's own fp32 z is within a quarter of the tests' bar on z (c192_t150_g4; every seed
tried is recorded with its two figures)."""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
import make_golden_align as A  # noqa: E402  (the monotonic_align stand-in, NET; imports the reference's models)
from make_golden_duration import Recorder, checksum, randomize  # noqa: E402

models = A.models
W = 32
YARD_MAX = 2.5e-5
PARTS = ("enc_p", "enc_q", "flow", "dp", "emb_g")
out = {}


def rel(a, b):
    return float(((a.double() - b.double()).abs() / (0.1 + b.double().abs())).max())


def mask_of(lengths, T):
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).unsqueeze(1).float()


def nll_with(sdp, x, x_mask, w, g, e_q):
    """sdp.forward(x, x_mask, w, g=g) with e_q as its draw -> (nll [B], z after the flows): z is the last flow's output."""
    got = {}
    hook = sdp.flows[-1].register_forward_hook(lambda m, i, o: got.update(z=o[0].detach().clone()))
    real = torch.randn
    torch.randn = lambda *a, **k: e_q.clone()
    try:
        with torch.no_grad():
            nll = sdp(x, x_mask, w, g=g)
    finally:
        torch.randn = real
        hook.remove()
    return nll, got["z"]


def yardstick(sdp, x, x_mask, w, g, e_q):
    import copy

    a, _ = nll_with(sdp, x, x_mask, w, g, e_q)
    d = copy.deepcopy(sdp).double()
    b, z = nll_with(d, x.double(), x_mask.double(), w.double(), None if g is None else g.double(), e_q.double())
    return rel(a, b), b, z


def z_ratio(sdp, x, x_mask, w, g, e_q):
    """The reference's own fp32 CPU z against the same module in fp64, as a fraction of the GPU tests' bar on z:
    max |a - b| / (ATOL + RTOL |b|) with RTOL, ATOL = 1e-4, 1e-5."""
    _, a = nll_with(sdp, x, x_mask, w, g, e_q)
    _, _, b = yardstick(sdp, x, x_mask, w, g, e_q)
    return float(((a.double() - b).abs() / (1e-5 + 1e-4 * b.abs())).max())


def big_case(seed):
    gen = torch.Generator().manual_seed(seed)
    lengths = [150, 149, 64, 2]
    x_mask = mask_of(lengths, 150)
    x = torch.randn(4, 192, 150, generator=gen) * x_mask
    w = torch.randint(1, 13, (4, 1, 150), generator=gen).float() * x_mask
    e_q = torch.randn(4, 2, 150, generator=gen)
    return x, x_mask, w, e_q


def predictors(meta):
    torch.manual_seed(3)  # make_golden_duration.predictors' x, x_mask and g
    x = torch.randn(3, W, 9)
    x_mask = mask_of([9, 5, 1], 9)
    x = x * x_mask
    g = torch.randn(3, 4, 1)
    gen = torch.Generator().manual_seed(77)
    w = torch.randint(1, 13, (3, 1, 9), generator=gen).float() * x_mask
    e_q = torch.randn(3, 2, 9, generator=gen)
    out.update({"case/x": x.numpy(), "case/x_mask": x_mask.numpy(), "case/g4": g.numpy(), "case/w": w.numpy(), "case/e_q": e_q.numpy()})
    meta["sdp"] = {}
    for gin in (0, 4):
        gg = g if gin else None
        for seed in range(20 + gin, 2000, 100):
            sdp = randomize(models.StochasticDurationPredictor(W, 192, 3, 0.5, 4, gin_channels=gin).eval(), seed)
            err, nll64, z64 = yardstick(sdp, x, x_mask, w, gg, e_q)
            if err <= YARD_MAX:
                break
        else:
            raise RuntimeError("no weights within the yardstick")
        nll, z = nll_with(sdp, x, x_mask, w, gg, e_q)
        out[f"sdp{gin}/nll"], out[f"sdp{gin}/z"] = nll.numpy(), z.numpy()
        out[f"sdp{gin}/nll64"], out[f"sdp{gin}/z64"] = nll64.numpy(), z64.numpy()
        meta["sdp"][str(gin)] = dict(seed=seed, checksum=checksum(sdp), cpu_f32_err=err)
    # the model dims
    for seed in range(7, 2000, 100):
        sdp = randomize(models.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=0).eval(), seed)
        x, x_mask, w, e_q = big_case(seed + 1)
        err, _, _ = yardstick(sdp, x, x_mask, w, None, e_q)
        if err <= YARD_MAX:
            break
    else:
        raise RuntimeError("no weights within the yardstick")
    nll, _ = nll_with(sdp, x, x_mask, w, None, e_q)
    meta["c192_t150"] = dict(seed=seed, case_seed=seed + 1, lengths=[150, 149, 64, 2], cpu_f32_err=err, nll=nll.tolist(),
                             z_cpu_f32_ratio=z_ratio(sdp, x, x_mask, w, None, e_q),
                             inputs="make_golden_durnll.big_case(case_seed)", torch=torch.__version__, threads=torch.get_num_threads())
    # the same inputs with speakers: weights drawn until the nll yardstick holds and the reference's own fp32 z lies within a
    # quarter of the tests' bar on z at every token (a token whose z fp32 cannot hold says nothing about a kernel)
    g = torch.randn(4, 4, 1, generator=torch.Generator().manual_seed(9))
    tried = {}
    for gseed in range(seed + 4, 10000, 100):
        sdp = randomize(models.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=4).eval(), gseed)
        err, _, _ = yardstick(sdp, x, x_mask, w, g, e_q)
        ratio = z_ratio(sdp, x, x_mask, w, g, e_q)
        tried[str(gseed)] = [err, ratio]
        if err <= YARD_MAX and ratio <= 0.25:
            break
    else:
        raise RuntimeError("no weights within the yardsticks")
    meta["c192_t150_g4"] = dict(seed=gseed, g_seed=9, cpu_f32_err=err, z_cpu_f32_ratio=ratio, z_ratio_max=0.25, tried=tried)


def model_case(meta, name, use_sdp, n_speakers, seed):
    gin = 4 if n_speakers else 0
    torch.manual_seed(seed)
    net = models.SynthesizerTrn(**A.NET, n_speakers=n_speakers, gin_channels=gin, use_sdp=use_sdp).eval()
    seeds = {part: 1000 * seed + len(part) for part in PARTS if hasattr(net, part)}
    for part, s in seeds.items():
        randomize(getattr(net, part), s)
    B, T_x, T_y = 4, 9, 47  # (every utterance has at least segment_size = 32 frames: forward goes on to slice them)
    x_lengths, y_lengths = torch.tensor([9, 6, 3, 1]), torch.tensor([47, 33, 32, 40])
    x = torch.randint(0, A.NET["n_vocab"], (B, T_x))
    y = torch.randn(B, A.NET["spec_channels"], T_y)
    sid = torch.tensor([0, 2, 1, 1]) if n_speakers else None
    with torch.no_grad(), Recorder() as rec:
        _, l_length, attn, _, x_mask, _, _, (hidden_x, logw, logw_) = net(x, x_lengths, y, y_lengths, sid=sid)
    # the posterior encoder's randn_like, then (SDP) the likelihood's and the reverse pass's torch.randn(B, 2, T_x)
    assert len(rec.draws) == (3 if use_sdp else 1) and rec.draws[0].shape == (B, A.NET["inter_channels"], T_y)
    r = dict(x=x, x_lengths=x_lengths, y=y, y_lengths=y_lengths, e_post=rec.draws[0], l_length=l_length, attn=attn.to(torch.int8), logw=logw,
             logw_=logw_, hidden_x=hidden_x)
    if use_sdp:
        assert rec.draws[1].shape == rec.draws[2].shape == (B, 2, T_x)
        r["e_q"], r["e_w"] = rec.draws[1], rec.draws[2]
    if sid is not None:
        r["sid"] = sid
    for k, v in r.items():
        out[f"{name}/{k}"] = v.numpy()
    assert l_length.shape == (B,) and x_mask.sum() == x_lengths.sum()
    meta["models"][name] = dict(use_sdp=use_sdp, n_speakers=n_speakers, gin_channels=gin, seeds=seeds,
                                checksums={part: checksum(getattr(net, part)) for part in seeds}, loss_dur=float(l_length.sum()))


def main():
    meta = {"width": W, "lengths": [9, 5, 1], "yardstick_max": YARD_MAX, "net": A.NET, "models": {}}
    predictors(meta)
    model_case(meta, "model_sdp", True, 0, 110)
    model_case(meta, "model_dp", False, 0, 120)
    model_case(meta, "model_sdp_g", True, 3, 130)
    np.savez_compressed(os.path.join(HERE, "durnll_small.npz"), **out)
    with open(os.path.join(HERE, "durnll_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(os.path.getsize(os.path.join(HERE, "durnll_small.npz")), "bytes", json.dumps(meta["sdp"]), json.dumps(meta["c192_t150"]))
    import shutil

    shutil.rmtree(A.TMP, ignore_errors=True)


if __name__ == "__main__":
    main()
