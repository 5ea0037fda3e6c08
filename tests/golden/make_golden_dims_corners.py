#!/usr/bin/env python3
"""Golden vectors for the corners of the dims that the generator, the duration predictors and DiscriminatorP accept
(tests/dims_corner_cases.py), produced by the reference's own models.Generator, StochasticDurationPredictor, DurationPredictor and
DiscriminatorP on CPU in fp32.  models.py imports monotonic_align at module level, which none of them uses: a stub module stands
in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dims_corners.py <path to the reference's vits2 directory>

No weight is stored: both sides fill the modules from the seeds of the case tables.  Writes tests/golden/dims_corners.npz +
dims_corners_meta.json:
  gen/<G>/T<T>/{x, g, y}            inputs [2, C, T], [2, 4, 1] and the reference's waveform [2, 1, T * prod(u)]
  sdp/<D>/{x, x_mask, g, noise, w, e_q}   the operands of both directions (dims_corner_cases.dur_inputs)
  sdp/<D>/{logw, nll, z}            sdp(x, x_mask, g=g, reverse=True, noise_scale=2.0) with `noise` as its draw; sdp(x, x_mask, w, g=g)
                                    with `e_q` as its draw, and the last flow's output z
  dp/<DP>/{x, x_mask, g, logw}      DurationPredictor
  disc/<P>/{x, score, fmap/<l>}     the input [2, 1, T], every score, and the elements at stride 13 of each flattened feature map
and in the meta JSON, per case, shapes, each feature map's fp64 mean |.|, the waveform's saturated fraction, and `ratio`: the
reference's fp32 result against the tests' fp64 restatement as a fraction of the bar the GPU tests hold the kernels to
(max |a - b| / (1e-5 + 1e-4 |b|) for the generator - waveform and every stage's activated output, which forward pre-hooks on ups[i]
and conv_post read - the discriminators and the likelihood's z; max |a - b| / (0.1 + |b|) / 1e-4 for logw and nll).  A case whose
ratio exceeds 0.5 would let the bar judge the case rather than a kernel: the script refuses to write it.  The zip members carry a
fixed date, so a second run writes the same bytes."""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.modules.setdefault("monotonic_align", types.ModuleType("monotonic_align"))  # (imported by models.py, unused here)
import models  # noqa: E402

import dims_corner_cases as K  # noqa: E402
from test_disc_host import reference_disc  # noqa: E402
from test_duration_host import dp_forward, sdp_reverse  # noqa: E402
from test_durnll_host import sdp_nll  # noqa: E402
from test_generator_host import reference_forward  # noqa: E402

torch.set_num_threads(8)
RTOL, ATOL, REL = 1e-4, 1e-5, 1e-4
RATIO_MAX = 0.5
out = {}


def ratio_close(a, b):
    """fp32 a against fp64 b as a fraction of the rtol / atol bar."""
    return float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max())


def ratio_rel(a, b):
    return float(((a.double() - b).abs() / (0.1 + b.abs())).max()) / REL


def state(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}


def with_draw(draw, fn):
    """fn() with torch.randn returning `draw` (the way make_golden_duration.py gives the SDP its noise)."""
    real = torch.randn
    torch.randn = lambda *a, **k: draw.clone()
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.randn = real


def generators(meta):
    for name, c in K.GEN_CASES.items():
        gen = K.make_generator(models, name)
        sd, n_up = state(gen), len(c["dims"]["upsample_rates"])
        acts = []
        hooks = [m.register_forward_pre_hook(lambda mod, inp: acts.append(inp[0].detach().transpose(1, 2).clone()))
                 for m in list(gen.ups) + [gen.conv_post]]
        rec = {"dims": c["dims"], "gain": c["gain"], "seed": c["seed"], "T": {}}
        for T in c["T"]:
            x, g = K.gen_inputs(name, T)
            del acts[:]
            with torch.no_grad():
                y = gen(x, g)
            y64, acts64 = reference_forward(sd, c["dims"], x, g, stages=True)
            assert len(acts) == len(acts64) == n_up + 1
            out[f"gen/{name}/T{T}/x"], out[f"gen/{name}/T{T}/g"], out[f"gen/{name}/T{T}/y"] = x.numpy(), g.numpy(), y.numpy()
            rec["T"][str(T)] = {"shape": list(y.shape), "sat_frac": float((y.abs() > 0.99).float().mean()), "y_rms": float(y.pow(2).mean().sqrt()),
                                "ratio": ratio_close(y, y64), "stage_ratio": max(ratio_close(a, b) for a, b in zip(acts, acts64))}
        for h in hooks:
            h.remove()
        rec["n_tensors"] = len(sd)
        meta["gen"][name] = rec


def durations(meta):
    for name, c in K.SDP_CASES.items():
        sdp = K.make_sdp(models, name)
        sd, i = state(sdp), K.dur_inputs(c)
        logw = with_draw(i["noise"], lambda: sdp(i["x"], i["x_mask"], g=i["g"], reverse=True, noise_scale=K.DUR_NOISE_SCALE))
        got = {}
        hook = sdp.flows[-1].register_forward_hook(lambda m, inp, o: got.update(z=o[0].detach().clone()))  # (the last Flip's output)
        nll = with_draw(i["e_q"], lambda: sdp(i["x"], i["x_mask"], i["w"], g=i["g"]))
        hook.remove()
        z = got["z"]
        logw64 = sdp_reverse(sd, i["x"], i["x_mask"], i["noise"], K.DUR_NOISE_SCALE, i["g"], n_flows=c["n_flows"])
        ref = sdp_nll(sd, i["x"], i["x_mask"], i["w"], i["e_q"], i["g"], n_flows=c["n_flows"])
        for k, v in i.items():
            if v is not None:
                out[f"sdp/{name}/{k}"] = v.numpy()
        out[f"sdp/{name}/logw"], out[f"sdp/{name}/nll"], out[f"sdp/{name}/z"] = logw.numpy(), nll.numpy(), z.numpy()
        meta["sdp"][name] = dict(c, ratio_reverse=ratio_rel(logw, logw64), ratio_nll=ratio_rel(nll, ref["nll"]), ratio_z=ratio_close(z, ref["z"]),
                                 logw_abs_max=float(logw.abs().max()), n_tensors=len(sd))
    for name, c in K.DP_CASES.items():
        dp = K.make_dp(models, name)
        sd, i = state(dp), K.dur_inputs(c)
        with torch.no_grad():
            logw = dp(i["x"], i["x_mask"], g=i["g"])
        for k in ("x", "x_mask", "g"):
            if i[k] is not None:
                out[f"dp/{name}/{k}"] = i[k].numpy()
        out[f"dp/{name}/logw"] = logw.numpy()
        meta["dp"][name] = dict(c, ratio=ratio_rel(logw, dp_forward(sd, i["x"], i["x_mask"], i["g"])), logw_abs_max=float(logw.abs().max()))


def discriminators(meta):
    for name, c in K.DISC_CASES.items():
        disc = K.make_disc(models, name)
        sd, x = state(disc), K.disc_input(name)
        with torch.no_grad():
            score, fmap = disc(x)
        s64, f64 = reference_disc(sd, 1, x, period=c["period"], stride=c["stride"], prefix="")
        assert len(fmap) == len(f64) == 6
        out[f"disc/{name}/x"], out[f"disc/{name}/score"] = x.numpy(), score.numpy()
        rec = dict(c, fmaps=[], ratio_score=ratio_close(score, s64), n_params=sum(p.numel() for p in disc.parameters()))
        for l, (f, r) in enumerate(zip(fmap, f64)):
            out[f"disc/{name}/fmap/{l}"] = f.reshape(-1)[::K.DISC_STRIDE].numpy().copy()
            rec["fmaps"].append({"shape": list(f.shape), "mean_abs": float(r.abs().mean()), "ratio": ratio_close(f, r)})
        rec["ratio"] = max([rec["ratio_score"]] + [f["ratio"] for f in rec["fmaps"]])
        meta["disc"][name] = rec


def all_ratios(meta):
    r = {}
    for name, c in meta["gen"].items():
        for T, t in c["T"].items():
            r[f"{name}/T{T}"] = max(t["ratio"], t["stage_ratio"])
    for name, c in meta["sdp"].items():
        r[f"{name} reverse"], r[f"{name} nll"], r[f"{name} z"] = c["ratio_reverse"], c["ratio_nll"], c["ratio_z"]
    for fam in ("dp", "disc"):
        for name, c in meta[fam].items():
            r[name] = c["ratio"]
    return r


def write_npz(path, arrays):
    """np.savez_compressed's format with a fixed date on every member (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    meta = {"ratio_max": RATIO_MAX, "stride": K.DISC_STRIDE, "gen": {}, "sdp": {}, "dp": {}, "disc": {}}
    generators(meta)
    durations(meta)
    discriminators(meta)
    ratios = all_ratios(meta)
    print(json.dumps(ratios, indent=1))
    bad = {k: v for k, v in ratios.items() if not v <= RATIO_MAX}
    if bad:
        raise SystemExit(f"cases whose reference fp32 lies beyond {RATIO_MAX} of the bar: {bad}")
    write_npz(os.path.join(HERE, "dims_corners.npz"), out)
    with open(os.path.join(HERE, "dims_corners_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "dims_corners.npz")), "bytes")


if __name__ == "__main__":
    main()
