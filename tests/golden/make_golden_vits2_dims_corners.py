#!/usr/bin/env python3
"""Golden vectors for the corners of the dims that the text encoder, the coupling flow and the posterior encoder accept
(tests/vits2_dims_corner_cases.py), produced by the reference's own models.TextEncoder, ResidualCouplingTransformersBlock (both
directions) and PosteriorEncoder on CPU in fp32.  models.py imports monotonic_align at module level, which none of them uses: a stub
module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vits2_dims_corners.py <path to the reference's vits2 directory>

No weight is stored: both sides fill the modules from the seeds and gains of the case tables.  Writes
tests/golden/vits2_dims_corners.npz + vits2_dims_corners_meta.json:
  te/<E>/{ids, lengths, g}          the inputs;  te/<E>/{x, m, logs}   TextEncoder(ids, lengths, g=g)
  flow/<F>/{z, lengths, g}          the inputs;  flow/<F>/{rev, fwd}   flow(z, mask, g=g, reverse=True) and flow(z, mask, g=g)
  post/<Q>/{y, lengths, g, eps}     the inputs;  post/<Q>/{z, m, logs} PosteriorEncoder(y, lengths, g=g) with `eps` as its draw
(g only where the case has gin_channels; the outputs of E6, F5 and Q5 as the elements at stride 13 of the flattened tensor) and in the
meta JSON, per case, the table's row, the output shapes, each output's largest |.| and `ratio`: the reference's fp32 outputs against the
tests' fp64 restatement on the same state dict, as a fraction of the bar the GPU tests hold the kernels to,
max |a - b| / (1e-5 + 1e-4 |b|) over every element of every output (padded frames are exactly zero on both sides, which the script
checks apart).  A case whose ratio exceeds 0.5 would let the bar judge the case rather than a kernel: the script refuses to write it -
the case's gain (the table's) is what to lower then.  The zip members carry a fixed date, so a second run writes the same bytes."""
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

import vits2_dims_corner_cases as K  # noqa: E402

torch.set_num_threads(8)
RTOL, ATOL = 1e-4, 1e-5
RATIO_MAX = 0.5
out = {}


def ratio_close(a, b):
    """fp32 a against fp64 b as a fraction of the rtol / atol bar."""
    return float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max())


def state(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}


def with_draw(draw, fn):
    """fn() with torch.randn_like returning `draw` (PosteriorEncoder.forward draws torch.randn_like(m))."""
    real = torch.randn_like
    torch.randn_like = lambda *a, **k: draw.clone()
    try:
        return fn()
    finally:
        torch.randn_like = real


def padded_are_zero(c, *tensors):
    _, _, lengths = K.layout(c)
    return all(float(t[b, :, n:].abs().sum()) == 0.0 for t in tensors for b, n in enumerate(lengths))


def record(fam, name, c, inputs, outs, refs, n_tensors):
    """inputs / outs: name -> tensor (None: absent), refs: the fp64 restatement of each output, in outs' order"""
    for k, v in inputs.items():
        if v is not None:
            out[f"{fam}/{name}/{k}"] = v.numpy()
    rec = dict(c, shapes={}, abs_max={}, ratios={}, n_tensors=n_tensors)
    for (k, v), r in zip(outs.items(), refs):
        assert v.shape == r.shape and v.dtype == torch.float32 and r.dtype == torch.float64, (name, k)
        out[f"{fam}/{name}/{k}"] = (v.reshape(-1)[::K.STRIDE] if name in K.BIG else v).numpy().copy()
        rec["shapes"][k], rec["abs_max"][k], rec["ratios"][k] = list(v.shape), float(v.abs().max()), ratio_close(v, r)
    rec["ratio"] = max(rec["ratios"].values())
    assert padded_are_zero(c, *outs.values()) and padded_are_zero(c, *refs), name
    return rec


def text_encoders(meta):
    for name, c in K.TE_CASES.items():
        te = K.make_text_encoder(models, name)
        i = K.te_inputs(name)
        with torch.no_grad():
            x, m, logs, _ = te(i["ids"], i["lengths"], g=i["g"])
        meta["te"][name] = record("te", name, c, i, dict(x=x, m=m, logs=logs), K.te_ref64(name, state(te), i), len(state(te)))


def flows(meta):
    for name, c in K.FLOW_CASES.items():
        fl = K.make_flow(models, name)
        i = K.flow_inputs(name)
        mask = K.mask_of(c)
        with torch.no_grad():
            rev = fl(i["z"], mask, g=i["g"], reverse=True)
            fwd = fl(i["z"], mask, g=i["g"], reverse=False)
        meta["flow"][name] = record("flow", name, c, i, dict(rev=rev, fwd=fwd), K.flow_ref64(name, state(fl), i), len(state(fl)))


def posteriors(meta):
    for name, c in K.POST_CASES.items():
        pe = K.make_post(models, name)
        i = K.post_inputs(name)
        with torch.no_grad():
            z, m, logs, _ = with_draw(i["eps"], lambda: pe(i["y"], i["lengths"], g=i["g"]))
        meta["post"][name] = record("post", name, c, i, dict(z=z, m=m, logs=logs), K.post_ref64(name, state(pe), i), len(state(pe)))


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
    meta = {"ratio_max": RATIO_MAX, "stride": K.STRIDE, "big": list(K.BIG), "n_vocab": K.N_VOCAB, "window": K.WINDOW, "te": {}, "flow": {}, "post": {}}
    text_encoders(meta)
    flows(meta)
    posteriors(meta)
    ratios = {name: c["ratios"] for fam in ("te", "flow", "post") for name, c in meta[fam].items()}
    print(json.dumps(ratios, indent=1))
    print(json.dumps({name: c["abs_max"] for fam in ("te", "flow", "post") for name, c in meta[fam].items()}))
    bad = {name: r for name, r in ratios.items() if not max(r.values()) <= RATIO_MAX}
    if bad:
        raise SystemExit(f"cases whose reference fp32 lies beyond {RATIO_MAX} of the bar: {bad}")
    write_npz(os.path.join(HERE, "vits2_dims_corners.npz"), out)
    with open(os.path.join(HERE, "vits2_dims_corners_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "vits2_dims_corners.npz")), "bytes")


if __name__ == "__main__":
    main()
