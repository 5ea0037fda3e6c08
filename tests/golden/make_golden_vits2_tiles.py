#!/usr/bin/env python3
"""Golden vectors for the modules of tests/vits2_tile_cases.py (the VITS2 row GEMMs on every tile and K-walk length), produced by the
reference's own models.TextEncoder, ResidualCouplingTransformersBlock (both directions) and PosteriorEncoder on CPU in fp32 at the
corner table's small layout (B = 3, T = 37, lengths 37 / 18 / 1): what shows that the fp64 restatements the GPU test judges by are the
reference at these dims.  models.py imports monotonic_align at module level, which none of them uses: a stub module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vits2_tiles.py <path to the reference's vits2 directory>

No weight and no input is stored: both sides fill the modules from the seeds and gains of the case tables and draw the inputs from
vits2_tile_cases.inputs.  Writes tests/golden/vits2_tiles.npz + vits2_tiles_meta.json:
  te/<case>/{x, m, logs}   TextEncoder(ids, lengths, g=g)
  flow/<case>/{rev, fwd}   flow(z, mask, g=g, reverse=True) and flow(z, mask, g=g)
  post/<case>/{z, m, logs} PosteriorEncoder(y, lengths, g=g) with the recipe's eps as its draw
each as the elements at stride 13 of the flattened tensor (as vits2_dims_corners.npz keeps its big cases), and in the meta JSON, per
case, the table's row, the output shapes, each output's largest |.| and `ratio`: the reference's fp32 outputs against the fp64
restatement on the same state dict as a fraction of the bar, max |a - b| / (1e-5 + 1e-4 |b|) over every element of every output.  A
case whose ratio exceeds 0.5 is refused: the case's gain is what to lower then.  The zip members carry a fixed date, so a second run
writes the same bytes."""
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

import vits2_tile_cases as K  # noqa: E402

torch.set_num_threads(8)
RTOL, ATOL = 1e-4, 1e-5
RATIO_MAX = 0.5
out = {}


def ratio_close(a, b):
    """fp32 a against fp64 b as a fraction of the rtol / atol bar."""
    return float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max())


def with_draw(draw, fn):
    """fn() with torch.randn_like returning `draw` (PosteriorEncoder.forward draws torch.randn_like(m))."""
    real = torch.randn_like
    torch.randn_like = lambda *a, **k: draw.clone()
    try:
        return fn()
    finally:
        torch.randn_like = real


def reference_outputs(fam, mod, i):
    mask = K.mask_of(K.SMALL)
    with torch.no_grad():
        if fam == "te":
            x, m, logs, _ = mod(i["ids"], i["lengths"], g=i["g"])
            return dict(x=x, m=m, logs=logs)
        if fam == "flow":
            return dict(rev=mod(i["z"], mask, g=i["g"], reverse=True), fwd=mod(i["z"], mask, g=i["g"], reverse=False))
        z, m, logs, _ = with_draw(i["eps"], lambda: mod(i["y"], i["lengths"], g=i["g"]))
        return dict(z=z, m=m, logs=logs)


def main():
    meta = {"ratio_max": RATIO_MAX, "stride": K.STRIDE, "layout": [K.SMALL[0], K.SMALL[1], list(K.SMALL[2])], "te": {}, "flow": {}, "post": {}}
    for fam, name in K.CASES:
        c = K.FAMILIES[fam][name]
        mod = K.make(models, fam, name)
        i = K.inputs(fam, name, K.SMALL)
        outs = reference_outputs(fam, mod, i)
        with torch.no_grad():
            ref = K.restatement(fam, name, K.state(mod), i, K.SMALL[1])
        rec = dict(c, shapes={}, abs_max={}, ratios={}, n_tensors=len(mod.state_dict()))
        for k in K.OUTPUTS[fam]:
            v, r = outs[k], ref[k]
            assert v.shape == r.shape and v.dtype == torch.float32 and r.dtype == torch.float64, (name, k)
            for b, n in enumerate(K.SMALL[2]):  # padded frames are exactly zero on both sides
                assert float(v[b, :, n:].abs().sum()) == 0.0 and float(r[b, :, n:].abs().sum()) == 0.0, (name, k, b)
            out[f"{fam}/{name}/{k}"] = v.reshape(-1)[::K.STRIDE].numpy().copy()
            rec["shapes"][k], rec["abs_max"][k], rec["ratios"][k] = list(v.shape), float(v.abs().max()), ratio_close(v, r)
        rec["ratio"] = max(rec["ratios"].values())
        meta[fam][name] = rec
        print(name, json.dumps(rec["ratios"]), json.dumps(rec["abs_max"]))
    bad = {n: r["ratios"] for fam in ("te", "flow", "post") for n, r in meta[fam].items() if not r["ratio"] <= RATIO_MAX}
    if bad:
        raise SystemExit(f"cases whose reference fp32 lies beyond {RATIO_MAX} of the bar: {bad}")
    path = os.path.join(HERE, "vits2_tiles.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:  # np.savez_compressed's format with a fixed date on every member
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    with open(os.path.join(HERE, "vits2_tiles_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
