#!/usr/bin/env python3
"""Golden vectors for the corners of the dims that the style encoders accept (tests/style_corner_cases.py), produced by the
reference's own modules.style.ReferenceEncoder, VAE, GST and GST_VAE on the CPU in fp32, eval mode.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_style_corners.py <path to the reference's tacotron directory>

No weight is stored: both sides build and fill the modules from the seeds of the case table.  Writes
tests/golden/style_corners.npz + style_corners_meta.json:
  <case>/B<B>/{enc_out, x, kl, eps}   the reference's outputs of that layout (x and kl where the kind has them; in the reference's
                                      own shapes) and the draw that stood in for torch.randn_like while the module ran
  <case>/B<B>/x13                     the elements at stride 13 of the flattened seeded input (the input itself is the table's
                                      recipe: the sample shows that this machine draws what the golden script drew)
and in the meta JSON, per entry, the output shapes, each output's mean |.| and `ratio`: the reference's fp32 result against the
same module in .double() on the same inputs, as a fraction of the bar the GPU tests hold the kernels to,
max |a - b| / (1e-5 + 1e-4 |b|).  An entry whose ratio exceeds 0.25 would let the bar judge the case rather than a kernel: the
script refuses to write it.  The zip members carry a fixed date, so a second run writes the same bytes."""
import contextlib
import copy
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.dirname(HERE))
from modules import style as ref_style  # noqa: E402

import style_corner_cases as K  # noqa: E402

torch.set_num_threads(8)
RTOL, ATOL = 1e-4, 1e-5
RATIO_MAX = 0.25
STRIDE = 13


def ratio_close(a, b):
    """a against the fp64 b as a fraction of the rtol / atol bar."""
    assert b.dtype == torch.float64 and a.shape == b.shape
    return float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max())


def run(m, x, lengths, eps):
    """{"enc_out", "x", "kl"} (those the module has) of the reference's forward, with `eps` as its draw; its eval-mode prints dropped."""
    dt = next(m.parameters()).dtype
    x = x.to(dt)
    real = torch.randn_like
    if eps is not None:
        torch.randn_like = lambda t, *a, **k: eps.to(t.dtype).view_as(t).clone()
    try:
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            if isinstance(m, ref_style.ReferenceEncoder):
                return {"enc_out": m(x, lengths)}
            out = {"enc_out": m.encoder(x, lengths)}
            xo, extra = m(x, lengths)
            out["x"] = xo
            if "kl" in extra:
                out["kl"] = extra["kl"]
            return out
    finally:
        torch.randn_like = real


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
    out = {}
    meta = {"ratio_max": RATIO_MAX, "stride": STRIDE, "entries": {},
            "cases": {n: {k: v for k, v in c.items() if k not in ("layouts", "cycle")} for n, c in K.CASES.items()}}
    modules = {}
    for name, i in K.all_layouts():
        if name not in modules:
            m = K.make_module(ref_style, name)
            modules[name] = (m, copy.deepcopy(m).double())
        m32, m64 = modules[name]
        x, lengths, eps = K.inputs(name, i)
        got, ref = run(m32, x, lengths, eps), run(m64, x, lengths, eps)
        key = K.key(name, i)
        out[f"{key}/x13"] = x.reshape(-1)[::STRIDE].numpy().copy()
        if eps is not None:
            out[f"{key}/eps"] = eps.numpy()
        rec = {"layout": [x.shape[0], x.shape[1]], "lengths": lengths.tolist(), "shapes": {}, "abs_mean": {}, "ratios": {}}
        for k, v in got.items():
            assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), (key, k)
            out[f"{key}/{k}"] = v.numpy()
            rec["shapes"][k], rec["abs_mean"][k], rec["ratios"][k] = list(v.shape), float(ref[k].abs().mean()), ratio_close(v, ref[k])
        rec["ratio"] = max(rec["ratios"].values())
        meta["entries"][key] = rec
    print(json.dumps({k: v["ratios"] for k, v in meta["entries"].items()}, indent=1))
    print(json.dumps({k: v["abs_mean"] for k, v in meta["entries"].items()}))
    bad = {k: v["ratio"] for k, v in meta["entries"].items() if not v["ratio"] <= RATIO_MAX}
    if bad:
        raise SystemExit(f"entries whose reference fp32 lies beyond {RATIO_MAX} of the bar: {bad}")
    write_npz(os.path.join(HERE, "style_corners.npz"), out)
    with open(os.path.join(HERE, "style_corners_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "style_corners.npz")), "bytes")


if __name__ == "__main__":
    main()
