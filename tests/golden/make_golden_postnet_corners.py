#!/usr/bin/env python3
"""Golden vectors for the corners of the dims that the Tacotron Postnets and Encoder2 accept (tests/postnet_corner_cases.py),
produced by the reference's own modules.modules.MelPostnet, modules.modules.MelPostnet2 and encoder.Encoder2 on CPU in fp32, eval
mode.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_postnet_corners.py [<path to the reference's tacotron directory>]

No weight is stored: both sides fill the modules from the seeds of the case tables.  Every shape of every case whose output holds
at most postnet_corner_cases.GOLDEN_MAX_ELEMENTS elements is run.  Writes tests/golden/postnet_corners.npz +
postnet_corners_meta.json:
  post/<case>/B<B>T<T>/{x13, y}        the elements at stride 13 of the flattened seeded input [B, T, d] (the input itself is the
                                       table's recipe: the sample shows that this machine draws what the golden script drew) and
                                       the reference's output [B, T, d]
  enc/<case>/<i>/{ids, lengths, memory}   ENC_SHAPES[i]: token ids [B, L], lengths [B], the reference's memory [B, max(lengths), d_out]
and in the meta JSON, per entry, the output's shape and `ratio`: the reference's fp32 result against the fp64 oracle
(oracle/tacotron_oracle.py on .double() weights and inputs) as a fraction of the bar the GPU tests hold the kernels to,
max |a - b| / (1e-5 + 1e-4 |b|).  An entry whose ratio exceeds 0.5 would let the bar judge the case rather than a kernel: the script
refuses to write it.  The zip members carry a fixed date, so a second run writes the same bytes."""
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
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/tacotron"  # (the default of make_golden_taco2.py / make_golden_encoder.py)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from encoder import Encoder2  # noqa: E402
from modules.modules import MelPostnet, MelPostnet2  # noqa: E402

import postnet_corner_cases as K  # noqa: E402

torch.set_num_threads(8)
RTOL, ATOL = 1e-4, 1e-5
RATIO_MAX = 0.5
STRIDE = 13
ref = types.SimpleNamespace(MelPostnet=MelPostnet, MelPostnet2=MelPostnet2, Encoder2=Encoder2)


def ratio_close(a, b):
    """fp32 a against fp64 b as a fraction of the rtol / atol bar."""
    assert b.dtype == torch.float64 and a.shape == b.shape
    return float(((a.double() - b).abs() / (ATOL + RTOL * b.abs())).max())


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
    meta = {"ratio_max": RATIO_MAX, "stride": STRIDE, "max_elements": K.GOLDEN_MAX_ELEMENTS, "post": {}, "enc": {},
            "dims": {n: list(K.case(n)["dims"]) for t in (K.MEL_CASES, K.MEL2_CASES, K.ENC_CASES) for n in t},
            "seeds": {n: K.case(n)["seed"] for t in (K.MEL_CASES, K.MEL2_CASES, K.ENC_CASES) for n in t}}
    modules = {}
    for name, B, T in K.postnet_shapes(golden_only=True):
        if name not in modules:
            modules[name] = (K.make_module(ref, name), K.weights(name))
        mod, wts = modules[name]
        x = K.postnet_input(name, B, T)
        with torch.no_grad():
            y = mod(x)
        key = f"{name}/B{B}T{T}"
        out[f"post/{key}/x13"], out[f"post/{key}/y"] = x.reshape(-1)[::STRIDE].numpy().copy(), y.numpy()
        meta["post"][key] = {"shape": list(y.shape), "ratio": ratio_close(y, K.postnet_oracle(name, x, wts, torch.float64)),
                             "y_minus_x_rms": float((y - x).pow(2).mean().sqrt())}
    for name in K.ENC_CASES:
        mod, wts = K.make_module(ref, name), K.weights(name)
        for i in range(len(K.ENC_SHAPES)):
            ids, lengths = K.encoder_input(name, i)
            with torch.no_grad():
                mem = mod(ids, lengths)
            key = f"{name}/{i}"
            out[f"enc/{key}/ids"], out[f"enc/{key}/lengths"], out[f"enc/{key}/memory"] = ids.numpy(), lengths.numpy(), mem.numpy()
            meta["enc"][key] = {"shape": list(mem.shape), "ratio": ratio_close(mem, K.encoder_oracle(name, ids, lengths, wts, torch.float64))}
    ratios = {f"{fam}/{k}": v["ratio"] for fam in ("post", "enc") for k, v in meta[fam].items()}
    print(json.dumps(ratios, indent=1))
    bad = {k: v for k, v in ratios.items() if not v <= RATIO_MAX}
    if bad:
        raise SystemExit(f"entries whose reference fp32 lies beyond {RATIO_MAX} of the bar: {bad}")
    write_npz(os.path.join(HERE, "postnet_corners.npz"), out)
    with open(os.path.join(HERE, "postnet_corners_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print(os.path.getsize(os.path.join(HERE, "postnet_corners.npz")), "bytes")


if __name__ == "__main__":
    main()
