#!/usr/bin/env python3
"""Times the style encoder (VAE at the reference's widths, 80 mels) on one GPU at B utterances of `frames` mel frames: the HIP path
(ttsenc_style_forward) against the SAME module's `_stock_forward` - plain torch ops on the same GPU, the timing baseline, not an
oracle - both in eval mode under no_grad, alternated in one process.  A timed window is `inner` back-to-back calls between two device
events (one call is a few hundred microseconds: too short a window on its own); per side the median and min of the rounds in ms per
call and the spread between them ((max - min) / median).  From the shapes: the algorithm's operations (conv stages, input projection,
recurrence) and bytes (input read, every activation written once and read once, weights read once), the larger of the two floors at
the exact-fp32 matrix peak and the measured copy rate, and the share of that floor the HIP call reaches - an end-to-end figure over
~20 launches, not a kernel's share of peak.  Lengths are ragged: the HIP path takes them as a device tensor and never reads them
back; the stock path takes them on the host, where pack_padded_sequence wants them.
Usage: python tools/time_style.py [--batch 64] [--frames 600] [--rounds 15] [--inner 20] [--only-hip]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_tts_amd as T  # noqa: E402
from tools.time_vits2_align import rounds  # noqa: E402

N_MELS = 80
F32_MFMA_PEAK = 157.3e12  # FLOP/s, exact-fp32 matrix instructions (MI355X_MICROARCH.md)
COPY_RATE = 6.29e12       # B/s, the measured copy rate of the MI355X


def algorithm(m, B, frames):
    """(FLOP, bytes) of one forward from the shapes."""
    t, f, cin = frames, N_MELS, 1
    flop, nbytes = 0, 4 * B * frames * N_MELS
    for conv in m.encoder.convs:
        t, f, co = (t - 1) // 2 + 1, (f - 1) // 2 + 1, conv.out_channels
        flop += 2 * B * t * f * co * 9 * cin
        nbytes += 4 * (2 * B * t * f * co + 9 * cin * co)  # written once, read once by the next stage; the weights
        cin = co
    H, feat = m.encoder.gru.hidden_size, cin * f
    flop += 2 * B * t * 4 * H * (feat + H)
    nbytes += 4 * (2 * B * t * 4 * H + 4 * H * (feat + H))
    return flop, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    m = T.VAE(num_mels=N_MELS, dim_vae=16).to(dev).eval()
    B, frames = args.batch, args.frames
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(frames // 2, frames + 1, (B,), generator=g)
    lengths[0] = frames
    x = torch.randn(B, frames, N_MELS, generator=g)
    for b, n in enumerate(lengths.tolist()):
        x[b, n:] = 0
    x, eps = x.to(dev), torch.randn(B, 16, generator=g).to(dev)
    lengths_dev = lengths.to(dev)

    def many(fn):
        def run():
            with torch.no_grad():
                for _ in range(args.inner):
                    fn()
        return run

    with torch.no_grad():
        assert m._hip_ok(x)
        xo, extra = m(x, lengths_dev, eps)
        xs, extra_s = m._stock_forward(x, lengths, eps)
    err = float((xo - xs).abs().max()), float((extra["kl"] - extra_s["kl"]).abs().max())
    fns = {"hip": many(lambda: m(x, lengths_dev, eps))}
    if not args.only_hip:
        fns["torch"] = many(lambda: m._stock_forward(x, lengths, eps))
    res = {k: [v / args.inner for v in vs] for k, vs in rounds(fns, args.rounds).items()}
    flop, nbytes = algorithm(m, B, frames)
    floor_ms = 1e3 * max(flop / F32_MFMA_PEAK, nbytes / COPY_RATE)
    row = dict(stage="style_vae", B=B, frames=frames, n_mels=N_MELS, inner=args.inner, rounds=args.rounds,
               max_abs_x_hip_minus_torch=err[0], max_abs_kl_hip_minus_torch=err[1])
    for k, v in res.items():
        row[f"{k}_ms_median"] = round(statistics.median(v), 4)
        row[f"{k}_ms_min"] = round(min(v), 4)
        row[f"{k}_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
    row.update(algorithmic_GFLOP=round(flop / 1e9, 3), algorithmic_MB=round(nbytes / 1e6, 2), floor_ms=round(floor_ms, 5),
               floor_bound="flop" if flop / F32_MFMA_PEAK > nbytes / COPY_RATE else "bytes",
               hip_share_of_floor=round(floor_ms / statistics.median(res["hip"]), 4))
    if "torch" in res:
        row["hip_over_torch"] = round(statistics.median(res["hip"]) / statistics.median(res["torch"]), 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
