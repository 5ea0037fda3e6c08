#!/usr/bin/env python3
"""Times the VITS2 waveform discriminators (models.py:977-1110): MultiPeriodDiscriminator(y, y_hat) in the HIP library
(torch_tts_amd.MultiPeriodDiscriminator, exact fp32) and the same module written with F.conv1d / F.conv2d on the same GPU in fp32
(what a user runs today; its weight-normed weights are folded once, outside the timed window), the two alternating in rounds in
one process.  Two shapes: one pair of 22050 samples (a second of audio to score) and 64 pairs of 8192 samples (the training
segment).  Reports ms per call (the median of the rounds) and the spread between the rounds, samples/s, and the algorithmic
FLOPs of the call against the fp32 matrix peak (157.3 TFLOP/s) - a whole-call rate, launch gaps and the direct kernels included,
not a kernel's share of peak.
Usage: python tools/time_vits2_disc.py [--shapes 1x22050 64x8192] [--rounds 5] [--min-seconds 1.0] [--skip-torch]"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore", category=FutureWarning)
import recipes  # noqa: E402
import torch_tts_amd as T  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3  # MI355X, fp32-input MFMA


def disc_flops(eng, T_):
    """Algorithmic FLOPs (2 per multiply-add) of one row of T_ samples through one discriminator, and the part in its dense convs."""
    total = dense = 0
    Ci = 1
    for i, ((Co, k, _), H) in enumerate(zip(eng.layers, eng.heights(T_))):
        grouped = eng.dims["period"] == 0 and 1 <= i <= 4  # DiscriminatorS convs.1-4: 4 input channels per group
        cin_per_out = 4 if grouped else Ci
        f = 2 * eng.p * H * Co * k * cin_per_out
        total += f
        if not grouped and Ci >= 32 and Co > 1:
            dense += f
        Ci = Co
    return total, dense


def fold_weights(mpd):
    """[(weights, biases)] per discriminator: the effective weights of convs and conv_post."""
    out = []
    for d in mpd.discriminators:
        convs = list(d.convs) + [d.conv_post]
        out.append(([torch._weight_norm(c.weight_v, c.weight_g, 0).contiguous() for c in convs], [c.bias for c in convs]))
    return out


def torch_disc(d, period, ws, bs, x):
    fmap = []
    if period == 0:
        for i, (stride, groups, pad) in enumerate([(1, 1, 7), (4, 4, 20), (4, 16, 20), (4, 64, 20), (4, 256, 20), (1, 1, 2)]):
            x = F.leaky_relu(F.conv1d(x, ws[i], bs[i], stride=stride, padding=pad, groups=groups), 0.1)
            fmap.append(x)
        x = F.conv1d(x, ws[6], bs[6], padding=1)
    else:
        b, c, t = x.shape
        if t % period:
            x = F.pad(x, (0, period - t % period), "reflect")
        x = x.view(b, c, -1, period)
        for i in range(5):
            x = F.leaky_relu(F.conv2d(x, ws[i], bs[i], stride=(3 if i < 4 else 1, 1), padding=(2, 0)), 0.1)
            fmap.append(x)
        x = F.conv2d(x, ws[5], bs[5], padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def torch_forward(folded, y, y_hat):
    """MultiPeriodDiscriminator.forward with torch functional ops, as the reference runs it: each member on y, then on y_hat."""
    outs = [[], [], [], []]
    for d, (period, (ws, bs)) in enumerate(zip([0, 2, 3, 5, 7, 11], folded)):
        s_r, f_r = torch_disc(d, period, ws, bs, y)
        s_g, f_g = torch_disc(d, period, ws, bs, y_hat)
        for lst, v in zip(outs, (s_r, s_g, f_r, f_g)):
            lst.append(v)
    return outs


def time_call(fn, min_seconds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    n = max(1, int(min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x22050", "64x8192"], help="pairs x samples")
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed seconds per path and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per path, the paths alternating")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    mpd = T.MultiPeriodDiscriminator()
    recipes.fill_by_key(mpd, 31, gain=1.2)  # O(1) activations (tests/test_disc_hip.py)
    mpd = mpd.to(dev).eval()
    with torch.no_grad():
        folded = fold_weights(mpd)
    engines = [T.vits2.DiscEngine(d._cfg, None) for d in mpd.discriminators]
    for shape in args.shapes:
        B, Tn = (int(v) for v in shape.split("x"))
        y, y_hat = torch.randn(B, 1, Tn, device=dev), torch.randn(B, 1, Tn, device=dev)
        flop = 2 * B * sum(disc_flops(e, Tn)[0] for e in engines)
        dense = 2 * B * sum(disc_flops(e, Tn)[1] for e in engines)
        paths = {"hip": lambda: mpd(y, y_hat)}
        if not args.skip_torch:
            paths["torch_ops"] = lambda: torch_forward(folded, y, y_hat)
        rows = {}
        with torch.no_grad():
            per = {n: [] for n in paths}
            for _ in range(args.rounds):  # hip, torch, hip, ...: drift of the clocks lands on both alike
                for n, fn in paths.items():
                    per[n].append(time_call(fn, args.min_seconds / args.rounds))
            for n, windows in per.items():
                ms = statistics.median(w[0] for w in windows)
                rows[n] = dict(ms_per_call=round(ms, 3), ms_rounds=[round(w[0], 3) for w in windows],
                               spread_ms=round(max(w[0] for w in windows) - min(w[0] for w in windows), 3), calls=sum(w[1] for w in windows),
                               samples_per_s=round(2 * B * Tn / ms * 1e3, 1), fp32_peak_fraction=round(flop / (ms * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4))
            if "torch_ops" in rows:
                rows["torch_over_hip"] = round(rows["torch_ops"]["ms_per_call"] / rows["hip"]["ms_per_call"], 3)
                a, b = mpd(y, y_hat), torch_forward(folded, y, y_hat)
                rows["max_abs_diff_scores"] = max((u - v).abs().max().item() for la, lb in zip(a[:2], b[:2]) for u, v in zip(la, lb))
                rows["max_abs_diff_fmaps"] = max((u - v).abs().max().item() for la, lb in zip(a[2:], b[2:]) for fa, fb in zip(la, lb) for u, v in zip(fa, fb))
        print(json.dumps(dict(pairs=B, T=Tn, gflop_per_call=round(flop / 1e9, 2), dense_conv_share=round(dense / flop, 4), **rows)), flush=True)


if __name__ == "__main__":
    main()
