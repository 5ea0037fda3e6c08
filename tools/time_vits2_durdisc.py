#!/usr/bin/env python3
"""Times the VITS2 duration discriminators (models.py:183-329): DurationDiscriminatorV1 / V2 forward(x, x_mask, dur_r, dur_hat)
in the HIP library (torch_tts_amd.DurationDiscriminatorV1 / V2, exact fp32) and the same module written with torch ops on the same
GPU in fp32 (what a user runs today: F.conv1d, F.layer_norm between transposes as modules.LayerNorm does it, torch.cat, the
mask multiplications, F.linear, sigmoid), the two alternating in rounds in one process.  C = F = 192; two shapes: one utterance
of 150 tokens and a training batch of 64 x 150 tokens with ragged lengths.  Reports ms per call (the median of the rounds) and the
spread between the rounds, tokens/s, and the call's multiply-adds: the reference's eight F x F x 3 conv passes' worth and the five the
HIP path runs, the latter against the fp32 matrix peak (157.3 TFLOP/s) - a whole-call rate, launch gaps and row kernels included, not
a kernel's share of peak.
Usage: python tools/time_vits2_durdisc.py [--shapes 1x150 64x150] [--rounds 5] [--min-seconds 1.0] [--skip-torch] [--versions 1 2]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recipes  # noqa: E402
import torch_tts_amd as T  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3  # MI355X, fp32-input MFMA
CH = 192


def _norm(sd, name, x):  # modules.LayerNorm.forward (modules.py:24-27)
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), sd[name + ".gamma"], sd[name + ".beta"], 1e-5).transpose(1, -1)


def _conv(sd, name, x):
    return F.conv1d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1)


def torch_forward(sd, v2, x, m, dur_r, dur_hat):
    """forward and forward_probability as the reference writes them (eval mode), on the state dict's tensors."""
    h = _conv(sd, "conv_1", x * m)
    if v2:
        h = _norm(sd, "norm_1", torch.relu(h))
    h = _conv(sd, "conv_2", h * m)
    if v2:
        h = _norm(sd, "norm_2", torch.relu(h))
    out = []
    for dur in (dur_r, dur_hat):
        d = F.conv1d(dur, sd["dur_proj.weight"], sd["dur_proj.bias"])
        u = _conv(sd, "pre_out_conv_1", torch.cat([h, d], dim=1) * m)
        if v2:
            u = _norm(sd, "pre_out_norm_1", torch.relu(u))
        u = _conv(sd, "pre_out_conv_2", u * m)
        if v2:
            u = _norm(sd, "pre_out_norm_2", torch.relu(u))
        p = torch.sigmoid(F.linear((u * m).transpose(1, 2), sd["output_layer.0.weight"], sd["output_layer.0.bias"]))
        out.append([p] if v2 else p)
    return out


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
    ap.add_argument("--shapes", nargs="+", default=["1x150", "64x150"], help="utterances x tokens")
    ap.add_argument("--versions", nargs="+", type=int, default=[1, 2])
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed seconds per path and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per path, the paths alternating")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    for version in args.versions:
        net = (T.DurationDiscriminatorV1 if version == 1 else T.DurationDiscriminatorV2)(CH, CH, 3, 0.1)
        recipes.fill_by_key(net, 47, gain=1.2)  # O(1) logits (tests/golden/make_golden_durdisc.py)
        net = net.to(dev).eval()
        sd = {k: v.detach() for k, v in net.state_dict().items()}
        for shape in args.shapes:
            B, Tn = (int(v) for v in shape.split("x"))
            lengths = torch.linspace(Tn, max(1, Tn // 2), B).round().long() if B > 1 else torch.tensor([Tn])  # ragged, the longest first
            tokens = int(lengths.sum())
            m = (torch.arange(Tn)[None, :] < lengths[:, None]).unsqueeze(1).float().to(dev)
            x = torch.randn(B, CH, Tn, device=dev) * m
            dur_r = torch.log(torch.randint(1, 8, (B, 1, Tn), device=dev).float()) * m
            dur_hat = 0.8 + 0.7 * torch.randn(B, 1, Tn, device=dev)
            mac_pass = B * Tn * CH * CH * 3  # one F x F x 3 conv over the padded batch
            paths = {"hip": lambda: net(x, m, dur_r, dur_hat)}
            if not args.skip_torch:
                paths["torch_ops"] = lambda: torch_forward(sd, version == 2, x, m, dur_r, dur_hat)
            rows = {}
            with torch.no_grad():
                per = {n: [] for n in paths}
                for _ in range(args.rounds):  # hip, torch, hip, ...: drift of the clocks lands on both alike
                    for n, fn in paths.items():
                        per[n].append(time_call(fn, args.min_seconds / args.rounds))
                for n, windows in per.items():
                    ms = statistics.median(w[0] for w in windows)
                    rows[n] = dict(ms_per_call=round(ms, 4), ms_rounds=[round(w[0], 4) for w in windows],
                                   spread_ms=round(max(w[0] for w in windows) - min(w[0] for w in windows), 4), calls=sum(w[1] for w in windows),
                                   tokens_per_s=round(tokens / ms * 1e3, 1))
                rows["hip"]["fp32_peak_fraction"] = round(2 * 5 * mac_pass / (rows["hip"]["ms_per_call"] * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4)
                if "torch_ops" in rows:
                    rows["torch_over_hip"] = round(rows["torch_ops"]["ms_per_call"] / rows["hip"]["ms_per_call"], 3)
                    a, b = net(x, m, dur_r, dur_hat), torch_forward(sd, version == 2, x, m, dur_r, dur_hat)
                    flat = lambda o: [t for e in o for t in (e if isinstance(e, list) else [e])]  # noqa: E731
                    rows["max_abs_diff_prob"] = max((u - v).abs().max().item() for u, v in zip(flat(a), flat(b)))
            # (x 3 taps each) the reference: conv_1, conv_2, 2 x (pre_out_conv_1 over 2F channels, pre_out_conv_2) = 8 F x F passes;
            # the HIP path: conv_1, conv_2, one h half, pre_out_conv_2 over both durations = 5 passes
            print(json.dumps(dict(version=version, utterances=B, T=Tn, tokens=tokens, gflop_reference=round(2 * 8 * mac_pass / 1e9, 3),
                                  gflop_hip=round(2 * 5 * mac_pass / 1e9, 3), **rows)), flush=True)


if __name__ == "__main__":
    main()
