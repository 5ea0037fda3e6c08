#!/usr/bin/env python3
"""Times the VITS2 HiFi-GAN generator (models.py:900-974) at the ModelConfig dims: the HIP library (torch_tts_amd.Generator) in exact
fp32 and in split-fp16 - the two modes in one process, alternating in rounds - and the same module written with F.conv1d /
F.conv_transpose1d on the same GPU in fp32 (what a user runs today).  Reports ms per call (the median of the rounds) and the
spread between the rounds of one mode, mel-frames/s, audio-seconds/s at 22.05 kHz and the share of the matrix pipe: for f32 the
algorithmic FLOPs against the fp32 matrix peak (157.3 TFLOP/s), for split_f16 the three fp16 products it issues per algorithmic
product against the fp16 matrix peak (2516.8 TFLOP/s dense).
Usage: python tools/time_generator.py [--batch 64] [--frames 600] [--precision f32 split_f16] [--rounds 5] [--min-seconds 1.0] [--skip-torch]"""
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
warnings.filterwarnings("ignore", category=FutureWarning)
import torch_tts_amd as T  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3  # MI355X, fp32-input MFMA
FP16_MATRIX_TFLOPS = 16 * FP32_MATRIX_TFLOPS  # fp16 MFMA, dense: 16 x the fp32-input rate (~2.5 PFLOP/s)
SAMPLE_RATE = 22050
DIMS = dict(initial_channel=192, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
            upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4], gin_channels=0)


def generator_flops(d, T):
    """Algorithmic FLOPs (2 per multiply-add) of one utterance of T frames: 368.9 GFLOP at the ModelConfig dims, T = 600."""
    C0 = d["upsample_initial_channel"]
    f = 2 * T * C0 * d["initial_channel"] * 7  # conv_pre
    Ts, Cin = T, C0
    for i, (u, k) in enumerate(zip(d["upsample_rates"], d["upsample_kernel_sizes"])):
        C = C0 >> (i + 1)
        f += 2 * Ts * Cin * C * k  # ConvTranspose1d: every input frame meets k kernel taps per (in, out) pair
        Ts *= u
        f += sum(6 * 2 * Ts * C * C * kr for kr in d["resblock_kernel_sizes"])  # 3 x (c1, c2) per ResBlock1
        Cin = C
    return f + 2 * Ts * Cin * 7  # conv_post


def torch_forward(gen, x):
    """Generator.forward with torch functional ops (fp32, the weights of `gen`)."""
    w = lambda m: torch._weight_norm(m.weight_v, m.weight_g, 0) if hasattr(m, "weight_g") else m.weight  # noqa: E731
    x = F.conv1d(x, gen.conv_pre.weight, gen.conv_pre.bias, padding=3)
    nk = gen.num_kernels
    for i, (u, k) in enumerate(zip(DIMS["upsample_rates"], DIMS["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, w(gen.ups[i]), gen.ups[i].bias, stride=u, padding=(k - u) // 2)
        xs = None
        for j in range(nk):
            rb = gen.resblocks[i * nk + j]
            xr = x
            for c1, c2 in zip(rb.convs1, rb.convs2):
                xt = F.conv1d(F.leaky_relu(xr, 0.1), w(c1), c1.bias, dilation=c1.dilation, padding=c1.padding)
                xr = F.conv1d(F.leaky_relu(xt, 0.1), w(c2), c2.bias, padding=c2.padding) + xr
            xs = xr if xs is None else xs + xr
        x = xs / nk
    return torch.tanh(F.conv1d(F.leaky_relu(x), gen.conv_post.weight, padding=3))


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
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--precision", nargs="+", choices=["f32", "split_f16"], default=["f32", "split_f16"])
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per mode, the modes alternating (--min-seconds is one mode's total)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    gen = T.Generator(**DIMS)
    with torch.no_grad():  # O(1) activations (tests/test_generator_host.py scaled_weights)
        for n, p in gen.named_parameters():
            if n.endswith("weight_g"):
                p.uniform_(0.6, 1.0)
            elif n.endswith("weight_v") or n.endswith("weight"):
                fan_in = p[0].numel() if not n.startswith("ups") else p.shape[0] * p.shape[2]
                p.normal_(0.0, fan_in**-0.5)
            else:
                p.normal_(0.0, 0.1)
    gen = gen.to(dev).eval()
    Tn = args.frames
    up = 256
    flop = generator_flops(DIMS, Tn)
    for B in args.batch:
        z = torch.randn(B, DIMS["initial_channel"], Tn, device=dev)
        rows = {}
        def hip(mode):
            gen.precision = mode
            return gen(z)

        def rates(ms):
            return dict(mel_frames_per_s=round(B * Tn / ms * 1e3, 1), audio_s_per_s=round(B * Tn * up / SAMPLE_RATE / ms * 1e3, 1))

        with torch.no_grad():
            per = {m: [] for m in args.precision}
            for _ in range(args.rounds):  # f32, split_f16, f32, ...: drift of the clocks lands on both modes alike
                for m in args.precision:
                    per[m].append(time_call(lambda: hip(m), args.min_seconds / args.rounds))
            for m, windows in per.items():
                ms = statistics.median(w[0] for w in windows)
                rows["hip" if m == "f32" else "hip_split_f16"] = dict(
                    ms_per_call=round(ms, 3), ms_rounds=[round(w[0], 3) for w in windows], spread_ms=round(max(w[0] for w in windows) - min(w[0] for w in windows), 3),
                    calls=sum(w[1] for w in windows), **rates(ms),
                    **(dict(fp32_pipe_fraction=round(B * flop / (ms * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4)) if m == "f32" else
                       dict(fp16_pipe_fraction=round(3 * B * flop / (ms * 1e-3) / (FP16_MATRIX_TFLOPS * 1e12), 4))))
            if len(per) == 2:
                rows["f32_over_split_f16"] = round(rows["hip"]["ms_per_call"] / rows["hip_split_f16"]["ms_per_call"], 3)
                rows["max_abs_diff_split_f16_vs_f32"] = (hip("split_f16") - hip("f32")).abs().max().item()
            if not args.skip_torch:
                ms, n = time_call(lambda: torch_forward(gen, z), args.min_seconds)
                rows["torch_ops"] = dict(ms_per_call=round(ms, 3), calls=n, **rates(ms),
                                         fp32_pipe_fraction=round(B * flop / (ms * 1e-3) / (FP32_MATRIX_TFLOPS * 1e12), 4))
                rows["max_abs_diff_hip_vs_torch"] = (hip("f32") - torch_forward(gen, z)).abs().max().item()
            gen.precision = "f32"
        print(json.dumps(dict(B=B, T=Tn, gflop_per_utterance=round(flop / 1e9, 2), **rows)), flush=True)


if __name__ == "__main__":
    main()
