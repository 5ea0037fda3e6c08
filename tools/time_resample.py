#!/usr/bin/env python3
"""Times sample-rate conversion on one GPU, the variants alternated in one process (median and min of the rounds, ms per call; every
timed region is `--reps` calls between two device events), at B utterances of `--seconds` s for 22050 / 44100 / 48000 -> 16000 Hz:
  hip_resample    audio.resample_native (ttsdec_resample: the table launch and the filter launch)
  torch_resample  audio.resample on the whole batch, as torch ops on the same GPU (the timing baseline, not an oracle)
and, at 44100 Hz, the chain into the mel (n_fft 1024, hop 256, 80 mels, 16 kHz):
  hip_encode      AudioFrontend.encode_native(sr=44100, spectrogram=False)
  torch_encode    AudioFrontend.encode(audio.resample(w, 44100, 16000), 16000) looped over the batch, as the reference has it
From the shapes: the algorithm's bytes (input plus output samples) and FLOPs (2 * taps per output, the dense polyphase filter as
torchaudio states it), the two floors at the 6.29 TB/s copy rate and the 157.3 TFLOP/s fp32 rate, which of them binds, and the share
of it the HIP call reaches; the spread between the repeats of one side is (max - min) over the median.
Usage: python tools/time_resample.py [--batch 1 64] [--seconds 10] [--rounds 15] [--reps 10] [--only-hip]"""
import argparse
import json
import math
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=FutureWarning)
from torch_tts_amd import audio as A  # noqa: E402
from tools.time_audio import COPY_RATE, stats  # noqa: E402
from tools.time_vits2_align import rounds  # noqa: E402

SR, N_FFT, HOP, N_MELS = 16000, 1024, 256, 80
RATES = (22050, 44100, 48000)
FP32_RATE = 157.3e12  # FLOP/s, the fp32 vector (= fp32-input matrix) peak of the MI355X


def repeated(fn, reps):
    def run():
        for _ in range(reps):
            fn()
    return run


def per_call(res, reps):
    return {k: [t / reps for t in v] for k, v in res.items()}


def floors(row, name, nbytes, flops):
    bytes_ms, flops_ms = 1e3 * nbytes / COPY_RATE, 1e3 * flops / FP32_RATE
    row["algorithmic_MB"] = round(nbytes / 1e6, 2)
    row["algorithmic_GFLOP"] = round(flops / 1e9, 3)
    row["bytes_floor_ms"] = round(bytes_ms, 5)
    row["flops_floor_ms"] = round(flops_ms, 5)
    row["binding_floor"] = "bytes" if bytes_ms >= flops_ms else "flops"
    row[f"{name}_share_of_floor"] = round(max(bytes_ms, flops_ms) / row[f"{name}_ms_median"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-hip", action="store_true", help="the native calls alone (for a profiler)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=SR, hop_length=HOP, win_length=N_FFT, num_mels=N_MELS, fmin=0, fmax=8000), dev)
    for B in args.batch:
        for rate in RATES:
            N = int(round(args.seconds * rate))
            wave = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
            o, n, _, _, taps = A._resample_plan(rate, SR, 6, 0.99, "time_resample")
            n_out = -(-n * N // o)
            out, counts = A.resample_native(wave, rate, SR)
            assert out.shape == (B, n_out) and int(counts.min()) == n_out
            fns = {"hip_resample": lambda: A.resample_native(wave, rate, SR)}
            if not args.only_hip:
                ref = A.resample(wave, rate, SR)
                err = float((out - ref).abs().max() / ref.abs().max())  # (same result, before any time is compared)
                assert err < 1e-5, err
                fns["torch_resample"] = lambda: A.resample(wave, rate, SR)
            res = per_call(rounds({k: repeated(f, args.reps) for k, f in fns.items()}, args.rounds), args.reps)
            row = dict(stage="resample", B=B, seconds=args.seconds, orig_freq=rate, new_freq=SR, o=o, n=n, taps=taps, reps=args.reps)
            stats(res, row)
            floors(row, "hip_resample", 4 * B * (N + n_out), 2 * taps * B * n_out)
            if not args.only_hip:
                row["hip_over_torch"] = round(row["hip_resample_ms_median"] / row["torch_resample_ms_median"], 4)
            print(json.dumps(row), flush=True)
        # the chain into the mel at 44100 Hz
        rate = 44100
        N = int(round(args.seconds * rate))
        wave = (torch.rand(B, N, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev)
        o, n, _, _, taps = A._resample_plan(rate, SR, 6, 0.99, "time_resample")
        n_out = -(-n * N // o)
        T = 1 + n_out // HOP
        _, M_db, frames = fe.encode_native(wave, spectrogram=False, sr=rate)
        assert M_db.shape == (B, T, N_MELS) and int(frames.min()) == T
        fns = {"hip_encode": lambda: fe.encode_native(wave, spectrogram=False, sr=rate)}
        if not args.only_hip:
            fns["torch_encode"] = lambda: [fe.encode(A.resample(w, rate, SR), SR) for w in wave]
        res = per_call(rounds({k: repeated(f, args.reps) for k, f in fns.items()}, args.rounds), args.reps)
        row = dict(stage="resample_encode", B=B, seconds=args.seconds, orig_freq=rate, new_freq=SR, frames=T, n_fft=N_FFT, hop=HOP, n_mels=N_MELS,
                   reps=args.reps)
        stats(res, row)
        # input samples, the resampled wave written and read once, the mel written; the filter's and (5 N log2 N per frame) the FFT's FLOPs
        floors(row, "hip_encode", 4 * B * (N + 2 * n_out + T * N_MELS), 2 * taps * B * n_out + B * T * 5 * N_FFT * int(math.log2(N_FFT)))
        if not args.only_hip:
            row["hip_over_torch"] = round(row["hip_encode_ms_median"] / row["torch_encode_ms_median"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
