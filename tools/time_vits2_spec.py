#!/usr/bin/env python3
"""Times the VITS2 spectrogram front-end on one GPU, the variants alternated in one process (median and min of the rounds, ms per
call), at B utterances of `frames` frames, n_fft 1024, hop 256, 80 mels:
  hip_spec / hip_mel / hip_spec_to_mel       mel_processing.spectrogram_torch / mel_spectrogram_torch / spec_to_mel_torch
  torch_spec / torch_mel / torch_spec_to_mel the reference's lines (mel_processing.py:58-187) as torch ops on the same GPU, on the whole
                                             batch at once (rocFFT through torch.stft; this mirrors at the batch's end, not at each
                                             utterance's - it is the timing baseline, not an oracle)
and from the shapes the algorithmic bytes (waveforms read once, the result written once), the floor at the 6.29 TB/s copy rate, the
share of it the HIP call reaches, and the spread between the repeats of one side (max - min over the median).
Usage: python tools/time_vits2_spec.py [--batch 64] [--frames 600] [--rounds 15]"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=FutureWarning)
from torch_tts_amd import mel_processing as MP  # noqa: E402
from tools.time_vits2_align import rounds  # noqa: E402

SR, N_FFT, HOP, N_MELS = 22050, 1024, 256, 80
COPY_RATE = 6.29e12  # B/s, the measured copy rate of the MI355X


def torch_spec(y, window):
    pad = int((N_FFT - HOP) / 2)
    yp = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    s = torch.stft(yp, N_FFT, hop_length=HOP, win_length=N_FFT, window=window, center=False, pad_mode="reflect", normalized=False,
                   onesided=True, return_complex=True)
    return torch.sqrt(torch.view_as_real(s).pow(2).sum(-1) + 1e-6)


def torch_mel_of(spec, basis):
    return torch.log(torch.clamp(torch.matmul(basis, spec), min=1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    B, T = args.batch, args.frames
    N = T * HOP
    y = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) * 1.8 - 0.9).to(dev)
    window = MP.hann(N_FFT, dev)
    basis = MP.default_mel_basis(N_FFT, N_MELS, SR, 0.0, None, dev)
    spec = MP.spectrogram_torch(y, N_FFT, SR, HOP, N_FFT)
    assert spec.shape == (B, N_FFT // 2 + 1, T)
    fns = {
        "hip_spec": lambda: MP.spectrogram_torch(y, N_FFT, SR, HOP, N_FFT),
        "torch_spec": lambda: torch_spec(y, window),
        "hip_mel": lambda: MP.mel_spectrogram_torch(y, N_FFT, N_MELS, SR, HOP, N_FFT, 0.0, None),
        "torch_mel": lambda: torch_mel_of(torch_spec(y, window), basis),
        "hip_spec_to_mel": lambda: MP.spec_to_mel_torch(spec, N_FFT, N_MELS, SR, 0.0, None),
        "torch_spec_to_mel": lambda: torch_mel_of(spec, basis),
    }
    d_spec = float((spec - torch_spec(y, window)).abs().max() / spec.max())
    res = rounds(fns, args.rounds)
    row = dict(stage="spec", B=B, frames=T, n_fft=N_FFT, hop=HOP, n_mels=N_MELS, spec_max_abs_diff_hip_vs_torch_over_max=d_spec)
    for k, v in res.items():
        row[f"{k}_ms_median"] = round(statistics.median(v), 4)
        row[f"{k}_ms_min"] = round(min(v), 4)
        row[f"{k}_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
    nbytes = dict(spec=4 * B * (N + (N_FFT // 2 + 1) * T), mel=4 * B * (N + N_MELS * T), spec_to_mel=4 * B * T * (N_FFT // 2 + 1 + N_MELS))
    for k, nb in nbytes.items():
        floor_ms = 1e3 * nb / COPY_RATE
        row[f"{k}_algorithmic_MB"] = round(nb / 1e6, 2)
        row[f"{k}_floor_ms"] = round(floor_ms, 4)
        row[f"hip_{k}_share_of_floor"] = round(floor_ms / statistics.median(res[f"hip_{k}"]), 3)
        row[f"hip_{k}_over_torch"] = round(statistics.median(res[f"hip_{k}"]) / statistics.median(res[f"torch_{k}"]), 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
