#!/usr/bin/env python3
"""Times the mel -> waveform step on one GPU, the variants alternated in one process (median and min of the rounds, ms per call), at B
utterances of `frames` mel frames, n_fft 1024, hop 256, 80 mels, 32 iterations:
  hip_synth / hip_gl / hip_mel        audio.synth_audio_native / griffinlim_native / AudioFrontend.mel_to_magnitude
  torch_synth / torch_gl / torch_mel  audio.synth_audio (utterance by utterance, as the reference has it) / audio.griffinlim on the whole
                                      batch / the mel_inv chain on the whole batch, as torch ops on the same GPU (the timing baseline,
                                      not an oracle)
and from the shapes the algorithmic bytes of the native path's design (per frame and iteration the frame-major magnitude
and two spectra read, the windowed inverse frames written and read once, one spectrum written), the floor at the 6.29 TB/s copy
rate, the share of it the HIP call reaches, and the spread between the repeats of one side (max - min over the median).
--analysis times the opposite direction, waveform -> dB spectrogram / mel, by the same protocol, at B utterances of
hop * (frames - 1) samples:
  hip_mel_only / hip_mel_spec         AudioFrontend.encode_native(spectrogram=False) / (spectrogram=True)
  torch_encode                        AudioFrontend.encode looped over the batch, as torch ops on the same GPU (the timing baseline)
with the call's byte floor: the waveform read once plus the outputs written.
Usage: python tools/time_audio.py [--analysis] [--batch 64] [--frames 600] [--rounds 15] [--only-hip]"""
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
from torch_tts_amd import audio as A  # noqa: E402
from tools.time_vits2_align import rounds  # noqa: E402

SR, N_FFT, HOP, N_MELS, N_ITER = 22050, 1024, 256, 80, 32
COPY_RATE = 6.29e12  # B/s, the measured copy rate of the MI355X


def stats(res, row):
    for k, v in res.items():
        row[f"{k}_ms_median"] = round(statistics.median(v), 4)
        row[f"{k}_ms_min"] = round(min(v), 4)
        row[f"{k}_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)


def analysis(args, dev):
    """waveform -> dB spectrogram / mel: the two forms of the native call against the torch-op encode, utterance by utterance."""
    B, T = args.batch, args.frames
    bins = N_FFT // 2 + 1
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=SR, hop_length=HOP, win_length=N_FFT, num_mels=N_MELS, fmin=0, fmax=8000), dev)
    n = HOP * (T - 1)
    wave = (torch.rand(B, n, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    D_db, M_db, frames = fe.encode_native(wave)
    assert D_db.shape == (B, T, bins) and M_db.shape == (B, T, N_MELS) and int(frames.min()) == T
    fns = {
        "hip_mel_only": lambda: fe.encode_native(wave, spectrogram=False),
        "hip_mel_spec": lambda: fe.encode_native(wave),
    }
    if not args.only_hip:
        fns["torch_encode"] = lambda: [fe.encode(w, SR) for w in wave]
    res = rounds(fns, args.rounds)
    row = dict(stage="analysis", B=B, frames=T, n_fft=N_FFT, hop=HOP, n_mels=N_MELS)
    stats(res, row)
    for k, nb in dict(mel_only=4 * B * (n + T * N_MELS), mel_spec=4 * B * (n + T * (N_MELS + bins))).items():
        floor_ms = 1e3 * nb / COPY_RATE
        row[f"{k}_algorithmic_MB"] = round(nb / 1e6, 2)
        row[f"{k}_floor_ms"] = round(floor_ms, 5)
        row[f"hip_{k}_share_of_floor"] = round(floor_ms / statistics.median(res[f"hip_{k}"]), 4)
        if not args.only_hip:
            row[f"hip_{k}_over_torch"] = round(statistics.median(res[f"hip_{k}"]) / statistics.median(res["torch_encode"]), 4)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--analysis", action="store_true", help="time waveform -> dB spectrogram / mel instead of mel -> waveform")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--only-hip", action="store_true", help="the native calls alone (for a profiler)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.analysis:
        return analysis(args, dev)
    B, T = args.batch, args.frames
    bins = N_FFT // 2 + 1
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=SR, hop_length=HOP, win_length=N_FFT, num_mels=N_MELS, fmin=0, fmax=8000), dev)
    # a mel with the range the model emits: the dB of a random positive spectrum through the filterbank
    g = torch.Generator().manual_seed(1)
    S = (torch.rand(B, bins, T, generator=g) ** 4).to(dev)
    y = A.m_fwd(A.amplitude_to_db(fe.stft_to_mels(S), 10, 1e-12, 0).mT).contiguous()
    mag = fe.mel_to_magnitude(y)
    assert mag.shape == (B, bins, T)
    fns = {
        "hip_synth": lambda: A.synth_audio_native(y, fe),
        "hip_gl": lambda: A.griffinlim_native(mag, N_FFT, HOP, N_FFT, n_iter=N_ITER),
        "hip_mel": lambda: fe.mel_to_magnitude(y),
    }
    if not args.only_hip:
        fns.update({
            "torch_synth": lambda: A.synth_audio(y, fe),
            "torch_gl": lambda: A.griffinlim(mag, N_FFT, HOP, N_FFT, power=1.0, n_iter=N_ITER),
            "torch_mel": lambda: A.db_to_amplitude(fe.mel_inv(A.m_rev(y)), 1, 1).pow(0.5),
        })
    res = rounds(fns, args.rounds)
    row = dict(stage="audio", B=B, frames=T, n_fft=N_FFT, hop=HOP, n_mels=N_MELS, n_iter=N_ITER)
    stats(res, row)
    per_iter = B * T * (4 * bins + 2 * 8 * bins + 2 * 4 * N_FFT + 8 * bins)
    last = B * T * (4 * bins + 2 * 8 * bins + 2 * 4 * N_FFT) + 4 * B * HOP * (T - 1)
    nbytes = dict(gl=N_ITER * per_iter + last + B * T * bins * (2 * 4 + 2 * 8), mel=4 * B * T * (N_MELS + bins))
    nbytes["synth"] = nbytes["gl"] + nbytes["mel"] + 2 * 4 * B * HOP * (T - 1)
    for k, nb in nbytes.items():
        floor_ms = 1e3 * nb / COPY_RATE
        row[f"{k}_algorithmic_MB"] = round(nb / 1e6, 2)
        row[f"{k}_floor_ms"] = round(floor_ms, 4)
        row[f"hip_{k}_share_of_floor"] = round(floor_ms / statistics.median(res[f"hip_{k}"]), 3)
        if not args.only_hip:
            row[f"hip_{k}_over_torch"] = round(statistics.median(res[f"hip_{k}"]) / statistics.median(res[f"torch_{k}"]), 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
