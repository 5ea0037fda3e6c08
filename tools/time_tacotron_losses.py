#!/usr/bin/env python3
"""Times the loss terms of the Tacotron validation step - one fused ttsdec_val_losses call (csrc/valstep.hip through
torch_tts_amd.engine.Engine.val_losses) - against the same terms as torch ops on the same GPU (the forms of
torch_tts_amd.autograd_path under no_grad, composed as the reference's run_training_step and TacotronTask.train_forward compose
them), the two paths alternating in rounds in one process:

  fused      y, y_post, x [B, T, D], s [B, T], w [B, S, L], lengths -> terms [16]: the masked and unmasked mel and difference terms of
             y and y_post, the stop BCE, alignment_std_loss and alignment_max_loss
  torch_ops  mel_loss_fn(y, x, xmask), mel_loss_fn(y_post, x, xmask), the four difference terms on y.diff / y_post.diff / x.diff
             (unmasked and under xmask[:, 1:]), binary_cross_entropy_with_logits, alignment_std_loss, alignment_max_loss

at 64 and 256 utterances x 600 frames x 80 mels, r = 1 (600 steps), L = 120, ragged lengths.  Reports ms per call (the median of the
rounds), the spread between the rounds, the largest relative difference of the two paths' terms, and the fused call's algorithmic
bytes (3 B T D + B T + B S L floats: every operand once) with the time those bytes take at the HBM rate a float4 copy reaches on
this chip (6.29 TB/s) and its share of the measured time.
Usage: python tools/time_tacotron_losses.py [--batches 64 256] [--rounds 5] [--min-seconds 1.0]"""
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
import torch_tts_amd as T  # noqa: E402
from torch_tts_amd import autograd_path as AP  # noqa: E402

T_FRAMES, D_MEL, L_MEM = 600, 80, 120
HBM = 6.29e12  # bytes/s of a float4 copy on this chip


def torch_terms(y, y_post, x, s, w, lengths):
    xmask = (torch.arange(y.shape[1], device=y.device)[None, :] < lengths[:, None]).unsqueeze(2)
    dy, dp, dx = y.diff(dim=1), y_post.diff(dim=1), x.diff(dim=1)
    return torch.stack([
        AP.mel_loss_fn(y, x, xmask, 1), AP.mel_loss_fn(y_post, x, xmask, 1),
        AP.mel_loss_fn(dy, dx, None, 1), AP.mel_loss_fn(dp, dx, None, 1),
        AP.mel_loss_fn(dy, dx, xmask[:, 1:], 1), AP.mel_loss_fn(dp, dx, xmask[:, 1:], 1),
        AP.stop_loss(s, lengths, 0.1), AP.alignment_std_loss(w), AP.alignment_max_loss(w)])


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


def rounds(paths, n_rounds, min_seconds):
    per = {n: [] for n in paths}
    for _ in range(n_rounds):  # a, b, a, ...: drift of the clocks lands on every path alike
        for n, fn in paths.items():
            per[n].append(time_call(fn, min_seconds / n_rounds))
    return {n: dict(ms_per_call=round(statistics.median(v[0] for v in w), 4), ms_rounds=[round(v[0], 4) for v in w],
                    spread_ms=round(max(v[0] for v in w) - min(v[0] for v in w), 4), calls=sum(v[1] for v in w)) for n, w in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 256])
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed seconds per path and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per path, the paths alternating")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = T.tacotron._engine(dev)
    for B in args.batches:
        gen = torch.Generator().manual_seed(B)
        with torch.no_grad():
            x = (0.5 * torch.randn(B, T_FRAMES, D_MEL, generator=gen) + 0.2).to(dev)
            y = x + (0.3 * torch.randn(B, T_FRAMES, D_MEL, generator=gen)).to(dev)
            y_post = x + (0.2 * torch.randn(B, T_FRAMES, D_MEL, generator=gen)).to(dev)
            s = (4.0 * torch.randn(B, T_FRAMES, generator=gen)).to(dev)
            w = torch.softmax(2.0 * torch.randn(B, T_FRAMES, L_MEM, generator=gen), dim=2).to(dev)
            lengths = torch.linspace(T_FRAMES, T_FRAMES // 2, B).round().to(torch.int32).to(dev)  # ragged, the longest first
            row = rounds({"fused": lambda: eng.val_losses(y, y_post, x, s, w, lengths, 0.1),
                          "torch_ops": lambda: torch_terms(y, y_post, x, s, w, lengths)}, args.rounds, args.min_seconds)
            a, b = eng.val_losses(y, y_post, x, s, w, lengths, 0.1)[1][:9].double(), torch_terms(y, y_post, x, s, w, lengths).double()
            nbytes = 4 * (3 * B * T_FRAMES * D_MEL + B * T_FRAMES + B * T_FRAMES * L_MEM)
            us = nbytes / HBM * 1e6
            row["fused"].update(algorithmic_bytes=nbytes, hbm_floor_us=round(us, 2), share_of_hbm_floor=round(us / (row["fused"]["ms_per_call"] * 1e3), 4))
            row.update(utterances=B, T=T_FRAMES, D=D_MEL, S=T_FRAMES, L=L_MEM, frames=int(lengths.sum()),
                       torch_over_fused=round(row["torch_ops"]["ms_per_call"] / row["fused"]["ms_per_call"], 3),
                       max_rel_diff=float(((a - b).abs() / b.abs()).max()))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
