#!/usr/bin/env python3
"""Times VITS2 monotonic alignment search at the ModelConfig width on one GPU, the variants alternated in one process (median and min
of the rounds, ms per call), at B utterances of `frames` x `tokens`, C = 192:
  hip_neg_cent       ttsvits_neg_cent alone (no host read)
  hip_mas            ttsvits_maximum_path on a given neg_cent: search, frame_token, dur, dense fp32 path, the status read
  hip_align          vits2.align: both, from [B, C, T] operands
  hip_forced         vits2.forced_alignment: enc_p, enc_q (80 -> 192, 16 WN layers), flow forward, align
  torch_ops_copies   for comparison on the same GPU: neg_cent in torch ops (models.py:1226-1239), then what the reference's wrapper
                     does around its CPU search - neg_cent to the host, a same-sized path back - WITHOUT the search itself: a lower
                     bound of the reference's procedure
and the search's time per row (hip_mas at B = 1 without the dense path, over `frames`): the length of the dependence chain.
Usage: python tools/time_vits2_align.py [--batch 64] [--frames 600] [--tokens 150] [--rounds 15]"""
import argparse
import json
import math
import os
import statistics
import sys
import warnings

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=FutureWarning)
import torch_tts_amd as T  # noqa: E402

V = T.vits2
SPEC, INTER, HIDDEN, GIN = 80, 192, 192, 256


def torch_neg_cent(z_p, m_p, logs_p):
    s = torch.exp(-2 * logs_p)
    return (torch.sum(-0.5 * math.log(2 * math.pi) - logs_p, [1], keepdim=True) + torch.matmul(-0.5 * (z_p**2).transpose(1, 2), s)
            + torch.matmul(z_p.transpose(1, 2), m_p * s) + torch.sum(-0.5 * (m_p**2) * s, [1], keepdim=True))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.enc_p = V.TextEncoder(178, INTER, HIDDEN, 768, 2, 6, 3, 0.1)
        self.enc_q = V.PosteriorEncoder(SPEC, INTER, HIDDEN, 5, 1, 16, gin_channels=GIN)
        self.flow = V.ResidualCouplingTransformersBlock(INTER, HIDDEN, 5, 1, 4, gin_channels=GIN, use_transformer_flows=True)
        self.emb_g = nn.Embedding(4, GIN)


def build(dev):
    torch.manual_seed(0)
    net = Net()
    with torch.no_grad():  # O(1) activations
        for n, p in net.named_parameters():
            if n.endswith("gamma"):
                p.normal_(1.0, 0.1)
            elif n.endswith("weight_g"):
                p.uniform_(0.6, 1.0)
            elif p.dim() >= 2 and "emb" not in n:
                p.normal_(0.0, p[0].numel() ** -0.5)
            else:
                p.normal_(0.0, 0.1)
        net.enc_q.proj.weight.mul_(0.1)
    return net.to(dev).eval()


def rounds(fns, n_rounds):
    """Alternates the variants: per round one timed call of each (after two warm-up calls each) -> {name: [ms, ...]}."""
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--tokens", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    net = build(dev)
    B, Ty, Tx = args.batch, args.frames, args.tokens
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        z_p = torch.randn(B, INTER, Ty, generator=gen).to(dev)
        m_p = torch.randn(B, INTER, Tx, generator=gen).to(dev)
        logs_p = (torch.rand(B, INTER, Tx, generator=gen) * 4.5 - 3.5).to(dev)
        x_mask, y_mask = torch.ones(B, 1, Tx, device=dev), torch.ones(B, 1, Ty, device=dev)
        t_y = torch.full((B,), Ty, dtype=torch.int32, device=dev)
        t_x = torch.full((B,), Tx, dtype=torch.int32, device=dev)
        cl = [t.transpose(1, 2).contiguous() for t in (z_p, m_p, logs_p)]
        eng = V._align_engine(dev)
        nc = eng.neg_cent(*cl, t_y, t_x)
        ids = torch.randint(0, 178, (B, Tx), generator=gen).to(dev)
        y = torch.randn(B, SPEC, Ty, generator=gen).to(dev)
        sid = (torch.arange(B) % 4).to(dev)
        e_q = torch.randn(B, INTER, Ty, generator=gen).to(dev)

        def copies():
            n = torch_neg_cent(z_p, m_p, logs_p)
            host = n.data.cpu().numpy()  # the wrapper's first line (a synchronising copy)
            return torch.from_numpy(host).to(device=dev, dtype=n.dtype)  # its last: the path, same size, back

        fns = {
            "hip_neg_cent": lambda: eng.neg_cent(*cl, t_y, t_x),
            "hip_mas": lambda: eng.maximum_path(nc, t_y, t_x),
            "hip_mas_no_dense_path": lambda: eng.maximum_path(nc, t_y, t_x, None),
            "hip_align": lambda: V.align(z_p, m_p, logs_p, x_mask, y_mask),
            "hip_forced": lambda: V.forced_alignment(net, ids, t_x, y, t_y, sid=sid, noise=e_q),
            "torch_ops_copies": copies,
        }
        diff = float((nc - torch_neg_cent(z_p, m_p, logs_p)).abs().max() / nc.abs().max())
        res = rounds(fns, args.rounds)
    row = dict(stage="align", B=B, frames=Ty, tokens=Tx, C=INTER, neg_cent_max_abs_diff_hip_vs_torch_over_max=diff)
    for k, v in res.items():
        row[f"{k}_ms_median"] = round(statistics.median(v), 4)
        row[f"{k}_ms_min"] = round(min(v), 4)
    row["mas_us_per_row_median"] = round(1e3 * statistics.median(res["hip_mas_no_dense_path"]) / Ty, 4)
    row["mas_us_per_row_min"] = round(1e3 * min(res["hip_mas_no_dense_path"]) / Ty, 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
