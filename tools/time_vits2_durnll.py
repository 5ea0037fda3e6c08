#!/usr/bin/env python3
"""Times the VITS2 duration likelihood (models.py:78-125): StochasticDurationPredictor.nll(x, x_mask, w) in the HIP library
(torch_tts_amd.StochasticDurationPredictor, exact fp32, 32 launches without g) and the same likelihood written with torch ops on the
same GPU in fp32 (F.conv1d, F.layer_norm between transposes as modules.LayerNorm does it, F.gelu, softmax / cumsum / gather for the
spline; the spline is evaluated for every token and the tails selected by torch.where, so the torch path has no host read either -
the reference's boolean indexing would add one per flow), the two alternating in rounds in one process, the same draw e_q given to
both.  C = 192, n_flows = 4; two shapes: one utterance of 150 tokens and a batch of 64 x 150 tokens with ragged lengths.  Reports ms
per call (the median of the rounds), the spread between the rounds, tokens/s, and the largest difference of the two paths' nll
(the project's metric |a - b| / (0.1 + |b|)).
Usage: python tools/time_vits2_durnll.py [--shapes 1x150 64x150] [--rounds 5] [--min-seconds 1.0] [--skip-torch]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_tts_amd as T  # noqa: E402
from test_duration_host import randomize  # noqa: E402

CH = 192


def _norm(sd, name, x):  # modules.LayerNorm.forward
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), sd[name + ".gamma"], sd[name + ".beta"], 1e-5).transpose(1, -1)


def _dds(sd, p, x, m, g=None):
    if g is not None:
        x = x + g
    for i in range(3):
        d = 3**i
        y = F.conv1d(x * m, sd[f"{p}.convs_sep.{i}.weight"], sd[f"{p}.convs_sep.{i}.bias"], dilation=d, padding=d, groups=x.shape[1])
        y = F.gelu(_norm(sd, f"{p}.norms_1.{i}", y))
        y = F.conv1d(y, sd[f"{p}.convs_1x1.{i}.weight"], sd[f"{p}.convs_1x1.{i}.bias"])
        x = x + F.gelu(_norm(sd, f"{p}.norms_2.{i}", y))
    return x * m


def _spline(x, uw, uh, ud, tail=5.0, mn=1e-3):
    """x [B, 1, T], uw / uh [B, 1, T, 10], ud [B, 1, T, 9] -> (y, log |dy/dx|); linear tails by torch.where."""
    inside = (x >= -tail) & (x <= tail)
    xi = x.clamp(-tail, tail)
    ud = F.pad(ud, (1, 1), value=math.log(math.exp(1 - mn) - 1))

    def knots(u):
        k = F.pad(torch.cumsum(mn + (1 - mn * 10) * F.softmax(u, dim=-1), -1), (1, 0))
        k = 2 * tail * k - tail
        k[..., 0], k[..., -1] = -tail, tail
        return k

    kx, ky, d = knots(uw), knots(uh), mn + F.softplus(ud)
    edges = kx.clone()
    edges[..., -1] += 1e-6
    idx = (torch.sum(xi[..., None] >= edges, dim=-1) - 1)[..., None]
    at = lambda t: t.gather(-1, idx)[..., 0]  # noqa: E731
    xk, wk, yk, hk = at(kx), at(kx[..., 1:] - kx[..., :-1]), at(ky), at(ky[..., 1:] - ky[..., :-1])
    sk, dk, dk1 = hk / wk, at(d), at(d[..., 1:])
    th = (xi - xk) / wk
    tt = th * (1 - th)
    den = sk + (dk + dk1 - 2 * sk) * tt
    y = yk + hk * (sk * th.pow(2) + dk * tt) / den
    lad = torch.log(sk.pow(2) * (dk1 * th.pow(2) + 2 * sk * tt + dk * (1 - th).pow(2))) - 2 * torch.log(den)
    return torch.where(inside, y, x), torch.where(inside, lad, torch.zeros_like(lad))


def _conv_flow(sd, p, z, m, g):
    x0, x1 = z[:, :1], z[:, 1:]
    h = F.conv1d(x0, sd[p + ".pre.weight"], sd[p + ".pre.bias"])
    h = _dds(sd, p + ".convs", h, m, g)
    h = F.conv1d(h, sd[p + ".proj.weight"], sd[p + ".proj.bias"]) * m
    B, _, Tn = x0.shape
    h = h.reshape(B, 1, -1, Tn).permute(0, 1, 3, 2)
    s = math.sqrt(sd[p + ".pre.weight"].shape[0])
    y1, lad = _spline(x1, h[..., :10] / s, h[..., 10:20] / s, h[..., 20:])
    return torch.cat([x0, y1], 1) * m, torch.sum(lad * m, [1, 2])


def torch_nll(sd, x, m, w, e_q, n_flows=4):
    """forward(x, x_mask, w) as the reference writes it (eval mode), on the state dict's tensors."""
    x = F.conv1d(x, sd["pre.weight"], sd["pre.bias"])
    x = F.conv1d(_dds(sd, "convs", x, m), sd["proj.weight"], sd["proj.bias"]) * m
    h_w = F.conv1d(w, sd["post_pre.weight"], sd["post_pre.bias"])
    h_w = F.conv1d(_dds(sd, "post_convs", h_w, m), sd["post_proj.weight"], sd["post_proj.bias"]) * m
    e_q = e_q * m
    z_q = (sd["post_flows.0.m"] + torch.exp(sd["post_flows.0.logs"]) * e_q) * m
    ldq = torch.sum(sd["post_flows.0.logs"] * m, [1, 2])
    for k in range(4):
        z_q, ld = _conv_flow(sd, f"post_flows.{2 * k + 1}", z_q, m, x + h_w)
        z_q, ldq = torch.flip(z_q, [1]), ldq + ld
    z_u, z1 = z_q[:, :1], z_q[:, 1:]
    z0 = (w - torch.sigmoid(z_u) * m) * m
    ldq = ldq + torch.sum((F.logsigmoid(z_u) + F.logsigmoid(-z_u)) * m, [1, 2])
    logq = torch.sum(-0.5 * (math.log(2 * math.pi) + e_q**2) * m, [1, 2]) - ldq
    y0 = torch.log(torch.clamp_min(z0, 1e-5)) * m
    ld_tot = torch.sum(-y0, [1, 2])
    z = (sd["flows.0.m"] + torch.exp(sd["flows.0.logs"]) * torch.cat([y0, z1], 1)) * m
    ld_tot = ld_tot + torch.sum(sd["flows.0.logs"] * m, [1, 2])
    for k in range(n_flows):
        z, ld = _conv_flow(sd, f"flows.{2 * k + 1}", z, m, x)
        z, ld_tot = torch.flip(z, [1]), ld_tot + ld
    return torch.sum(0.5 * (math.log(2 * math.pi) + z**2) * m, [1, 2]) - ld_tot + logq


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
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed seconds per path and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per path, the paths alternating")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    sdp = randomize(T.StochasticDurationPredictor(CH, 192, 3, 0.5, 4), 7).to(dev).eval()
    sd = {k: v.detach() for k, v in sdp.state_dict().items()}
    for shape in args.shapes:
        B, Tn = (int(v) for v in shape.split("x"))
        lengths = torch.linspace(Tn, max(1, Tn // 2), B).round().long() if B > 1 else torch.tensor([Tn])  # ragged, the longest first
        tokens = int(lengths.sum())
        m = (torch.arange(Tn)[None, :] < lengths[:, None]).unsqueeze(1).float().to(dev)
        x = torch.randn(B, CH, Tn, device=dev) * m
        w = torch.randint(1, 13, (B, 1, Tn), device=dev).float() * m
        e_q = torch.randn(B, 2, Tn, device=dev)
        paths = {"hip": lambda: sdp.nll(x, m, w, noise=e_q)}
        if not args.skip_torch:
            paths["torch_ops"] = lambda: torch_nll(sd, x, m, w, e_q)
        rows = {}
        with torch.no_grad():
            per = {n: [] for n in paths}
            for _ in range(args.rounds):  # hip, torch, hip, ...: drift of the clocks lands on both alike
                for n, fn in paths.items():
                    per[n].append(time_call(fn, args.min_seconds / args.rounds))
            for n, windows in per.items():
                ms = statistics.median(v[0] for v in windows)
                rows[n] = dict(ms_per_call=round(ms, 4), ms_rounds=[round(v[0], 4) for v in windows],
                               spread_ms=round(max(v[0] for v in windows) - min(v[0] for v in windows), 4), calls=sum(v[1] for v in windows),
                               tokens_per_s=round(tokens / ms * 1e3, 1))
            if "torch_ops" in rows:
                rows["torch_over_hip"] = round(rows["torch_ops"]["ms_per_call"] / rows["hip"]["ms_per_call"], 3)
                a, b = sdp.nll(x, m, w, noise=e_q).double(), torch_nll(sd, x, m, w, e_q).double()
                rows["max_rel_diff_nll"] = float(((a - b).abs() / (0.1 + b.abs())).max())
        print(json.dumps(dict(utterances=B, T=Tn, tokens=tokens, **rows)), flush=True)


if __name__ == "__main__":
    main()
