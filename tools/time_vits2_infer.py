#!/usr/bin/env python3
"""Times VITS2 inference at the ModelConfig dims on one GPU, the variants alternated in one process (median and min of the
rounds, ms per call):
  (a) sdp:   StochasticDurationPredictor reverse - the HIP library (torch_tts_amd.StochasticDurationPredictor, ttsdur_*) against the
             reference's algorithm in torch ops on the same GPU in fp32 (what a user runs today: the reference's module);
  (b) infer: ids -> waveform - torch_tts_amd.vits2.infer against SynthesizerTrn.infer's own sequence with the HIP enc_p / flow / dec
             but a torch-op duration predictor and the dense generate_path + two batched matmuls.
Usage: python tools/time_vits2_infer.py [--batch 1 64] [--tokens 150] [--rounds 15] [--only sdp-hip --iters 20]  (the last:
just the HIP SDP, for a rocprofv3 --kernel-trace --stats run)"""
import argparse
import json
import math
import os
import statistics
import sys
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=FutureWarning)
import torch_tts_amd as T  # noqa: E402

V = T.vits2
FULL = dict(n_vocab=100, inter=192, hidden=192, filter=768, n_heads=2, n_layers=6, kernel=3)
GEN = dict(resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2],
           upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])


# ---- the reference's StochasticDurationPredictor reverse (models.py:80-137, modules.py, transforms.py) in torch ops ----
def _ln(x, m):
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), m.gamma, m.beta, 1e-5).transpose(1, -1)


def _dds(dds, x, x_mask, g=None):
    if g is not None:
        x = x + g
    for i in range(dds.n_layers):
        y = dds.convs_sep[i](x * x_mask)
        y = F.gelu(_ln(y, dds.norms_1[i]))
        y = F.gelu(_ln(dds.convs_1x1[i](y), dds.norms_2[i]))
        x = x + y
    return x * x_mask


def _rqs_inverse(inputs, uw, uh, ud, tail=5.0, mn=1e-3):
    inside = (inputs >= -tail) & (inputs <= tail)
    outputs = torch.zeros_like(inputs)
    ud = F.pad(ud, pad=(1, 1))
    const = math.log(math.exp(1 - mn) - 1)
    ud[..., 0] = const
    ud[..., -1] = const
    outputs[~inside] = inputs[~inside]
    x, uw, uh, ud = inputs[inside], uw[inside, :], uh[inside, :], ud[inside, :]
    nb = uw.shape[-1]

    def cum(u):
        w = mn + (1 - mn * nb) * F.softmax(u, dim=-1)
        c = F.pad(torch.cumsum(w, dim=-1), pad=(1, 0), mode="constant", value=0.0)
        c = 2 * tail * c - tail
        c[..., 0], c[..., -1] = -tail, tail
        return c, c[..., 1:] - c[..., :-1]

    cw, widths = cum(uw)
    der = mn + F.softplus(ud)
    ch, heights = cum(uh)
    loc = ch.clone()
    loc[..., -1] += 1e-6
    idx = (torch.sum(x[..., None] >= loc, dim=-1) - 1)[..., None]
    g = lambda t: t.gather(-1, idx)[..., 0]  # noqa: E731
    icw, ibw, ich, ih, delta = g(cw), g(widths), g(ch), g(heights), g(heights / widths)
    d0, d1 = g(der), der[..., 1:].gather(-1, idx)[..., 0]
    a = (x - ich) * (d0 + d1 - 2 * delta) + ih * (delta - d0)
    b = ih * d0 - (x - ich) * (d0 + d1 - 2 * delta)
    c = -delta * (x - ich)
    root = (2 * c) / (-b - torch.sqrt(b.pow(2) - 4 * a * c))
    outputs[inside] = root * ibw + icw
    return outputs


def torch_sdp_reverse(sdp, x, x_mask, noise, noise_scale):
    x = sdp.pre(x)
    x = _dds(sdp.convs, x, x_mask)
    x = sdp.proj(x) * x_mask
    flows = list(reversed(sdp.flows))
    flows = flows[:-2] + [flows[-1]]
    z = noise.to(device=x.device, dtype=x.dtype) * noise_scale  # (the reference draws on the CPU and moves)
    for f in flows:
        if isinstance(f, V._Flip):
            z = torch.flip(z, [1])
        elif isinstance(f, V._ElementwiseAffine):
            z = (z - f.m) * torch.exp(-f.logs) * x_mask
        else:
            x0, x1 = torch.split(z, [1, 1], 1)
            h = _dds(f.convs, f.pre(x0), x_mask, g=x)
            h = f.proj(h) * x_mask
            b, c, t = x0.shape
            h = h.reshape(b, c, -1, t).permute(0, 1, 3, 2)
            s = math.sqrt(f.filter_channels)
            x1 = _rqs_inverse(x1, h[..., :10] / s, h[..., 10:20] / s, h[..., 20:])
            z = torch.cat([x0, x1], 1) * x_mask
    return z[:, :1]


def generate_path(duration, mask):  # commons.generate_path
    b, _, t_y, t_x = mask.shape
    cum = torch.cumsum(duration, -1).view(b * t_x)
    path = (torch.arange(t_y, device=cum.device)[None, :] < cum[:, None]).to(mask.dtype).view(b, t_x, t_y)
    path = path - F.pad(path, [0, 0, 1, 0, 0, 0])[:, :-1]
    return path.unsqueeze(1).transpose(2, 3) * mask


def torch_dp_infer(net, ids, lengths, noise_w, noise_scale=0.667, length_scale=1.0, noise_scale_w=0.8):
    """SynthesizerTrn.infer (models.py:1288-1323) with the HIP enc_p / flow / dec and the torch-op duration predictor."""
    x, m_p, logs_p, x_mask = net.enc_p(ids, lengths)
    logw = torch_sdp_reverse(net.dp, x, x_mask, noise_w, noise_scale_w)
    w = torch.exp(logw) * x_mask * length_scale
    w_ceil = torch.ceil(w)
    y_lengths = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    y_mask = (torch.arange(int(y_lengths.max()), device=x.device)[None, :] < y_lengths[:, None]).unsqueeze(1).to(x_mask.dtype)
    attn = generate_path(w_ceil, torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1))
    m_p = torch.matmul(attn.squeeze(1), m_p.transpose(1, 2)).transpose(1, 2)
    logs_p = torch.matmul(attn.squeeze(1), logs_p.transpose(1, 2)).transpose(1, 2)
    z_p = m_p + torch.randn_like(m_p) * torch.exp(logs_p) * noise_scale
    z = net.flow(z_p, y_mask, reverse=True)
    return net.dec(z * y_mask)


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        d = FULL
        self.enc_p = V.TextEncoder(d["n_vocab"], d["inter"], d["hidden"], d["filter"], d["n_heads"], d["n_layers"], d["kernel"], 0.1)
        self.dp = V.StochasticDurationPredictor(d["hidden"], 192, 3, 0.5, 4)
        self.flow = V.ResidualCouplingTransformersBlock(d["inter"], d["hidden"], 5, 1, 4, use_transformer_flows=True, transformer_flow_type="pre_conv")
        self.dec = V.Generator(d["inter"], **GEN)


def build(dev):
    torch.manual_seed(0)
    net = Net()
    with torch.no_grad():  # O(1) activations; durations of a few frames per token
        for n, p in net.named_parameters():
            if n.endswith("gamma"):
                p.normal_(1.0, 0.1)
            elif n.endswith("weight_g"):
                p.uniform_(0.6, 1.0)
            elif p.dim() >= 2 and "emb" not in n and not n.endswith((".m", ".logs")):
                fan_in = p[0].numel() if ".ups." not in f".{n}" else p.shape[0] * p.shape[2]
                p.normal_(0.0, fan_in**-0.5)
            else:
                p.normal_(0.0, 0.1)
        net.dp.flows[0].m.copy_(torch.tensor([[-0.8], [0.0]]))
        net.dp.flows[0].logs.copy_(torch.tensor([[0.4], [0.0]]))
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
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--tokens", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--only", choices=["sdp-hip"], default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--split-f16", action="store_true", help='also time infer with precision = "split_f16" on enc_p, flow and dec together')
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = build(dev)
    for B in args.batch:
        Tx = args.tokens
        g = torch.Generator().manual_seed(B)
        lengths = torch.randint(int(0.8 * Tx), Tx + 1, (B,), generator=g)
        lengths[0] = Tx
        ids = torch.randint(0, FULL["n_vocab"], (B, Tx), generator=g).to(dev)
        lengths_d = lengths.to(dev)
        noise_w = torch.randn(B, 2, Tx, generator=g)
        with torch.no_grad():
            x, _, _, x_mask = net.enc_p(ids, lengths_d)
            if args.only == "sdp-hip":
                for _ in range(args.iters):
                    net.dp(x, x_mask, reverse=True, noise_scale=0.8, noise=noise_w)
                torch.cuda.synchronize()
                continue
            lw_hip = net.dp(x, x_mask, reverse=True, noise_scale=0.8, noise=noise_w)
            lw_torch = torch_sdp_reverse(net.dp, x, x_mask, noise_w, 0.8)
            sdp = rounds({"hip": lambda: net.dp(x, x_mask, reverse=True, noise_scale=0.8, noise=noise_w),
                          "torch_ops": lambda: torch_sdp_reverse(net.dp, x, x_mask, noise_w, 0.8)}, args.rounds)
            o_hip = V.infer(net, ids, lengths_d, noise_scale=0.667, length_scale=1.0, noise_scale_w=0.8, noise=(noise_w, None))[0]
            def hip_infer(mode):
                net.enc_p.precision = net.flow.precision = net.dec.precision = mode
                return V.infer(net, ids, lengths_d, noise_scale=0.667, length_scale=1.0, noise_scale_w=0.8, noise=(noise_w, None))

            def torch_dp_path():  # (its enc_p / flow / dec are the HIP ones: in exact fp32, whatever the variant before it set)
                net.enc_p.precision = net.flow.precision = net.dec.precision = "f32"
                return torch_dp_infer(net, ids, lengths_d, noise_w)

            inf = rounds({"hip": lambda: hip_infer("f32"), **({"hip_split_f16": lambda: hip_infer("split_f16")} if args.split_f16 else {}),
                          "torch_dp_dense_path": torch_dp_path}, args.rounds)
        row = dict(B=B, tokens=Tx, mean_tokens=float(lengths.float().mean()), frames=int(o_hip.shape[2] // 256),
                   sdp_logw_max_abs_diff_hip_vs_torch=float((lw_hip - lw_torch).abs().max()))
        for tag, res in (("sdp", sdp), ("infer", inf)):
            for k, v in res.items():
                row[f"{tag}_{k}_ms_median"] = round(statistics.median(v), 3)
                row[f"{tag}_{k}_ms_min"] = round(min(v), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
