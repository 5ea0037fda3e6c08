#!/usr/bin/env python3
"""Times VITS2 voice conversion at the ModelConfig dims on one GPU, the variants alternated in one process (median and min of the rounds,
ms per call):
  (a) post: the PosteriorEncoder (80 -> 192, 16 WN layers of 5 taps, speaker-conditioned) at B x T frames - the HIP library
            (torch_tts_amd.vits2.PosteriorEncoder, ttspost_*; both precisions) against the reference's algorithm in torch ops on the same
            GPU in fp32; with the achieved TFLOP/s and its fraction of the fp32 matrix peak (157.3 TFLOP/s);
  (b) vc:   SynthesizerTrn.voice_conversion for one utterance - torch_tts_amd.vits2.voice_conversion against the same four stages in torch
            ops (posterior, flow forward, flow reverse, generator).
Usage: python tools/time_vits2_vc.py [--batch 64] [--frames 600] [--vc-frames 600] [--rounds 15]"""
import argparse
import json
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
from oracle import vits2_oracle as O  # noqa: E402

V = T.vits2
SPEC, INTER, HIDDEN, GIN = 80, 192, 192, 256
GEN = dict(resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2],
           upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])
PEAK_F32 = 157.3e12


def post_flops_per_frame(S=SPEC, H=HIDDEN, I=INTER, k=5, L=16):
    wn = sum(2 * 2 * H * k * H + 2 * (2 * H if j < L - 1 else H) * H for j in range(L))
    return 2 * S * H + wn + 2 * 2 * I * H


# ---- the reference's algorithms in torch ops (fp32), on the modules' own parameters ----
def torch_posterior(wts, y, lengths, g, noise):
    x_mask = (torch.arange(y.shape[2], device=y.device)[None, :] < lengths[:, None]).unsqueeze(1).to(y.dtype)  # commons.sequence_mask
    x = F.conv1d(y, wts["pre.weight"], wts["pre.bias"]) * x_mask
    x = O.wn(x, x_mask, wts, "enc", 16, 5, g=g)
    stats = F.conv1d(x, wts["proj.weight"], wts["proj.bias"]) * x_mask
    m, logs = torch.split(stats, INTER, dim=1)
    return (m + noise * torch.exp(logs)) * x_mask, x_mask


def torch_flow_forward(wts, x, x_mask, d, g):
    half = d.inter_channels // 2
    for i in range(d.n_flows):
        p = f"flow.flows.{2 * i}"
        x0, x1 = torch.split(x, [half, half], 1)
        x0_ = O.encoder_stack(x0 * x_mask, x_mask, wts, p + ".pre_transformer", d.flow_tf_layers, d.flow_tf_heads, None, d.flow_tf_kernel) + x0
        h = F.conv1d(x0_, wts[p + ".pre.weight"], wts[p + ".pre.bias"]) * x_mask
        h = O.wn(h, x_mask, wts, p + ".enc", d.flow_wn_layers, d.flow_kernel, g=g)
        m = F.conv1d(h, wts[p + ".post.weight"], wts[p + ".post.bias"]) * x_mask
        x = torch.flip(torch.cat([x0, m + x1 * x_mask], 1), [1])
    return x


def torch_generator(dec, x, g):
    x = dec.conv_pre(x) + dec.cond(g)
    for i, up in enumerate(dec.ups):
        x = up(F.leaky_relu(x, 0.1))
        xs = None
        for j in range(dec.num_kernels):
            rb = dec.resblocks[i * dec.num_kernels + j]
            xr = x
            for c1, c2 in zip(rb.convs1, rb.convs2):
                xr = c2(F.leaky_relu(c1(F.leaky_relu(xr, 0.1)), 0.1)) + xr
            xs = xr if xs is None else xs + xr
        x = xs / dec.num_kernels
    return torch.tanh(dec.conv_post(F.leaky_relu(x)))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.n_speakers = 4
        self.enc_q = V.PosteriorEncoder(SPEC, INTER, HIDDEN, 5, 1, 16, gin_channels=GIN)
        self.flow = V.ResidualCouplingTransformersBlock(INTER, HIDDEN, 5, 1, 4, gin_channels=GIN, use_transformer_flows=True)
        self.dec = V.Generator(INTER, **GEN, gin_channels=GIN)
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
                fan_in = p[0].numel() if ".ups." not in f".{n}" else p.shape[0] * p.shape[2]
                p.normal_(0.0, fan_in**-0.5)
            else:
                p.normal_(0.0, 0.1)
    return net.to(dev).eval()


def eff_weights(mod, prefix=""):
    """state dict with weight-normed weights folded (the oracle reads weight_g / weight_v itself; folding once keeps the torch-op
    variant from paying the norm per call, as a user's remove_weight_norm() would)."""
    sd = {prefix + k: v for k, v in mod.state_dict().items()}
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_v"):
            base = k[: -len(".weight_v")]
            out[base + ".weight"] = O.weight_norm_weight(sd, base)
        elif not k.endswith(".weight_g"):
            out[k] = v
    return out


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
    ap.add_argument("--vc-frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = build(dev)
    pw = eff_weights(net.enc_q)
    fw = eff_weights(net.flow, "flow.")
    d = O.Vits2Dims(inter_channels=INTER, flow_hidden=HIDDEN, gin_channels=GIN)
    with torch.no_grad():
        # (a) posterior encoder, B x T frames, all frames valid
        B, Tn = args.batch, args.frames
        gen = torch.Generator().manual_seed(1)
        y = torch.randn(B, SPEC, Tn, generator=gen).to(dev)
        lens = torch.full((B,), Tn, dtype=torch.int32, device=dev)
        g = net.emb_g(torch.arange(B, device=dev) % 4).unsqueeze(-1)
        noise = torch.randn(B, INTER, Tn, generator=gen).to(dev)
        fns = {}
        for prec in ("f32", "split_f16"):
            def hip(prec=prec):
                net.enc_q.precision = prec
                return net.enc_q.forward_cl(y, lens, g=g, noise=noise)
            fns[f"hip_{prec}"] = hip
        fns["torch_ops"] = lambda: torch_posterior(pw, y, lens, g, noise)
        z_hip = fns["hip_f32"]()[0]
        z_ref = torch_posterior(pw, y, lens, g, noise)[0]
        post = rounds(fns, args.rounds)
        flop = post_flops_per_frame() * B * Tn
        row = dict(stage="posterior_encoder", B=B, frames=Tn, gflop=round(flop / 1e9, 1),
                   z_max_abs_diff_hip_f32_vs_torch=float((z_hip.transpose(1, 2) - z_ref).abs().max()))
        for k, v in post.items():
            med = statistics.median(v)
            row[f"{k}_ms_median"] = round(med, 3)
            row[f"{k}_ms_min"] = round(min(v), 3)
            row[f"{k}_tflops"] = round(flop / (med * 1e-3) / 1e12, 1)
            row[f"{k}_of_f32_matrix_peak"] = round(flop / (med * 1e-3) / PEAK_F32, 3)
        print(json.dumps(row), flush=True)
        net.enc_q.precision = "f32"
        # (b) voice_conversion, one utterance
        Tv = args.vc_frames
        yv = torch.randn(1, SPEC, Tv, generator=gen).to(dev)
        lv = torch.tensor([Tv], device=dev)
        nv = torch.randn(1, INTER, Tv, generator=gen).to(dev)
        s_src, s_tgt = torch.tensor([0], device=dev), torch.tensor([2], device=dev)

        def torch_vc():
            g_src, g_tgt = net.emb_g(s_src).unsqueeze(-1), net.emb_g(s_tgt).unsqueeze(-1)
            z, y_mask = torch_posterior(pw, yv, lv, g_src, nv)
            z_p = torch_flow_forward(fw, z, y_mask, d, g_src)
            z_hat = O.flow_reverse(z_p, y_mask, fw, d, g=g_tgt)
            return torch_generator(net.dec, z_hat * y_mask, g_tgt)

        o_hip = V.voice_conversion(net, yv, lv, s_src, s_tgt, noise=nv)[0]
        o_ref = torch_vc()
        vc = rounds({"hip": lambda: V.voice_conversion(net, yv, lv, s_src, s_tgt, noise=nv), "torch_ops": torch_vc}, args.rounds)
        row = dict(stage="voice_conversion", B=1, frames=Tv, samples=int(o_hip.shape[2]),
                   o_hat_max_abs_diff_hip_vs_torch=float((o_hip - o_ref).abs().max()))
        for k, v in vc.items():
            row[f"{k}_ms_median"] = round(statistics.median(v), 3)
            row[f"{k}_ms_min"] = round(min(v), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
