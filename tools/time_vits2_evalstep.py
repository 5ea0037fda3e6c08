#!/usr/bin/env python3
"""Times the glue of the VITS2 validation step (csrc/evalstep.hip through torch_tts_amd.vits2) against the reference's formulation in
torch ops on the same GPU, the paths alternating in rounds in one process:

  kl       ttsvits_kl_loss from the unexpanded prior and frame_token (``hip``: the losses alone, ``hip_expand``: the expanded prior
           written too), against two matmuls by the dense one-hot path [B, T_y, T_x] plus losses.kl_loss's elementwise lines
           (models.py:1270-1271, losses.py:37-46)
  slices   the three ttsvits_slice_segments launches of a step (z channel-last, the mel, the waveform at ids * hop), against
           commons.slice_segments' Python loop, which reads one device scalar per utterance (three times B host syncs)
  step     vits2.validation_losses end to end, against the same step - the same drop-ins for the encoders, the flow, the search,
           the duration predictor, the generator, the front-end and the discriminators - with those torch-op pieces and F.l1_loss
           swapped in

at C = 192, T_x = 150 tokens, T_y = 600 frames, 1 and 64 utterances (ragged lengths at 64), hop 256, n_fft 1024, 80 mels, segments of
32 frames = 8192 samples.  Reports ms per call (the median of the rounds), the spread between the rounds, the paths' largest
difference in the project's metric |a - b| / (0.1 + |b|), and for each new kernel's call its algorithmic bytes (computed from
the shapes below) with the time those bytes take at the HBM rate a float4 copy reaches on this chip (6.29 TB/s) and its share.
Usage: python tools/time_vits2_evalstep.py [--batches 1 64] [--rounds 5] [--min-seconds 1.0] [--skip-step]"""
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

V = T.vits2
SPEC, INTER, HIDDEN = 80, 192, 192
T_X, T_Y, HOP, N_FFT, SEG = 150, 600, 256, 1024, 32
GEN = dict(resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2],
           upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])
AUDIO = dict(n_fft=N_FFT, hop_size=HOP, win_size=N_FFT, sampling_rate=22050, n_mels=SPEC, fmin=0.0, fmax=None, segment_size=SEG * HOP)
HBM = 6.29e12  # bytes/s of a float4 copy on this chip


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.segment_size = SEG
        self.enc_p = V.TextEncoder(178, INTER, HIDDEN, 768, 2, 6, 3, 0.1)
        self.enc_q = V.PosteriorEncoder(SPEC, INTER, HIDDEN, 5, 1, 16)
        self.flow = V.ResidualCouplingTransformersBlock(INTER, HIDDEN, 5, 1, 4, use_transformer_flows=True)
        self.dp = V.StochasticDurationPredictor(HIDDEN, 192, 3, 0.5, 4)
        self.dec = V.Generator(INTER, **GEN)


def build(mod, dev):
    torch.manual_seed(0)
    with torch.no_grad():  # O(1) activations
        for n, p in mod.named_parameters():
            if n.endswith("gamma"):
                p.normal_(1.0, 0.1)
            elif n.endswith("weight_g"):
                p.uniform_(0.6, 1.0)
            elif p.dim() >= 2 and "emb" not in n:
                p.normal_(0.0, p[0].numel() ** -0.5)
            else:
                p.normal_(0.0, 0.1)
        if hasattr(mod, "enc_q"):
            mod.enc_q.proj.weight.mul_(0.25)  # logs_q in a trained posterior's range
            mod.enc_q.proj.bias.mul_(0.25)
    return mod.to(dev).eval()


# ---- the reference's formulation in torch ops ----
def ref_slice(x, ids_str, segment_size):  # commons.py:50-56
    ret = torch.zeros_like(x[:, :, :segment_size])
    for i in range(x.size(0)):
        idx_str = ids_str[i]
        idx_end = idx_str + segment_size
        ret[i] = x[i, :, idx_str:idx_end]
    return ret


def ref_kl(z_p, logs_q, m_p, logs_p, z_mask):  # losses.py:37-46
    kl = logs_p - logs_q - 0.5
    kl += 0.5 * ((z_p - m_p) ** 2) * torch.exp(-2.0 * logs_p)
    kl = torch.sum(kl * z_mask)
    return kl / torch.sum(z_mask)


def ref_expand_kl(attn, z_p, logs_q, m_p, logs_p, z_mask):  # models.py:1270-1271, then kl_loss
    m = torch.matmul(attn, m_p.transpose(1, 2)).transpose(1, 2)
    logs = torch.matmul(attn, logs_p.transpose(1, 2)).transpose(1, 2)
    return ref_kl(z_p, logs_q, m, logs, z_mask)


def torch_step(net, net_d, x, t_x, spec, t_y, wav, ids, noise, c_mel=10.0, c_kl=0.2):
    """validation_losses with the glue as the reference writes it; everything else is the same drop-ins."""
    p = V._alignment_parts(net, x, t_x, spec, t_y, None, None, noise[0], {"dp": V.StochasticDurationPredictor, "dec": V.Generator}, "torch_step")
    l_length, _ = V._duration_terms(net.dp, p.xs, p.t_x, p.x_mask, p.w, p.logw_, p.g, noise[1], noise[2])
    tr = lambda t: t.transpose(1, 2)  # noqa: E731
    y_mask = (torch.arange(spec.shape[2], device=spec.device)[None, :] < p.t_y[:, None]).unsqueeze(1).to(torch.float32)
    attn = p.attn.squeeze(1)
    m_p = torch.matmul(attn, p.m_cl).transpose(1, 2)
    logs_p = torch.matmul(attn, p.logs_cl).transpose(1, 2)
    o = net.dec(ref_slice(tr(p.z_cl), ids, SEG))
    y_mel = ref_slice(spec, ids, SEG)
    y_hat_mel = V.mel_spectrogram_torch(o.squeeze(1), N_FFT, SPEC, 22050, HOP, N_FFT, 0.0, None)
    y = ref_slice(wav, ids * HOP, SEG * HOP)
    y_d_hat_r, y_d_hat_g, fmap_r, fmap_g = net_d(y, o)
    dr, dg = V.discriminator_loss(y_d_hat_r, y_d_hat_g)
    out = {"loss_disc": dr.sum() + dg.sum(), "loss_gen": V.generator_loss(y_d_hat_g).sum(), "loss_fm": V.feature_loss(fmap_r, fmap_g),
           "loss_mel": F.l1_loss(y_mel, y_hat_mel) * c_mel, "loss_dur": torch.sum(l_length.float()),
           "loss_kl": ref_kl(tr(p.zp_cl), tr(p.logsq_cl), m_p, logs_p, y_mask) * c_kl}
    out["loss_gen_all"] = out["loss_gen"] + out["loss_fm"] + out["loss_mel"] + out["loss_dur"] + out["loss_kl"]
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


def rounds(paths, n_rounds, min_seconds):
    per = {n: [] for n in paths}
    for _ in range(n_rounds):  # a, b, a, ...: drift of the clocks lands on every path alike
        for n, fn in paths.items():
            per[n].append(time_call(fn, min_seconds / n_rounds))
    return {n: dict(ms_per_call=round(statistics.median(v[0] for v in w), 4), ms_rounds=[round(v[0], 4) for v in w],
                    spread_ms=round(max(v[0] for v in w) - min(v[0] for v in w), 4), calls=sum(v[1] for v in w)) for n, w in per.items()}


def rel(a, b):
    return float(((a.double() - b.double()).abs() / (0.1 + b.double().abs())).max())


def floor(rows, name, nbytes):
    us = nbytes / HBM * 1e6
    rows[name].update(algorithmic_bytes=int(nbytes), hbm_floor_us=round(us, 2), share_of_hbm_floor=round(us / (rows[name]["ms_per_call"] * 1e3), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 64])
    ap.add_argument("--min-seconds", type=float, default=1.0, help="timed seconds per path and shape, over all rounds")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per path, the paths alternating")
    ap.add_argument("--skip-step", action="store_true", help="only the kernels' comparisons")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = V._align_engine(dev)
    net, net_d = (None, None) if args.skip_step else (build(Net(), dev), build(T.MultiPeriodDiscriminator(), dev))
    for B in args.batches:
        gen = torch.Generator().manual_seed(B)
        t_y = (torch.linspace(T_Y, T_Y // 2, B).round().long() if B > 1 else torch.tensor([T_Y])).to(dev)  # ragged, the longest first
        t_x = (torch.linspace(T_X, T_X // 2, B).round().long() if B > 1 else torch.tensor([T_X])).to(dev)
        frames = int(t_y.sum())
        with torch.no_grad():
            # ---- the KL from an alignment: every token of an utterance holds t_y / t_x frames, in order
            z_p, logs_q = torch.randn(B, INTER, T_Y, generator=gen).to(dev), (0.3 * torch.randn(B, INTER, T_Y, generator=gen)).to(dev)
            m_p, logs_p = torch.randn(B, INTER, T_X, generator=gen).to(dev), (0.3 * torch.randn(B, INTER, T_X, generator=gen)).to(dev)
            ar = torch.arange(T_Y, device=dev)[None, :]
            ft = torch.where(ar < t_y[:, None], (ar * t_x[:, None]) // t_y[:, None], torch.full_like(ar, -1)).to(torch.int32).contiguous()
            attn = (ft[:, :, None] == torch.arange(T_X, device=dev)[None, None, :]).float()
            y_mask = (ar < t_y[:, None]).unsqueeze(1).float()
            t_y32 = t_y.to(torch.int32)
            cl = [t.transpose(1, 2).contiguous() for t in (z_p, logs_q, m_p, logs_p)]
            kl = rounds({"hip": lambda: eng.kl_loss(*cl, ft, t_y32), "hip_expand": lambda: eng.kl_loss(*cl, ft, t_y32, True),
                         "torch_ops": lambda: ref_expand_kl(attn, z_p, logs_q, m_p, logs_p, y_mask)}, args.rounds, args.min_seconds)
            kl["torch_over_hip"] = round(kl["torch_ops"]["ms_per_call"] / kl["hip"]["ms_per_call"], 3)
            kl["max_rel_diff"] = rel(eng.kl_loss(*cl, ft, t_y32)[0][1], ref_expand_kl(attn, z_p, logs_q, m_p, logs_p, y_mask))
            # bytes: z_p and logs_q of the live frames, the prior's live rows once, frame_token and t_y; the frame sums written and read
            rows_bytes = 4 * INTER * (2 * frames + 2 * int(t_x.sum())) + 4 * B * T_Y + 4 * B + 2 * 4 * B * T_Y + 4 * (B + 2)
            floor(kl, "hip", rows_bytes)
            floor(kl, "hip_expand", rows_bytes + 2 * 4 * INTER * B * T_Y)
            # ---- the three slices of a step
            z_cl = torch.randn(B, T_Y, INTER, generator=gen).to(dev)
            z = z_cl.transpose(1, 2).contiguous()
            mel = torch.randn(B, SPEC, T_Y, generator=gen).to(dev)
            wav = (torch.rand(B, 1, T_Y * HOP, generator=gen) - 0.5).to(dev)
            ids = (torch.rand(B, generator=gen).to(dev) * (t_y - SEG + 1)).long()

            def hip_slices():
                return (eng.slice_segments(z_cl, ids, 1, T_Y, INTER, SEG)[0], eng.slice_segments(mel, ids, SPEC, T_Y, 1, SEG)[0],
                        eng.slice_segments(wav, ids, 1, T_Y * HOP, 1, SEG * HOP, HOP)[0])

            def torch_slices():
                return ref_slice(z, ids, SEG), ref_slice(mel, ids, SEG), ref_slice(wav, ids * HOP, SEG * HOP)

            sl = rounds({"hip": hip_slices, "torch_loop": torch_slices}, args.rounds, args.min_seconds)
            sl["torch_over_hip"] = round(sl["torch_loop"]["ms_per_call"] / sl["hip"]["ms_per_call"], 3)
            a, b = hip_slices(), torch_slices()
            sl["equal"] = bool(torch.equal(a[0].view(B, SEG, INTER).transpose(1, 2), b[0]) and torch.equal(a[1].view_as(b[1]), b[1])
                               and torch.equal(a[2].view_as(b[2]), b[2]))
            floor(sl, "hip", 2 * 4 * B * (SEG * INTER + SEG * SPEC + SEG * HOP) + 3 * (8 * B + 4))
            # ---- the mel L1 of a segment
            y_hat_mel = torch.randn(B, SPEC, SEG, generator=gen).to(dev)
            l1 = rounds({"hip": lambda: eng.sliced_l1(mel, y_hat_mel, ids), "torch_loop": lambda: F.l1_loss(ref_slice(mel, ids, SEG), y_hat_mel)},
                        args.rounds, args.min_seconds)
            l1["torch_over_hip"] = round(l1["torch_loop"]["ms_per_call"] / l1["hip"]["ms_per_call"], 3)
            l1["max_rel_diff"] = rel(eng.sliced_l1(mel, y_hat_mel, ids)[0][1], F.l1_loss(ref_slice(mel, ids, SEG), y_hat_mel))
            floor(l1, "hip", 2 * 4 * B * SPEC * SEG + 8 * B + 2 * 4 * B + 12)
            row = dict(utterances=B, T_y=T_Y, T_x=T_X, C=INTER, frames=frames, kl=kl, slices=sl, sliced_l1=l1)
            # ---- the step, end to end
            if not args.skip_step:
                x = torch.randint(0, 178, (B, T_X), generator=gen).to(dev)
                spec = (2.0 * torch.randn(B, SPEC, T_Y, generator=gen) - 4.0).to(dev)  # a log-mel's range
                noise = (torch.randn(B, INTER, T_Y, generator=gen).to(dev), torch.randn(B, 2, T_X, generator=gen), torch.randn(B, 2, T_X, generator=gen))
                t_x32 = t_x.to(torch.int32)

                def hip_step():
                    return V.validation_losses(net, net_d, x, t_x32, spec, t_y32, wav, **AUDIO, noise=noise, ids_slice=ids)

                def ref_step():
                    return torch_step(net, net_d, x, t_x32, spec, t_y32, wav, ids, noise)

                st = rounds({"hip": hip_step, "torch_pieces": ref_step}, args.rounds, args.min_seconds)
                st["torch_over_hip"] = round(st["torch_pieces"]["ms_per_call"] / st["hip"]["ms_per_call"], 3)
                a, b = hip_step(), ref_step()
                st["max_rel_diff"] = {k: rel(a[k], b[k]) for k in b}
                row["step"] = st
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
