#!/usr/bin/env python3
"""Golden vectors for the VITS2 duration predictors (vits2/models.py:29-180) and the whole SynthesizerTrn.infer
(models.py:1288-1323), produced by the reference's own models.py on CPU.  models.py imports monotonic_align at module level,
which inference never uses: a stub module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_duration.py <path to the reference's vits2 directory>

Writes tests/golden/duration_small.npz + duration_meta.json (reduced dims, no reference source):
  sdp{0,4}/w/<key>, dp{0,4}/w/<key>   StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin) / DurationPredictor(32, 48, 3, 0.5, gin)
                                      state dicts with every weight randomised (the reference zero-initialises each ConvFlow proj,
                                      which would make every spline an identity)
  case/x, case/x_mask, case/g4, case/noise    x [3, 32, 9] (lengths 9, 5, 1; padded frames zero), speaker rows, the SDP's noise
  sdp{0,4}/logw, dp{0,4}/logw         the reference's outputs (SDP: reverse=True, noise_scale 2.0, the noise recorded)
  infer_{sdp,dp}[_g]/{ids, lengths, sid, e_w, e_z, o, attn, y_mask, z, z_p, m_p, logs_p, logw}   one infer call of a SynthesizerTrn at the
                                      VITS2 fixtures' dims with upsampling [4, 2], and both of its draws
and in the meta JSON the seeds and checksums of that model's enc_p / dp / flow / dec (/ emb_g) weights (randomize() below
redraws them; storing them would take several MB), the dims, the call arguments and the state-dict key / shape records of both predictors at the ModelConfig dims.
The weights are drawn until no duration w = exp(logw) * length_scale lies within 1e-4 of an integer (ceil is discontinuous)."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = sys.argv[1]
sys.path.insert(0, REF)
sys.modules.setdefault("monotonic_align", types.ModuleType("monotonic_align"))  # (imported by models.py, unused by inference)
import models  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
W = 32  # SDP / DP width at the small dims
NET = dict(n_vocab=23, spec_channels=16, segment_size=32, inter_channels=16, hidden_channels=32, filter_channels=48, n_heads=2, n_layers=2,
           kernel_size=3, p_dropout=0.1, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
           upsample_rates=[4, 2], upsample_initial_channel=32, upsample_kernel_sizes=[8, 4], use_transformer_flows=True,
           transformer_flow_type="pre_conv")
PARTS = ("enc_p", "dp", "flow", "dec", "emb_g")
out = {}


def randomize(mod, seed):
    """Weights that keep activations O(1): LayerNorm gains near 1, weight_norm gains in [0.6, 1], weights at 1/sqrt(fan_in),
    biases, embeddings and ElementwiseAffine parameters 0.1 N(0, 1).  ConvFlow projections at 1.5/sqrt(fan_in): spline bins of
    clearly unequal widths.  (tests/test_duration_host.py redraws with the same rule.)"""
    gsd = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("gamma"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gsd))
            elif n.endswith("weight_g"):
                p.copy_(0.6 + 0.4 * torch.rand(p.shape, generator=gsd))
            elif p.dim() >= 2 and not n.endswith((".m", ".logs")) and "emb" not in n:
                fan_in = p[0].numel() if not ".ups." in f".{n}" else p.shape[0] * p.shape[2]
                scale = 1.5 if ("flows" in n and "proj" in n) else 1.0
                p.copy_(scale * torch.randn(p.shape, generator=gsd) / fan_in**0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gsd))
    return mod


def save_sd(prefix, mod):
    for k, v in mod.state_dict().items():
        out[f"{prefix}/w/{k}"] = v.detach().numpy().copy()


def checksum(mod):
    """[tensors, elements, sum, sum |v|, sum over tensors of (index + 1) * sum]: a state dict's keys, shapes, values and order."""
    vs = [v.double() for v in mod.state_dict().values()]
    return [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
            float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]


def write_meta(meta, path):
    """JSON with one line per scalar entry, per infer case and per state-dict record."""
    lines = []
    for k, v in meta.items():
        if k.startswith("fulldims_"):
            lines.append(f" {json.dumps(k)}: [\n  " + ",\n  ".join(json.dumps(r) for r in v) + "\n ]")
        elif k == "infer":
            lines.append(f" {json.dumps(k)}: {{\n  " + ",\n  ".join(f"{json.dumps(n)}: {json.dumps(c)}" for n, c in v.items()) + "\n }")
        else:
            lines.append(f" {json.dumps(k)}: {json.dumps(v)}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


def near_integer(w, mask):
    w = w[mask > 0]
    return bool(((w - w.round()).abs() < 1e-4).any())


class Recorder:
    """Records what torch.randn / torch.randn_like return inside models.py (the two draws of infer)."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self._randn, self._randn_like = torch.randn, torch.randn_like

        def randn(*a, **k):
            r = self._randn(*a, **k)
            self.draws.append(r.clone())
            return r

        def randn_like(*a, **k):
            r = self._randn_like(*a, **k)
            self.draws.append(r.clone())
            return r

        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self._randn, self._randn_like


def predictors(meta):
    torch.manual_seed(3)
    x = torch.randn(3, W, 9)
    lengths = torch.tensor([9, 5, 1])
    x_mask = (torch.arange(9)[None, :] < lengths[:, None]).unsqueeze(1).float()
    x = x * x_mask
    g = torch.randn(3, 4, 1)
    noise = torch.randn(3, 2, 9)
    noise[0, 0, 1], noise[0, 1, 2], noise[1, 1, 3] = 3.1, -3.4, 2.8  # x 2.0: spline inputs beyond the +-5 tails
    noise[2, 0, 0] = 2.5  # x 2.0 = 5.0: the first ConvFlow's spline input on the top edge (searchsorted's eps keeps it in the last bin)
    out.update({"case/x": x.numpy(), "case/x_mask": x_mask.numpy(), "case/g4": g.numpy(), "case/noise": noise.numpy()})
    meta["sdp_noise_scale"] = 2.0
    for gin in (0, 4):
        sdp = randomize(models.StochasticDurationPredictor(W, 192, 3, 0.5, 4, gin_channels=gin).eval(), 20 + gin)
        dp = randomize(models.DurationPredictor(W, 48, 3, 0.5, gin_channels=gin).eval(), 30 + gin)
        save_sd(f"sdp{gin}", sdp)
        save_sd(f"dp{gin}", dp)
        gg = g if gin else None
        real = torch.randn
        with torch.no_grad():
            torch.randn = lambda *a, **k: noise.clone()  # the recorded draw
            try:
                logw = sdp(x, x_mask, g=gg, reverse=True, noise_scale=2.0)
            finally:
                torch.randn = real
            out[f"sdp{gin}/logw"] = logw.numpy()
            out[f"dp{gin}/logw"] = dp(x, x_mask, g=gg).numpy()
        # how much of the spline the case exercises: the inputs of the first ConvFlow's spline (noise * 2, channel 0 after the Flip)
        meta[f"sdp{gin}_first_spline_outside_tails"] = int(((noise[:, 0] * 2.0).abs() > 5).logical_and(x_mask[:, 0] > 0).sum())


def infer_case(meta, name, use_sdp, n_speakers, seed):
    gin = 4 if n_speakers else 0
    for attempt in range(200):
        torch.manual_seed(seed + attempt)
        net = models.SynthesizerTrn(**NET, n_speakers=n_speakers, gin_channels=gin, use_sdp=use_sdp).eval()
        for part in PARTS:
            if hasattr(net, part):
                randomize(getattr(net, part), 1000 * seed + 10 * attempt + len(part))
        with torch.no_grad():
            if use_sdp:  # durations of 1 - 8 frames: logw = (y - m) exp(-logs)
                net.dp.flows[0].m.copy_(torch.tensor([[-0.8], [0.0]]))
                net.dp.flows[0].logs.copy_(torch.tensor([[0.4], [0.0]]))
            else:
                net.dp.proj.bias.fill_(1.0)
        ids = torch.randint(0, NET["n_vocab"], (3, 7))
        lengths = torch.tensor([7, 4, 1])
        sid = torch.tensor([1, 0, 1]) if n_speakers else None
        args = dict(noise_scale=0.667, length_scale=1.1, noise_scale_w=0.8)
        with torch.no_grad(), Recorder() as rec:
            o, attn, y_mask, (z, z_p, m_p, logs_p) = net.infer(ids, lengths, sid=sid, **args)
            # logw, recomputed with the recorded draw (for the duration check and the tests' comparisons)
            g = None if sid is None else net.emb_g(sid).unsqueeze(-1)
            xh, _, _, x_mask = net.enc_p(ids, lengths, g=g)
            if use_sdp:
                real = torch.randn
                torch.randn = lambda *a, **k: rec.draws[0].clone()
                try:
                    logw = net.dp(xh, x_mask, g=g, reverse=True, noise_scale=args["noise_scale_w"])
                finally:
                    torch.randn = real
            else:
                logw = net.dp(xh, x_mask, g=g)
        w = torch.exp(logw) * x_mask * args["length_scale"]
        if near_integer(w, x_mask.expand_as(w)):
            continue
        e_w, e_z = (rec.draws[0], rec.draws[1]) if use_sdp else (None, rec.draws[0])
        assert e_z.shape == m_p.shape
        # (the weights are not stored - the flow alone would be 1.2 MB: the tests redraw them with randomize() and these seeds,
        # and check each part against the checksum recorded here)
        sums = {part: checksum(getattr(net, part)) for part in PARTS if hasattr(net, part)}
        rec_out = dict(ids=ids, lengths=lengths, e_z=e_z, o=o, attn=attn, y_mask=y_mask, z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, logw=logw)
        if use_sdp:
            rec_out["e_w"] = e_w
        if sid is not None:
            rec_out["sid"] = sid
        for k, v in rec_out.items():
            out[f"{name}/{k}"] = v.numpy()
        meta["infer"][name] = dict(use_sdp=use_sdp, n_speakers=n_speakers, gin_channels=gin, args=args, attempt=attempt, checksums=sums,
                                   seeds={part: 1000 * seed + 10 * attempt + len(part) for part in PARTS},
                                   y_lengths=y_mask[:, 0].sum(1).long().tolist(), w_min_dist_to_int=float((w - w.round()).abs()[x_mask.expand_as(w) > 0].min()))
        return
    raise RuntimeError("no draw without a duration next to an integer")


def main():
    meta = {"width": W, "dp_filter": 48, "lengths": [9, 5, 1], "net": NET, "infer": {}}
    predictors(meta)
    infer_case(meta, "infer_sdp", True, 0, 40)
    infer_case(meta, "infer_dp", False, 0, 50)
    infer_case(meta, "infer_sdp_g", True, 2, 60)
    sdp = models.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=0)
    dp = models.DurationPredictor(192, 256, 3, 0.5, gin_channels=0)
    meta["fulldims_sdp_state_dict"] = [[k, list(v.shape)] for k, v in sdp.state_dict().items()]
    meta["fulldims_dp_state_dict"] = [[k, list(v.shape)] for k, v in dp.state_dict().items()]
    np.savez_compressed(os.path.join(HERE, "duration_small.npz"), **out)
    write_meta(meta, os.path.join(HERE, "duration_meta.json"))
    print(json.dumps(meta["infer"]), os.path.getsize(os.path.join(HERE, "duration_small.npz")), "bytes")


if __name__ == "__main__":
    main()
