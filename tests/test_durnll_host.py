"""Host-side checks of the VITS2 duration likelihood (vits2/models.py:78-125, the l_length of SynthesizerTrn.forward): the fp64
restatement below - the oracle of tests/test_durnll_hip.py - against the reference's own outputs
(tests/golden/make_golden_durnll.py), the ttsvits_durnll_* C ABI's counts, sizes and refusals, and what the module refuses.
No GPU needed."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_duration_host import dds_conv, randomize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NLL_REL = 1e-4  # the project's bar: |a - b| / (0.1 + |b|)


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "durnll_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "durnll_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def rel(a, b):
    return float(((a.double() - b.double()).abs() / (0.1 + b.double().abs())).max())


def mask_of(lengths, T):
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).unsqueeze(1).float()


def checksum(mod):
    vs = [v.double() for v in mod.state_dict().values()]
    return [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
            float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]


def same_checksum(mod, want):
    got = checksum(mod)
    return got[:2] == want[:2] and all(abs(a - b) <= 1e-9 * max(1.0, abs(want[3]) * got[0]) for a, b in zip(got[2:], want[2:]))


def golden_sdp(meta, gin):
    """The drop-in predictor of the small fixture: weights redrawn with the recorded seed, checked against the reference's sums."""
    import torch_tts_amd as T

    sdp = randomize(T.StochasticDurationPredictor(meta["width"], 192, 3, 0.5, 4, gin_channels=gin), meta["sdp"][str(gin)]["seed"])
    assert same_checksum(sdp, meta["sdp"][str(gin)]["checksum"]), gin
    return sdp.eval()


def big_case(seed):
    """The C = 192, T = 150 inputs of the yardstick (tests/golden/make_golden_durnll.big_case): x, x_mask, w, e_q."""
    gen = torch.Generator().manual_seed(seed)
    x_mask = mask_of([150, 149, 64, 2], 150)
    x = torch.randn(4, 192, 150, generator=gen) * x_mask
    w = torch.randint(1, 13, (4, 1, 150), generator=gen).float() * x_mask
    e_q = torch.randn(4, 2, 150, generator=gen)
    return x, x_mask, w, e_q


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 restatement of StochasticDurationPredictor.forward(x, x_mask, w, g) over a state dict
# ---------------------------------------------------------------------------------------------------------------------------
def spline_forward(x, uw, uh, ud, tail=5.0):
    """The rational-quadratic spline with linear tails, forward: x [N], uw / uh [N, nb], ud [N, nb - 1] -> (y, log |dy/dx|).
    Knots: bin widths / heights mn + (1 - nb mn) softmax(.), scaled to [-tail, tail]; knot derivatives mn + softplus(.), with the
    two outer ones fixed so that they are 1; inside bin k with theta = (x - x_k) / w_k and s_k = h_k / w_k:
      y = y_k + h_k (s_k theta^2 + d_k theta (1 - theta)) / (s_k + (d_k + d_k+1 - 2 s_k) theta (1 - theta))
      dy/dx = s_k^2 (d_k+1 theta^2 + 2 s_k theta (1 - theta) + d_k (1 - theta)^2) / (the same denominator)^2."""
    mn, nb = 1e-3, uw.shape[-1]
    y, lad = x.clone(), torch.zeros_like(x)
    inside = (x >= -tail) & (x <= tail)
    if not inside.any():
        return y, lad
    xi = x[inside]
    ud = F.pad(ud[inside], (1, 1), value=math.log(math.exp(1 - mn) - 1))

    def knots(u):
        k = F.pad(torch.cumsum(mn + (1 - mn * nb) * F.softmax(u[inside], dim=-1), -1), (1, 0))
        k = 2 * tail * k - tail
        k[..., 0], k[..., -1] = -tail, tail
        return k

    kx, ky, d = knots(uw), knots(uh), mn + F.softplus(ud)
    edges = kx.clone()
    edges[..., -1] += 1e-6
    idx = (torch.sum(xi[..., None] >= edges, dim=-1) - 1)[..., None]
    at = lambda t, j=idx: t.gather(-1, j)[..., 0]  # noqa: E731
    xk, wk, yk, hk = at(kx), at(kx[..., 1:] - kx[..., :-1]), at(ky), at(ky[..., 1:] - ky[..., :-1])
    sk, dk, dk1 = hk / wk, at(d), at(d[..., 1:])
    th = (xi - xk) / wk
    den = sk + (dk + dk1 - 2 * sk) * th * (1 - th)
    y[inside] = yk + hk * (sk * th**2 + dk * th * (1 - th)) / den
    lad[inside] = torch.log(sk**2 * (dk1 * th**2 + 2 * sk * th * (1 - th) + dk * (1 - th) ** 2)) - 2 * torch.log(den)
    return y, lad


def conv_flow_forward(sd, p, z, x_mask, g, probe=None):
    """modules.ConvFlow.forward (in_channels 2, num_bins 10): -> (cat([x0, spline(x1)]) * mask, logdet [B])."""
    x0, x1 = z[:, :1], z[:, 1:]
    Cw = sd[p + ".pre.weight"].shape[0]
    h = F.conv1d(x0, sd[p + ".pre.weight"].double(), sd[p + ".pre.bias"].double())
    h = dds_conv(sd, p + ".convs", h, x_mask, g=g)
    h = F.conv1d(h, sd[p + ".proj.weight"].double(), sd[p + ".proj.bias"].double()) * x_mask
    B, _, T = x0.shape
    h = h.reshape(B, 1, -1, T).permute(0, 1, 3, 2)
    uw, uh, ud = h[..., :10] / math.sqrt(Cw), h[..., 10:20] / math.sqrt(Cw), h[..., 20:]
    if probe is not None:
        probe.append((x1 * x_mask)[x_mask.expand_as(x1) > 0])
    y1, lad = spline_forward(x1.reshape(-1), uw.reshape(-1, 10), uh.reshape(-1, 10), ud.reshape(-1, 9))
    y1, lad = y1.reshape(B, 1, T), lad.reshape(B, 1, T)
    return torch.cat([x0, y1], 1) * x_mask, torch.sum(lad * x_mask, [1, 2])


def _affine(sd, p, z, x_mask):
    return (sd[p + ".m"].double() + torch.exp(sd[p + ".logs"].double()) * z) * x_mask, torch.sum(sd[p + ".logs"].double() * x_mask, [1, 2])


def sdp_nll(sd, x, x_mask, w, e_q, g=None, n_flows=4):
    """-> dict(nll [B], terms [B, 4] as ttsvits_durnll_forward orders them, z [B, 2, T] after the last flow, spline_inputs: every
    in-length x1 a spline saw, clamped: whether Log's clamp_min was hit at an in-length token), fp64."""
    x, x_mask, w, e_q = x.double(), x_mask.double(), w.double(), e_q.double()
    x = F.conv1d(x, sd["pre.weight"].double(), sd["pre.bias"].double())
    if g is not None:
        x = x + F.conv1d(g.double(), sd["cond.weight"].double(), sd["cond.bias"].double())
    x = dds_conv(sd, "convs", x, x_mask)
    x = F.conv1d(x, sd["proj.weight"].double(), sd["proj.bias"].double()) * x_mask
    h_w = F.conv1d(w, sd["post_pre.weight"].double(), sd["post_pre.bias"].double())
    h_w = dds_conv(sd, "post_convs", h_w, x_mask)
    h_w = F.conv1d(h_w, sd["post_proj.weight"].double(), sd["post_proj.bias"].double()) * x_mask
    probe = []
    e_q = e_q * x_mask
    z_q, logdet_q = _affine(sd, "post_flows.0", e_q, x_mask)
    for k in range(4):
        z_q, ld = conv_flow_forward(sd, f"post_flows.{2 * k + 1}", z_q, x_mask, x + h_w, probe)
        z_q, logdet_q = torch.flip(z_q, [1]), logdet_q + ld
    z_u, z1 = z_q[:, :1], z_q[:, 1:]
    u = torch.sigmoid(z_u) * x_mask
    z0 = (w - u) * x_mask
    logdet_q = logdet_q + torch.sum((F.logsigmoid(z_u) + F.logsigmoid(-z_u)) * x_mask, [1, 2])
    t1 = torch.sum(-0.5 * (math.log(2 * math.pi) + e_q**2) * x_mask, [1, 2])
    clamped = bool(((z0 < 1e-5) & (x_mask > 0)).any())
    y0 = torch.log(torch.clamp_min(z0, 1e-5)) * x_mask
    logdet = torch.sum(-y0, [1, 2])
    z, ld = _affine(sd, "flows.0", torch.cat([y0, z1], 1), x_mask)
    logdet = logdet + ld
    for k in range(n_flows):
        z, ld = conv_flow_forward(sd, f"flows.{2 * k + 1}", z, x_mask, x, probe)
        z, logdet = torch.flip(z, [1]), logdet + ld
    t3 = torch.sum(0.5 * (math.log(2 * math.pi) + z**2) * x_mask, [1, 2])
    return dict(nll=(t3 - logdet) + (t1 - logdet_q), terms=torch.stack([t1, logdet_q, t3, logdet], 1), z=z, spline_inputs=torch.cat(probe),
                clamped=clamped)


def state(mod):
    return {k: v.detach().clone().cpu() for k, v in mod.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference():
    """To 1e-9 relative against the reference's own module in fp64, and within the reference's fp32 error of its fp32 records."""
    sd, meta = load_golden()
    for gin in (0, 4):
        got = sdp_nll(state(golden_sdp(meta, gin)), sd["case/x"], sd["case/x_mask"], sd["case/w"], sd["case/e_q"], sd["case/g4"] if gin else None)
        assert sd[f"sdp{gin}/nll64"].dtype == torch.float64 and got["z"].shape == sd[f"sdp{gin}/z64"].shape == (3, 2, 9)
        assert rel(got["nll"], sd[f"sdp{gin}/nll64"]) <= 1e-9, (gin, rel(got["nll"], sd[f"sdp{gin}/nll64"]))
        assert rel(got["z"], sd[f"sdp{gin}/z64"]) <= 1e-9, (gin, rel(got["z"], sd[f"sdp{gin}/z64"]))
        t = got["terms"]
        assert rel((t[:, 2] - t[:, 3]) + (t[:, 0] - t[:, 1]), sd[f"sdp{gin}/nll64"]) <= 1e-9
        err = meta["sdp"][str(gin)]["cpu_f32_err"]
        assert abs(rel(sd[f"sdp{gin}/nll"], got["nll"]) - err) <= 1e-9 and err <= meta["yardstick_max"] <= NLL_REL / 4
        # (not an identity chain, and nothing at padded tokens)
        assert float(t[:, 1].abs().min()) > 0.1 and float(t[:, 3].abs().min()) > 0.1 and float(sd[f"sdp{gin}/z"][2, :, 1:].abs().max()) == 0.0
    assert meta["c192_t150"]["cpu_f32_err"] <= meta["yardstick_max"]


def test_yardstick_case_is_reproducible():
    _, meta = load_golden()
    c = meta["c192_t150"]
    x, x_mask, w, e_q = big_case(c["case_seed"])
    assert x_mask[:, 0].sum(1).long().tolist() == c["lengths"] and float(w.max()) == 12.0 and float(w[x_mask > 0].min()) == 1.0


def _dims(**over):
    from torch_tts_amd import _lib

    d = _lib.DurNllDims(192, 3, 4, 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_c_abi_symbols_counts_and_refusals():
    from torch_tts_amd import _lib

    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ttsvits_durnll_[a-z_0-9]+)\s*\(", hdr))
    want = {f"ttsvits_durnll_{n}" for n in ("create", "workspace_bytes", "forward", *_lib.SHARED)}
    assert declared == want and want <= set(_lib.FAMILY_SYMBOLS["ttsvits"]) and len(want) == 9
    for s in want:
        assert hasattr(lib, s), s
    h = C.c_void_p()
    for bad in (dict(kernel_size=5), dict(in_channels=190), dict(in_channels=512), dict(n_flows=1), dict(n_flows=9), dict(gin_channels=-1)):
        assert lib.ttsvits_durnll_create(C.byref(_dims(**bad)), C.byref(h)) == _lib.ERR_DIMS, bad
    for n_flows, gin, count in ((4, 0, 284), (4, 4, 286), (6, 0, 172 + 28 * 6), (2, 3, 172 + 28 * 2 + 2)):
        assert lib.ttsvits_durnll_create(C.byref(_dims(n_flows=n_flows, gin_channels=gin)), C.byref(h)) == _lib.OK
        try:
            assert lib.ttsvits_durnll_num_weight_tensors(h) == count, (n_flows, gin)
        finally:
            lib.ttsvits_durnll_destroy(h)
    assert lib.ttsvits_durnll_create(C.byref(_dims()), C.byref(h)) == _lib.OK
    try:
        vp, ws = C.c_void_p(256), 1 << 40
        fwd = lib.ttsvits_durnll_forward
        assert fwd(h, vp, vp, None, vp, vp, 2, 8, vp, None, None, vp, ws, None) == _lib.ERR_NOT_BOUND
        assert fwd(h, vp, vp, None, None, vp, 2, 8, vp, None, None, vp, ws, None) == _lib.ERR_INVALID_ARG  # no w
        assert fwd(h, vp, vp, None, vp, None, 2, 8, vp, None, None, vp, ws, None) == _lib.ERR_INVALID_ARG  # no noise
        assert fwd(h, vp, vp, vp, vp, vp, 2, 8, vp, None, None, vp, ws, None) == _lib.ERR_INVALID_ARG  # g with gin = 0
        assert fwd(h, vp, vp, None, vp, vp, 0, 8, vp, None, None, vp, ws, None) == _lib.ERR_INVALID_ARG
        assert lib.ttsvits_durnll_workspace_bytes(h, 0, 8) == 0
        # 4 activation buffers [B*T, C], the 2-channel state, the two per-token log-det sums and the cond rows
        assert lib.ttsvits_durnll_workspace_bytes(h, 64, 150) == (4 * 64 * 150 * 192 + 4 * 64 * 150 + 64 * 192) * 4
    finally:
        lib.ttsvits_durnll_destroy(h)


@pytest.mark.parametrize("gin", [0, 4])
def test_packed_bytes_is_the_sum_of_the_tensors(gin):
    import torch_tts_amd as T

    sdp = T.StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin_channels=gin)
    tensors = sdp.nll_weight_tensors()
    eng = T.vits2.DurNllEngine(sdp._nll_cfg, None)
    try:
        assert int(eng._fn("num_weight_tensors")(eng._h)) == len(tensors) == 284 + (2 if gin else 0)
        up = lambda n: (n + 63) // 64 * 64  # noqa: E731  (every tensor starts on the blob's 256-byte grid)
        assert int(eng._fn("packed_bytes")(eng._h)) == 4 * sum(up(t.numel()) for t in tensors)
        assert sum(t.numel() for t in tensors) == sum(p.numel() for p in sdp.parameters())
        assert len({id(t) for t in tensors}) == len(tensors) == len(list(sdp.parameters()))
    finally:
        eng.close()


def test_module_refusals_and_what_stays():
    import torch_tts_amd as T

    sdp = T.StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin_channels=0)
    x, m, w = torch.zeros(1, 32, 5), torch.ones(1, 1, 5), torch.ones(1, 1, 5)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        sdp.nll(x, m, w)  # CPU tensors
    with pytest.raises(NotImplementedError):
        sdp.nll(x, m, w)  # grad mode
    with torch.no_grad(), pytest.raises(NotImplementedError):
        sdp.nll(x.double(), m, w)  # fp64
    with torch.no_grad(), pytest.raises(NotImplementedError):
        sdp.nll_cl(x.transpose(1, 2), torch.tensor([5]), w[:, 0])
    with pytest.raises(NotImplementedError, match="nll"):
        sdp(x, m, w=w)  # the forward call keeps raising, and names the method
    assert len(sdp.weight_tensors()) == 114
    with pytest.raises(TypeError):
        T.vits2.duration_loss(torch.nn.Module(), torch.zeros(1, 3, dtype=torch.long), torch.tensor([3]), torch.zeros(1, 16, 8), torch.tensor([8]))
    assert callable(T.vits2.duration_loss_from_audio)
