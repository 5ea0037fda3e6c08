"""Host-side checks of the VITS2 duration predictors and length regulation (vits2/models.py:29-180, 1288-1320): the drop-ins'
parameters against the reference's, the ttsdur_* C ABI's refusals, and the fp64 restatement below - the oracle of
tests/test_duration_hip.py - against the reference's own outputs (tests/golden/make_golden_duration.py), including that each of
five plausible slips in it would fail that comparison.  No GPU needed."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "duration_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "duration_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def weights(sd, prefix):
    pre = f"{prefix}/w/"
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _ln(x, sd, p):  # modules.LayerNorm over channels of [B, C, T]
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), sd[p + ".gamma"].double(), sd[p + ".beta"].double(), 1e-5).transpose(1, -1)


def _gelu(x, slip):
    return F.gelu(x, approximate="tanh") if "tanh_gelu" in slip else F.gelu(x)


def dds_conv(sd, p, x, x_mask, g=None, n_layers=3, k=3, slip=()):
    """modules.DDSConv.forward (modules.py:116-127)."""
    if g is not None:
        x = x + g
    C = x.shape[1]
    for i in range(n_layers):
        d = 1 if "no_dilation" in slip else k**i
        y = F.conv1d(x * x_mask, sd[f"{p}.convs_sep.{i}.weight"].double(), sd[f"{p}.convs_sep.{i}.bias"].double(), dilation=d,
                     padding=(k * d - d) // 2, groups=C)
        y = _gelu(_ln(y, sd, f"{p}.norms_1.{i}"), slip)
        y = F.conv1d(y, sd[f"{p}.convs_1x1.{i}.weight"].double(), sd[f"{p}.convs_1x1.{i}.bias"].double())
        y = _gelu(_ln(y, sd, f"{p}.norms_2.{i}"), slip)
        x = x + y
    return x * x_mask


def spline_inverse(x, uw, uh, ud, tail=5.0, slip=()):
    """transforms.unconstrained_rational_quadratic_spline(inverse=True, tails='linear') for x [N], uw / uh [N, nb], ud [N, nb-1]."""
    mn = 1e-3
    nb = uw.shape[-1]
    out = x.clone()
    inside = (x >= -tail) & (x <= tail)
    if not inside.any():
        return out
    xi, uw, uh, ud = x[inside], uw[inside], uh[inside], ud[inside]
    const = math.log(math.exp(1 - mn) - 1)
    ud = F.pad(ud, (1, 1))
    ud[..., 0] = const
    ud[..., -1] = const

    def cum(u):
        w = mn + (1 - mn * nb) * F.softmax(u, dim=-1)
        cw = F.pad(torch.cumsum(w, -1), (1, 0))
        cw = 2 * tail * cw - tail
        cw[..., 0], cw[..., -1] = -tail, tail
        return cw, cw[..., 1:] - cw[..., :-1]

    cw, widths = cum(uw)
    ch, heights = cum(uh)
    der = mn + F.softplus(ud)
    edges = ch.clone()
    if "searchsorted_no_eps" not in slip:
        edges[..., -1] += 1e-6
    idx = (torch.sum(xi[..., None] >= edges, dim=-1) - 1)[..., None]  # (without the eps, x = +5 gets bin nb: gather refuses)
    g = lambda t, j=idx: t.gather(-1, j)[..., 0]  # noqa: E731
    icw, ibw, ich, ih = g(cw), g(widths), g(ch), g(heights)
    delta = g(heights / widths)
    d0, d1 = g(der), g(der[..., 1:])
    xs = xi - ich
    a = xs * (d0 + d1 - 2 * delta) + ih * (delta - d0)
    b = ih * d0 - xs * (d0 + d1 - 2 * delta)
    c = -delta * xs
    root = (2 * c) / (-b - torch.sqrt(b.pow(2) - 4 * a * c))
    out[inside] = root * ibw + icw
    return out


def conv_flow_reverse(sd, p, z, x_mask, g, slip=(), probe=None):
    """modules.ConvFlow.forward(reverse=True) (modules.py:484-516), in_channels 2, num_bins 10.  probe: a list that receives the
    spline's in-length inputs x1."""
    x0, x1 = z[:, :1], z[:, 1:]
    if probe is not None:
        probe.append(x1[x_mask.expand_as(x1) > 0])
    C = sd[p + ".pre.weight"].shape[0]
    h = F.conv1d(x0, sd[p + ".pre.weight"].double(), sd[p + ".pre.bias"].double())
    h = dds_conv(sd, p + ".convs", h, x_mask, g=g, slip=slip)
    h = F.conv1d(h, sd[p + ".proj.weight"].double(), sd[p + ".proj.bias"].double()) * x_mask
    B, _, T = x0.shape
    h = h.reshape(B, 1, -1, T).permute(0, 1, 3, 2)
    uw, uh, ud = h[..., :10] / math.sqrt(C), h[..., 10:20] / math.sqrt(C), h[..., 20:]
    y1 = spline_inverse(x1.reshape(-1), uw.reshape(-1, 10), uh.reshape(-1, 10), ud.reshape(-1, 9), slip=slip).reshape(B, 1, T)
    return torch.cat([x0, y1], 1) * x_mask


def sdp_reverse(sd, x, x_mask, noise, noise_scale=1.0, g=None, n_flows=4, slip=(), probe=None):
    """StochasticDurationPredictor.forward(reverse=True) (models.py:80-137) with the noise given: -> logw [B, 1, T] fp64.
    slip: test aid - 'keep_dropped_flow', 'drop_wrong_flow', 'missing_flip', 'tanh_gelu', 'no_dilation', 'searchsorted_no_eps';
    probe: a list that receives every inverse spline's in-length inputs, in the order the splines run."""
    x, x_mask, noise = x.double(), x_mask.double(), noise.double()
    x = F.conv1d(x, sd["pre.weight"].double(), sd["pre.bias"].double())
    if g is not None:
        x = x + F.conv1d(g.double(), sd["cond.weight"].double(), sd["cond.bias"].double())
    x = dds_conv(sd, "convs", x, x_mask, slip=slip)
    x = F.conv1d(x, sd["proj.weight"].double(), sd["proj.bias"].double()) * x_mask
    # reversed([EA, CF1, Flip, CF2, Flip, ..., CFn, Flip]) without CF1 (models.py:127-128)
    seq = []
    for k in range(n_flows, 0, -1):
        seq += ["flip", f"flows.{2 * k - 1}"]
    if "keep_dropped_flow" not in slip and "drop_wrong_flow" not in slip:
        seq = seq[:-1]
    if "missing_flip" in slip:
        seq.remove("flip")
    if "drop_wrong_flow" not in slip:  # (the slip: flows[:-1] - ElementwiseAffine dropped, flows.1 kept)
        seq.append("ea")
    z = noise * noise_scale
    for f in seq:
        if f == "flip":
            z = torch.flip(z, [1])
        elif f == "ea":
            z = (z - sd["flows.0.m"].double()) * torch.exp(-sd["flows.0.logs"].double()) * x_mask
        else:
            z = conv_flow_reverse(sd, f, z, x_mask, x, slip=slip, probe=probe)
    return z[:, :1]


def dp_forward(sd, x, x_mask, g=None):
    """DurationPredictor.forward (models.py:166-180): -> logw [B, 1, T] fp64."""
    x, x_mask = x.double(), x_mask.double()
    if g is not None:
        x = x + F.conv1d(g.double(), sd["cond.weight"].double(), sd["cond.bias"].double())
    for i in (1, 2):
        x = F.conv1d(x * x_mask, sd[f"conv_{i}.weight"].double(), sd[f"conv_{i}.bias"].double(), padding=1)
        x = _ln(torch.relu(x), sd, f"norm_{i}")
    return F.conv1d(x * x_mask, sd["proj.weight"].double(), sd["proj.bias"].double()) * x_mask


def length_regulate(logw, x_mask, m_p, logs_p, e_z, noise_scale=1.0, length_scale=1.0):
    """models.py:1304-1320 with commons.generate_path (dense, as the reference): logw [B, 1, T_x], m_p / logs_p [B, C, T_x],
    e_z [B, C, >= T_y] -> dict of w_ceil, y_len, y_mask, attn [B, 1, T_y, T_x], m_p, logs_p, z_p [B, C, T_y] (fp64 where not
    integer).  The durations are computed in fp32 as the reference computes them."""
    w = torch.exp(logw.float()) * x_mask.float() * length_scale
    w_ceil = torch.ceil(w)
    y_len = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    T_y = int(y_len.max())
    y_mask = (torch.arange(T_y)[None, :] < y_len[:, None]).unsqueeze(1).to(torch.float64)
    cum = torch.cumsum(w_ceil[:, 0].double(), -1)  # [B, T_x]
    t = torch.arange(T_y, dtype=torch.float64)
    path = (t[None, :, None] < cum[:, None, :]).double()  # [B, T_y, T_x]
    path = path - F.pad(path, (1, 0))[:, :, :-1]
    attn = (path * x_mask.double()[:, :, None, :][:, 0] * y_mask[:, 0, :, None]).unsqueeze(1)
    mp = torch.matmul(attn[:, 0], m_p.double().transpose(1, 2)).transpose(1, 2)
    lp = torch.matmul(attn[:, 0], logs_p.double().transpose(1, 2)).transpose(1, 2)
    z_p = mp + e_z.double()[:, :, :T_y] * torch.exp(lp) * noise_scale
    return dict(w=w, w_ceil=w_ceil, y_len=y_len, y_mask=y_mask, attn=attn, m_p=mp, logs_p=lp, z_p=z_p)


# ---------------------------------------------------------------------------------------------------------------------------
# the infer fixtures' weights: redrawn (tests/golden/make_golden_duration.randomize), checked against the recorded sums
# ---------------------------------------------------------------------------------------------------------------------------
def randomize(mod, seed):
    gsd = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("gamma"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gsd))
            elif n.endswith("weight_g"):
                p.copy_(0.6 + 0.4 * torch.rand(p.shape, generator=gsd))
            elif p.dim() >= 2 and not n.endswith((".m", ".logs")) and "emb" not in n:
                fan_in = p[0].numel() if ".ups." not in f".{n}" else p.shape[0] * p.shape[2]
                scale = 1.5 if ("flows" in n and "proj" in n) else 1.0
                p.copy_(scale * torch.randn(p.shape, generator=gsd) / fan_in**0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gsd))
    return mod


class Net(nn.Module):
    """The inference half of SynthesizerTrn (models.py:1159-1212) built from the drop-ins: enc_p, dp, flow, dec (, emb_g)."""

    def __init__(self, d, use_sdp, n_speakers=0, gin_channels=0):
        super().__init__()
        import torch_tts_amd as T

        V = T.vits2
        self.use_sdp = use_sdp
        self.enc_p = V.TextEncoder(d["n_vocab"], d["inter_channels"], d["hidden_channels"], d["filter_channels"], d["n_heads"], d["n_layers"],
                                   d["kernel_size"], d["p_dropout"])
        self.dec = V.Generator(d["inter_channels"], d["resblock"], d["resblock_kernel_sizes"], d["resblock_dilation_sizes"], d["upsample_rates"],
                               d["upsample_initial_channel"], d["upsample_kernel_sizes"], gin_channels=gin_channels)
        self.flow = V.ResidualCouplingTransformersBlock(d["inter_channels"], d["hidden_channels"], 5, 1, 4, gin_channels=gin_channels,
                                                        use_transformer_flows=True, transformer_flow_type="pre_conv")
        if use_sdp:
            self.dp = V.StochasticDurationPredictor(d["hidden_channels"], 192, 3, 0.5, 4, gin_channels=gin_channels)
        else:
            self.dp = V.DurationPredictor(d["hidden_channels"], 256, 3, 0.5, gin_channels=gin_channels)
        if n_speakers > 1:
            self.emb_g = nn.Embedding(n_speakers, gin_channels)


def infer_net(meta, name):
    """The drop-in model of one infer fixture, its weights redrawn and checked against the recorded checksums."""
    c = meta["infer"][name]
    net = Net(meta["net"], c["use_sdp"], c["n_speakers"], c["gin_channels"])
    for part, seed in c["seeds"].items():
        if hasattr(net, part):
            randomize(getattr(net, part), seed)
    with torch.no_grad():
        if c["use_sdp"]:
            net.dp.flows[0].m.copy_(torch.tensor([[-0.8], [0.0]]))
            net.dp.flows[0].logs.copy_(torch.tensor([[0.4], [0.0]]))
        else:
            net.dp.proj.bias.fill_(1.0)
    assert sorted(c["checksums"]) == sorted(p for p in c["seeds"] if hasattr(net, p))
    for part, want in c["checksums"].items():
        vs = [v.double() for v in getattr(net, part).state_dict().values()]
        got = [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
               float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]
        assert got[:2] == want[:2] and all(abs(a - b) <= 1e-9 * max(1.0, abs(want[3]) * len(vs)) for a, b in zip(got[2:], want[2:])), part
    return net.eval()


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def _T():
    import torch_tts_amd as T

    return T


def _rel(a, b):
    return float(((a.double() - b.double()).abs() / (1e-5 / 1e-4 + b.double().abs())).max())


def _sdp_case(sd, meta, gin, slip=()):
    g = sd["case/g4"] if gin else None
    return sdp_reverse(weights(sd, f"sdp{gin}"), sd["case/x"], sd["case/x_mask"], sd["case/noise"], meta["sdp_noise_scale"], g, slip=slip)


def test_restatement_reproduces_reference_predictors():
    sd, meta = load_golden()
    for gin in (0, 4):
        got = _sdp_case(sd, meta, gin)
        assert got.shape == sd[f"sdp{gin}/logw"].shape
        assert (got - sd[f"sdp{gin}/logw"].double()).abs().max() < 1e-5, gin
        g = sd["case/g4"] if gin else None
        got = dp_forward(weights(sd, f"dp{gin}"), sd["case/x"], sd["case/x_mask"], g)
        assert (got - sd[f"dp{gin}/logw"].double()).abs().max() < 1e-5, gin
        assert sd[f"sdp{gin}/logw"].abs().max() > 0.5  # (not an identity chain)


def test_the_dropped_flow_cannot_reach_logw():
    """Keeping flows.1 (models.py:128 drops it) changes only channel 1, which the reverse pass discards: no logw comparison can
    see it - the reason the reference calls it useless.  The kernel's launch schedule is what keeps it out;
    dropping the wrong element instead (flows[:-1]) is caught below."""
    sd, meta = load_golden()
    for gin in (0, 4):
        assert _rel(_sdp_case(sd, meta, gin, slip=("keep_dropped_flow",)), sd[f"sdp{gin}/logw"]) < 1e-4


@pytest.mark.parametrize("slip", ["drop_wrong_flow", "missing_flip", "tanh_gelu", "no_dilation", "searchsorted_no_eps"])
def test_fixture_catches_slips(slip):
    """Each slip in the restatement must fail the comparison the GPU tests use (logw relative error <= 1e-4)."""
    sd, meta = load_golden()
    errs = []
    for gin in (0, 4):
        if slip == "searchsorted_no_eps":
            # the fixture holds a spline input of exactly +5 (the first ConvFlow's x1 of utterance 2): without the eps on the last
            # edge it falls past the last bin, and the reference's own gather refuses the index
            with pytest.raises(RuntimeError):
                _sdp_case(sd, meta, gin, slip=(slip,))
            errs.append(math.inf)
        else:
            errs.append(_rel(_sdp_case(sd, meta, gin, slip=(slip,)), sd[f"sdp{gin}/logw"]))
    assert min(errs) > 1e-3, (slip, errs)


def test_length_regulation_restatement_matches_reference_infer():
    sd, meta = load_golden()
    for name, c in meta["infer"].items():
        lengths = sd[f"{name}/lengths"]
        T_x = sd[f"{name}/ids"].shape[1]
        x_mask = (torch.arange(T_x)[None, :] < lengths[:, None]).unsqueeze(1).float()
        # m / logs of the text encoder are not recorded: recover them from the recorded expansion where tokens have frames
        lr = length_regulate(sd[f"{name}/logw"], x_mask, torch.zeros(3, 16, T_x), torch.zeros(3, 16, T_x), sd[f"{name}/e_z"],
                             c["args"]["noise_scale"], c["args"]["length_scale"])
        assert lr["y_len"].tolist() == c["y_lengths"], name
        assert torch.equal(lr["y_mask"].float(), sd[f"{name}/y_mask"]), name
        assert torch.equal(lr["attn"].float(), sd[f"{name}/attn"]), name
        # the reference's m_p / logs_p are attn-expansions of per-token rows, and z_p follows the formula
        ref_mp, ref_lp = sd[f"{name}/m_p"].double(), sd[f"{name}/logs_p"].double()
        T_y = ref_mp.shape[2]
        zp = ref_mp + sd[f"{name}/e_z"].double()[:, :, :T_y] * torch.exp(ref_lp) * c["args"]["noise_scale"]
        assert (zp - sd[f"{name}/z_p"].double()).abs().max() < 1e-5, name


def test_state_dicts_match_reference_records():
    _, meta = load_golden()
    T = _T()
    sdp = T.StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=0)
    assert [[k, list(v.shape)] for k, v in sdp.state_dict().items()] == meta["fulldims_sdp_state_dict"]
    dp = T.DurationPredictor(192, 256, 3, 0.5, gin_channels=0)
    assert [[k, list(v.shape)] for k, v in dp.state_dict().items()] == meta["fulldims_dp_state_dict"]
    sd, _ = load_golden()
    for gin in (0, 4):
        for kind, cls, args in (("sdp", T.StochasticDurationPredictor, (32, 192, 3, 0.5, 4)), ("dp", T.DurationPredictor, (32, 48, 3, 0.5))):
            m = cls(*args, gin_channels=gin)
            ref = weights(sd, f"{kind}{gin}")
            assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.items()]
            m.load_state_dict(ref, strict=True)
    for name in meta["infer"]:
        infer_net(meta, name)  # (the drop-in model's keys and redrawn weights equal the reference model's)


def _dur_dims(**over):
    from torch_tts_amd import _lib

    d = _lib.DurDims(0, 192, 192, 3, 4, 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_c_abi_symbols_refusals_and_not_bound():
    import re

    from torch_tts_amd import _lib

    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ttsdur_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.DUR_SYMBOLS) and len(declared) == 12, declared ^ set(_lib.DUR_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s
    assert not set(_lib.DUR_SYMBOLS) & set(_lib.SYMBOLS + _lib.GEN_SYMBOLS)
    assert lib.ttsdec_version() == 2
    h = C.c_void_p()
    for bad in (dict(kind=2), dict(kernel_size=5), dict(in_channels=190), dict(in_channels=512), dict(n_flows=1), dict(kind=1, filter_channels=258),
                dict(gin_channels=-1)):
        assert lib.ttsdur_create(C.byref(_dur_dims(**bad)), C.byref(h)) == _lib.ERR_DIMS, bad
    assert lib.ttsdur_create(C.byref(_dur_dims()), C.byref(h)) == _lib.OK
    try:
        assert lib.ttsdur_num_weight_tensors(h) == 114
        vp = C.c_void_p(256)
        ws = 1 << 40
        assert lib.ttsdur_sdp_reverse(h, vp, vp, None, vp, 1.0, 2, 8, vp, vp, ws, None) == _lib.ERR_NOT_BOUND
        assert lib.ttsdur_sdp_reverse(h, vp, vp, vp, vp, 1.0, 2, 8, vp, vp, ws, None) == _lib.ERR_INVALID_ARG  # g with gin = 0
        assert lib.ttsdur_sdp_reverse(h, vp, vp, None, None, 1.0, 2, 8, vp, vp, ws, None) != _lib.OK  # no noise
        assert lib.ttsdur_dp_forward(h, vp, vp, None, 2, 8, vp, vp, ws, None) == _lib.ERR_INVALID_ARG  # wrong kind
        assert lib.ttsdur_sdp_reverse(h, vp, vp, None, vp, 1.0, 0, 8, vp, vp, ws, None) == _lib.ERR_INVALID_ARG
        # 4 activation buffers [B*T, C], the 2-channel state and the cond rows
        assert lib.ttsdur_workspace_bytes(h, 64, 150) == (4 * 64 * 150 * 192 + 2 * 64 * 150 + 64 * 192) * 4
    finally:
        lib.ttsdur_destroy(h)
    assert lib.ttsdur_create(C.byref(_dur_dims(kind=1, filter_channels=256, gin_channels=4)), C.byref(h)) == _lib.OK
    try:
        assert lib.ttsdur_num_weight_tensors(h) == 12
    finally:
        lib.ttsdur_destroy(h)


def test_modules_refuse_what_is_outside_the_path():
    T = _T()
    sdp = T.StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin_channels=0)
    dp = T.DurationPredictor(32, 48, 3, 0.5)
    x, m = torch.zeros(1, 32, 5), torch.ones(1, 1, 5)
    with pytest.raises(NotImplementedError):
        sdp(x, m, w=torch.ones(1, 1, 5))  # the training direction
    with torch.no_grad(), pytest.raises(NotImplementedError):
        sdp(x, m, reverse=True)  # CPU tensors
    with torch.no_grad(), pytest.raises(NotImplementedError):
        dp(x, m)
    with pytest.raises(NotImplementedError):
        sdp(x, m, reverse=True)  # grad mode (checked before the device)
    with pytest.raises(TypeError):
        T.vits2.infer(nn.Module(), torch.zeros(1, 3, dtype=torch.long), torch.tensor([3]))


def test_new_exports():
    T = _T()
    assert T.StochasticDurationPredictor is T.vits2.StochasticDurationPredictor and T.DurationPredictor is T.vits2.DurationPredictor
    assert callable(T.vits2.infer) and {"StochasticDurationPredictor", "DurationPredictor"} <= set(T.__all__)
