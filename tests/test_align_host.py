"""Host-side checks of monotonic alignment search (vits2/models.py:1224-1254, monotonic_align/core.pyx:7-33): the numpy / torch
restatement that the GPU tests (tests/test_align_hip.py) use as their oracle is pinned here against the reference's own paths
(tests/golden/make_golden_align.py: the reference's core.pyx, compiled, called as its wrapper calls it) and against brute-force
enumeration of every monotonic path; plus the C-ABI exports and the refusals of the Python entry points.  No GPU."""
import itertools
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_duration_host import randomize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEG = np.float32(-1e9)  # core.pyx max_neg_val
ALONE_TX = (1, 2, 63, 64, 65, 129)  # tokens of the stand-alone cases: around the lane and column-run boundaries of the kernel


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "align_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "align_meta.json")))
    return {k: z[k] for k in z.files}, meta


# ---------------------------------------------------------------------------------------------------------------------------
# restatement
# ---------------------------------------------------------------------------------------------------------------------------
def mas_frame_token(value, t_y, t_x):
    """core.pyx maximum_path_each on one utterance, one numpy row operation per frame: value [>= t_y, >= t_x] fp32 (not modified)
    -> frame_token [t_y] (the token of each frame).  fp32 `+` and compare-select in the reference's order; the backtrack needs only
    the bit `v_cur < v_prev` of each cell and the reference's `index == y` rule."""
    assert 1 <= t_x <= t_y, (t_y, t_x)  # (outside this the reference reads out of bounds)
    v = np.array(value[:t_y, :t_x], dtype=np.float32, copy=True)
    bits = np.zeros(v.shape, bool)
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        xs = np.arange(lo, hi)
        if y == 0:
            v_cur, v_prev = np.full(len(xs), NEG), np.zeros(len(xs), np.float32)  # (the band of row 0 is x = 0 alone)
        else:
            v_cur = np.where(xs == y, NEG, v[y - 1, lo:hi])
            v_prev = np.where(xs == 0, NEG, v[y - 1, np.maximum(xs - 1, 0)])
        bits[y, lo:hi] = v_cur < v_prev
        v[y, lo:hi] = v[y, lo:hi] + np.where(v_cur > v_prev, v_cur, v_prev).astype(np.float32)
    ft = np.zeros(t_y, np.int32)
    idx = t_x - 1
    for y in range(t_y - 1, -1, -1):
        ft[y] = idx
        if idx != 0 and (idx == y or bits[y, idx]):
            idx -= 1
    return ft


def mas_batch(neg_cent, t_ys, t_xs):
    """-> frame_token [B, T_y] int32 (-1 at padded frames), dur [B, T_x] int32, path [B, T_y, T_x] fp32 of a batch."""
    neg_cent = np.asarray(neg_cent, np.float32)
    B, T_y, T_x = neg_cent.shape
    ft = np.full((B, T_y), -1, np.int32)
    dur = np.zeros((B, T_x), np.int32)
    path = np.zeros((B, T_y, T_x), np.float32)
    for b in range(B):
        ty, tx = int(t_ys[b]), int(t_xs[b])
        ft[b, :ty] = mas_frame_token(neg_cent[b], ty, tx)
        path[b, np.arange(ty), ft[b, :ty]] = 1.0
        dur[b] = path[b].sum(0).astype(np.int32)
    return ft, dur, path


def neg_cent_torch(z_p, m_p, logs_p):
    """models.py:1226-1239 in the operands' dtype, the reference's operations in its order: z_p [B, C, T_y], m_p / logs_p
    [B, C, T_x] -> neg_cent [B, T_y, T_x]."""
    s_p_sq_r = torch.exp(-2 * logs_p)
    nc1 = torch.sum(-0.5 * math.log(2 * math.pi) - logs_p, [1], keepdim=True)
    nc2 = torch.matmul(-0.5 * (z_p**2).transpose(1, 2), s_p_sq_r)
    nc3 = torch.matmul(z_p.transpose(1, 2), (m_p * s_p_sq_r))
    nc4 = torch.sum(-0.5 * (m_p**2) * s_p_sq_r, [1], keepdim=True)
    return nc1 + nc2 + nc3 + nc4


def neg_cent_inputs(seed, B, C, T_y, T_x):
    """The operands of the neg_cent error measurements: z_p, m_p ~ N(0, 1), logs_p ~ U[-3.5, 1] (exp(-2 logs_p) from 0.1 to 1e3, so the
    four terms cancel against each other) - fp32, [B, C, T]."""
    g = torch.Generator().manual_seed(seed)
    z_p = torch.randn(B, C, T_y, generator=g)
    m_p = torch.randn(B, C, T_x, generator=g)
    logs_p = torch.rand(B, C, T_x, generator=g) * 4.5 - 3.5
    return z_p, m_p, logs_p


def rel_err(a, ref):
    """max |a - ref| / max |ref| (ref fp64)."""
    return float((a.double() - ref).abs().max() / ref.abs().max())


def alone_cases():
    """(name, t_y, t_x) of the stand-alone cases of the fixture; costs are in the npz under alone/<name>."""
    out = []
    for tx in ALONE_TX:
        for ty in sorted({tx, 4 * tx + 7}):
            out.append((f"int_{ty}x{tx}", ty, tx))
    for tx in (1, 2, 65):
        out.append((f"frac_{3 * tx + 2}x{tx}", 3 * tx + 2, tx))
    return out


def alone_costs(name, t_y, t_x):
    """Integer-valued costs in [-3, 3] (ties at almost every cell), or multiples of 1 / 64 (ties rare): both exact in fp32."""
    rng = np.random.default_rng(sum(name.encode()) * 1000 + t_y * 7 + t_x)
    if name.startswith("int"):
        return rng.integers(-3, 4, (t_y, t_x)).astype(np.float32)
    return (rng.integers(-2000, 2001, (t_y, t_x)) / 64.0).astype(np.float32)


class AlignNet(nn.Module):
    """The forced-alignment half of SynthesizerTrn (models.py:1159-1212) built from the drop-ins: enc_p, enc_q, flow (, emb_g)."""

    def __init__(self, d, n_speakers, gin_channels):
        super().__init__()
        import torch_tts_amd as T

        V = T.vits2
        self.enc_p = V.TextEncoder(d["n_vocab"], d["inter_channels"], d["hidden_channels"], d["filter_channels"], d["n_heads"], d["n_layers"],
                                   d["kernel_size"], d["p_dropout"])
        self.enc_q = V.PosteriorEncoder(d["spec_channels"], d["inter_channels"], d["hidden_channels"], 5, 1, 16, gin_channels=gin_channels)
        self.flow = V.ResidualCouplingTransformersBlock(d["inter_channels"], d["hidden_channels"], 5, 1, 4, gin_channels=gin_channels,
                                                        use_transformer_flows=True, transformer_flow_type="pre_conv")
        if n_speakers > 1:
            self.emb_g = nn.Embedding(n_speakers, gin_channels)


def checksum(mod):
    vs = [v.double() for v in mod.state_dict().values()]
    return [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
            float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]


def align_net(meta):
    """The drop-in model of the fixture, its weights redrawn and checked against the recorded checksums."""
    c = meta["model"]
    net = AlignNet(meta["net"], c["n_speakers"], c["gin_channels"])
    for part, seed in c["seeds"].items():
        randomize(getattr(net, part), seed)
    for part, want in c["checksums"].items():
        got = checksum(getattr(net, part))
        assert got[:2] == want[:2] and all(abs(a - b) <= 1e-9 * max(1.0, abs(want[3]) * got[0]) for a, b in zip(got[2:], want[2:])), part
    return net.eval()


def forced_alignment_host(net, x, x_lengths, y, y_lengths, sid, noise, dtype=torch.float64):
    """SynthesizerTrn.forward up to neg_cent (models.py:1214-1239) chained from the oracles of enc_p, enc_q and the flow's forward
    direction over a model's state dicts, in dtype: -> z, z_p, m_p, logs_p ([B, C, T]) and neg_cent [B, T_y, T_x]."""
    from oracle import vits2_oracle as V
    from test_vc_host import _cast, flow_dims, flow_forward, posterior_encoder

    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    part = lambda p: {k[len(p) + 1:]: v for k, v in sd.items() if k.startswith(p + ".")}  # noqa: E731
    g = None if sid is None else sd["emb_g.weight"].to(dtype)[sid.cpu()].unsqueeze(-1)
    ep = net.enc_p
    d = V.Vits2Dims(n_vocab=ep.n_vocab, inter_channels=ep.out_channels, hidden_channels=ep.hidden_channels, filter_channels=ep.filter_channels,
                    n_heads=ep.n_heads, n_layers=ep.n_layers, kernel_size=ep.kernel_size)
    _, m_p, logs_p, _ = V.text_encoder(x.cpu(), x_lengths.cpu(), _cast({f"enc_p.{k}": v for k, v in part("enc_p").items()}, dtype), d)
    eq = net.enc_q
    z, _, _, y_mask = posterior_encoder(part("enc_q"), y.detach().cpu().to(dtype), y_lengths.cpu(), g, noise.cpu(), eq.n_layers, eq.kernel_size)
    fl = net.flow
    fd = flow_dims(fl.channels, fl.hidden_channels, fl.kernel_size, fl.n_layers, fl.n_flows, fl.gin_channels)
    z_p = flow_forward(z, y_mask, {f"flow.{k}": v for k, v in part("flow").items()}, fd, g=g)
    return z, z_p, m_p, logs_p, neg_cent_torch(z_p, m_p, logs_p)


def path_score(neg_cent64, ft):
    """fp64 sum of the costs along frame_token."""
    return float(neg_cent64[np.arange(len(ft)), ft].sum())


def best_score(neg_cent64, t_y, t_x):
    """The maximum over all monotonic paths, by the recurrence in fp64."""
    q = np.full(t_x, -np.inf)
    q[0] = neg_cent64[0, 0]
    for y in range(1, t_y):
        q = neg_cent64[y, :t_x] + np.maximum(q, np.concatenate(([-np.inf], q[:-1])))
    return float(q[t_x - 1])


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_paths():
    sd, meta = load_golden()
    n = 0
    for name, ty, tx in alone_cases():
        nc = alone_costs(name, ty, tx)
        assert np.array_equal(sd[f"alone/{name}/neg_cent"].astype(np.float32) / (1.0 if name.startswith("int") else 64.0), nc), name
        assert np.array_equal(mas_frame_token(nc, ty, tx), sd[f"alone/{name}/frame_token"].astype(np.int32)), name
        n += 1
    assert n == len(meta["alone"]) == 2 * len(ALONE_TX) + 3
    # the ragged batch of the model case and of the random batch: the reference's paths on the reference's neg_cent
    for key in ("model", "ragged"):
        ft, dur, path = mas_batch(sd[f"{key}/neg_cent"], sd[f"{key}/t_y"], sd[f"{key}/t_x"])
        assert np.array_equal(ft, sd[f"{key}/frame_token"].astype(np.int32)), key
    _, dur, _ = mas_batch(sd["model/neg_cent"], sd["model/t_y"], sd["model/t_x"])
    assert np.array_equal(dur.astype(np.float32)[:, None, :], sd["model/w"])


def test_neg_cent_restatement_is_the_reference_arithmetic():
    sd, meta = load_golden()
    t = lambda k: torch.from_numpy(sd[k])  # noqa: E731
    nc = neg_cent_torch(t("model/z_p"), t("model/m_p"), t("model/logs_p"))
    # (fp32 on another host's BLAS may order a dot product differently: a few ulp of the largest term)
    assert rel_err(nc, t("model/neg_cent").double()) <= 1e-6
    e = meta["neg_cent_cpu_f32_err"]
    assert 0 < e["golden"] < 1e-5 and 0 < e["c192_600x150"] < 1e-5, e  # what fp32 can be expected to give; sets the GPU test's bar


def test_the_path_is_the_maximum_over_all_monotonic_paths():
    rng = np.random.default_rng(3)

    def brute(v, ty, tx):
        best = -np.inf
        for cuts in itertools.combinations(range(1, ty), tx - 1):
            e = [0, *cuts, ty]
            best = max(best, sum(float(v[e[i]:e[i + 1], i].astype(np.float64).sum()) for i in range(tx)))
        return best

    for ty, tx in ((9, 4), (7, 7), (6, 1), (8, 3), (5, 4)):
        for kind in ("int", "float"):
            v = rng.integers(-3, 4, (ty, tx)).astype(np.float32) if kind == "int" else rng.standard_normal((ty, tx)).astype(np.float32)
            ft = mas_frame_token(v, ty, tx)
            assert ft[0] == 0 and ft[-1] == tx - 1 and set(np.diff(ft)) <= {0, 1}
            b = brute(v, ty, tx)
            assert abs(best_score(v.astype(np.float64), ty, tx) - b) < 1e-9
            s = path_score(v.astype(np.float64), ft)
            assert s == b if kind == "int" else s >= b - 1e-4, (ty, tx, kind, s, b)


def test_new_ttsvits_symbols_are_declared_bound_and_exported():
    import torch_tts_amd as T
    from torch_tts_amd import _lib

    new = ("ttsvits_align_workspace_bytes", "ttsvits_neg_cent", "ttsvits_maximum_path", "ttsvits_align")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in new:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsvits"] and hasattr(lib, sym), sym
    assert lib.ttsdec_version() == 2
    # host-only: sizes and refusals that need no device, on the weightless handle the stand-alone calls use
    eng = T.vits2.VitsEngine(T.vits2._ALIGN_DIMS, None)
    h = eng._h
    assert lib.ttsvits_align_workspace_bytes(h, 64, 600, 150) == 64 * 600 * 64
    assert lib.ttsvits_align_workspace_bytes(h, 1, 2000, 1024) == 2000 * 128 and lib.ttsvits_align_workspace_bytes(h, 1, 10, 1025) == 0
    one = 256  # (non-null placeholders: the size checks come first)
    assert lib.ttsvits_maximum_path(h, one, one, one, 1, 10, 1025, None, 0, one, one, one, one, 1 << 20, None) == _lib.ERR_DIMS
    assert lib.ttsvits_maximum_path(h, one, one, one, 1, 10, 0, None, 0, one, one, one, one, 1 << 20, None) == _lib.ERR_INVALID_ARG
    assert lib.ttsvits_maximum_path(h, one, one, one, 1, 10, 8, None, 0, one, one, one, one, 64, None) == _lib.ERR_WORKSPACE
    assert lib.ttsvits_neg_cent(h, one, one, one, None, None, 1, 10, 8, 6, one, None) == _lib.ERR_DIMS  # C not a multiple of 4
    eng.close()


def test_entry_points_refuse_what_is_not_on_the_path():
    import torch_tts_amd as T

    V = T.vits2
    _, meta = load_golden()
    net = align_net(meta)
    x, xl = torch.zeros(1, 5, dtype=torch.long), torch.tensor([5])
    y, yl = torch.zeros(1, meta["net"]["spec_channels"], 9), torch.tensor([9])
    with torch.no_grad(), pytest.raises(NotImplementedError):
        V.forced_alignment(net, x, xl, y, yl)  # CPU tensors: no fallback
    with pytest.raises(NotImplementedError):
        V.maximum_path(torch.zeros(1, 4, 2), torch.ones(1, 4, 2))
    with pytest.raises(NotImplementedError):
        V.align(torch.zeros(1, 4, 6), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.ones(1, 1, 3), torch.ones(1, 1, 6))
    for part in ("enc_p", "enc_q", "flow"):
        keep = getattr(net, part)
        setattr(net, part, nn.Identity())
        with pytest.raises(TypeError, match=part):
            V.forced_alignment(net, x, xl, y, yl)
        setattr(net, part, keep)
