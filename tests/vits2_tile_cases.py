"""The VITS2 row GEMMs on every tile and K-walk length the dispatcher can give them: the case table of
tests/test_vits2_tiles_host.py and tests/test_vits2_tiles_hip.py (and of tests/golden/make_golden_vits2_tiles.py, which runs the
REFERENCE's modules at these dims), with two restatements the host test pins to the source text:

  gemm_tile   decode_kernels.hip launch_gemm_cfg for launch_gemm<A_PLAIN | A_CONV, EPI_GENERIC> behind vits2.hip gemm_generic
  gemm_list   the 13 gemm_generic call sites of vits2.hip, as the GEMMs of one text encoder / flow / posterior encoder call

Every GEMM of the three families goes through gemm_generic; tests/vits2_dims_corner_cases.py runs their dims corners at M = 111 or
27 rows (the 32 x 32 fp32 tile and the 64 x 64 split tile), the ModelConfig tests the large-M tiles at widths that are whole column
tiles with long K walks.  The cases here put ragged column and row tiles, K walks of 1 ... S + 1 stages that end inside a stage, taps
that straddle a stage, mixed exact / split chains and both sides of the two M switches on the three large-M tiles.

The modules are filled by recipes.fill_by_key(module, seed, gain), as the corner table's; nothing stores a weight.  Layouts are
(B, T, lengths): large M comes from the batch where there is attention (B <= 31 and T odd, so that no utterance boundary b * T is a
multiple of 32, 64 or 128: every boundary lies strictly inside a row tile of every tile), T stays inside what the attention kernels
take at these head widths (tests/vits2_attention_cases.py: <= 1165 frames), and the lengths hold T, 1 and values in between.

Gains.  The fp32 restatement must stay within half of the bar from its fp64 evaluation at each case's real shape
(tests/test_vits2_tiles_host.py test_margin).  It does at the corner table's gains (1.2 text encoder, 0.8 flow and posterior
encoder) for every case - at most 0.39 of the bar (W8's LayerNorm over eight values) - so no gain had to be lowered."""
import functools

import torch

import postnet_corner_cases as P
import recipes
import vits2_dims_corner_cases as K
from hip_helpers import sample_utterances
from oracle import vits2_oracle as V
from test_vc_host import flow_dims, flow_forward, posterior_encoder

N_VOCAB, WINDOW, STRIDE = K.N_VOCAB, K.WINDOW, K.STRIDE
SMALL = (K.B, K.T, tuple(K.LENGTHS))  # the corner table's layout: what the golden file records
LARGE_ROWS = 5000  # beyond this many rows the oracle runs on a sample of the utterances (they never interact)

# ---------------------------------------------------------------------------------------------------------------------------
# gemm_tile
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (BM, BN, k per stage, stages); tests/test_vits2_tiles_host.py derives each row from the TileCfg<...> of its branch
TILES = {
    "f32/32x32k4": (32, 32, 128, 4),
    "f32/64x64": (64, 64, 32, 4),
    "split/64x64": (64, 64, 64, 4),
    "split/128x128": (128, 128, 64, 2),
    "split/lean64": (64, 64, 32, 4),
}
LARGE_TILES = ("f32/64x64", "split/128x128", "split/lean64")
ROW_SWITCH_SPLIT = 2048  # `a.M >= 2048`
ROW_SWITCH_F32 = 10881   # N = 136: ceil(M / 64) * 3 >= 512 from M = 170 * 64 + 1


def gemm_tile(precision, conv, M, N, K):
    """-> (tile name, (k per stage, stages)) of gemm_generic's launch for out [M, N] = A [M, K] . W, K = taps * Cin.
    gemm_generic: `cx.split && !(K & 7)` on the layer's Cin - every kernel is odd, so K & 7 == 0 exactly when Cin & 7 == 0 - keeps
    a layer of a split-fp16 call on exact fp32.  launch_gemm_cfg: the lean tile for A_PLAIN with K <= 256 and M >= 2048, else what
    postnet_corner_cases.shared_tile restates (128 x 128 for N >= 128 and M >= 2048, else 64 x 64; fp32: 64 x 64 from 512 tiles)."""
    split = precision == "split_f16" and not K & 7
    if split and not conv and K <= 256 and M >= ROW_SWITCH_SPLIT:
        name = "split/lean64"
    else:
        t = P.shared_tile("split_f16" if split else "f32", M, N)
        name = ("split/" + t) if split else {"64x64": "f32/64x64", "32x32": "f32/32x32k4"}[t]
    return name, TILES[name][2:]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _lengths(B, T):
    """T, 1 and values in between; the last two utterances whole (the last one's rows are the ragged last row tile, and the frames
    on either side of the boundary in front of it are real)"""
    base = [T, 1, T // 2, T - 1, 2, T // 3, 17]
    return tuple([base[b % len(base)] for b in range(B - 2)] + [T, T])


L2107 = (7, 301, _lengths(7, 301))      # 2107 rows = 16 * 128 + 59 = 32 * 64 + 59: the split-fp16 large tiles
L10881 = (31, 351, _lengths(31, 351))   # 10 881 rows = 170 * 64 + 1: the fp32 64 x 64 tile from three column tiles on
L32705 = (31, 1055, _lengths(31, 1055))  # 32 705 rows = 511 * 64 + 1: the fp32 64 x 64 tile with ONE column tile
# the switches: one utterance; on the upper side its last frame is padding, so both sides compute the same rows
SWITCH_LAYOUTS = ((1, 2047, (2047,)), (1, 2048, (2047,)), (1, 10880, (10880,)), (1, 10881, (10880,)))

TE_CASES = {
    # the walk series: w1 (conv, K = 3 C, N = 136 = 128 + 8 = 2 * 64 + 8) walks K = 24, 48, 72, 120, 144: on the 128 x 128 tile
    # (2107 rows, split) 1, 1, 2, 2, 3 stages of 64 k; on the fp32 64 x 64 tile (10 881 rows) 1, 2, 3, 4, 5 stages of 32 k
    "W8": dict(hidden=8, filter=136, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=201),
    "W16": dict(hidden=16, filter=136, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=202),
    "W24": dict(hidden=24, filter=136, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=203),
    "W40": dict(hidden=40, filter=136, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=204),
    "W48": dict(hidden=48, filter=136, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=205),
    # the mixed chains.  X2 (as E2: C % 8 != 0, F % 8 == 0) at widths that put the split conv_2 on the 128 x 128 tile (N = 132) with
    # its residual: the exact conv_1 in front of it (32 x 32 at 2107 rows, 64 x 64 at 10 881) writes conv_2's planes by partial tiles
    "X2": dict(hidden=132, filter=136, heads=4, layers=2, kernel=5, inter=8, gin=0, cond=0, gain=1.2, seed=206),
    # X3 = E3's dims (C % 8 == 0, F % 8 != 0): a split conv_1 on the 64 x 64 split tile (N = 20) between lean-tile 1x1s, in front
    # of an exact conv_2
    "X3": dict(hidden=32, filter=20, heads=2, layers=3, kernel=7, inter=12, gin=4, cond=0, gain=1.2, seed=207),
}
FLOW_CASES = {
    # ragged widths: half = 48 (wqkv: N = 144), hidden 72: `in` has N = 144 = 128 + 16, Cin = 72 (neither divides 64 or 32 nor is a
    # multiple) under 5 taps, K = 360; `rs` has N = 144 and 72
    "RF": dict(channels=96, hidden=72, kernel=5, wn_layers=2, flows=2, gin=0, gain=0.8, seed=211),
}
POST_CASES = {
    "RQ": dict(spec=29, inter=12, hidden=72, kernel=5, layers=2, gin=4, gain=0.8, seed=221),
    # one column tile (N = 40, 20, 24) at 32 705 rows: hidden % 8 != 0, so in split-fp16 too all but `pre` are exact
    "N1": dict(spec=13, inter=12, hidden=20, kernel=5, layers=1, gin=0, gain=0.8, seed=222),
    # the switches: N = 136 in pre, rs and proj (three column tiles: 510 | 513 fp32 tiles), 272 in `in`
    "S1": dict(spec=40, inter=68, hidden=136, kernel=3, layers=1, gin=0, gain=0.8, seed=223),
}
# the lean-tile walk series: `pre` walks K = the staged spec width (spec rounded up to 8) = 24 ... 168: 1 ... 6 stages of 32 k,
# each ending inside a stage; N = 72 = 64 + 8
LEAN_SPECS = {"L24": 21, "L40": 37, "L72": 69, "L104": 101, "L136": 133, "L168": 165}
for _i, (_n, _s) in enumerate(LEAN_SPECS.items()):
    POST_CASES[_n] = dict(spec=_s, inter=8, hidden=72, kernel=3, layers=1, gin=0, gain=0.8, seed=231 + _i)

FAMILIES = {"te": TE_CASES, "flow": FLOW_CASES, "post": POST_CASES}
LAYOUTS = {n: (L2107, L10881) for n in list(TE_CASES) + ["RF", "RQ"]}
LAYOUTS.update({n: (L2107,) for n in LEAN_SPECS})
LAYOUTS["N1"] = (L32705,)
LAYOUTS["S1"] = SWITCH_LAYOUTS
SWITCH_CASE = "S1"
CASES = [(fam, name) for fam, table in FAMILIES.items() for name in table]
RUNS = [(fam, name, li) for fam, name in CASES for li in range(len(LAYOUTS[name]))]
OUTPUTS = {"te": ("x", "m", "logs"), "flow": ("rev", "fwd"), "post": ("z", "m", "logs")}


def run_id(run):
    fam, name, li = run
    B, T, _ = LAYOUTS[name][li]
    return f"{name}-{B}x{T}"


def spec_pad(spec):
    """ttspost_create: `h->spec_pad = (int)up((size_t)dims->spec_channels, 8);` - K of the posterior encoder's `pre`"""
    return (spec + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_list
# ---------------------------------------------------------------------------------------------------------------------------
def _stack(out, prefix, M, C, F, layers, kernel):
    """run_stack: per layer wqkv, wo (+ residual), w1 (conv, ReLU, mask, planes), w2 (conv, mask, residual)"""
    for i in range(layers):
        out.append((f"{prefix}wqkv.{i}", False, M, 3 * C, C, C, 1, False, False, False))
        out.append((f"{prefix}wo.{i}", False, M, C, C, C, 1, False, True, False))
        out.append((f"{prefix}w1.{i}", kernel > 1, M, F, kernel * C, C, kernel, True, False, True))
        out.append((f"{prefix}w2.{i}", kernel > 1, M, C, kernel * F, F, kernel, True, True, False))


def _wn(out, prefix, M, B, H, layers, kernel, gin):
    """run_wn: cond (M = B, always exact), then per layer `in` (conv, N = 2 H) and `rs` (N = 2 H; H in the last layer)"""
    if gin:
        out.append((f"{prefix}cond", False, B, 2 * H * layers, gin, gin, 1, False, False, False))
    for j in range(layers):
        out.append((f"{prefix}in.{j}", kernel > 1, M, 2 * H, kernel * H, H, kernel, False, False, False))
        out.append((f"{prefix}rs.{j}", False, M, H if j == layers - 1 else 2 * H, H, H, 1, False, False, False))


def gemm_list(family, case, B, T):
    """Every gemm_generic call of one forward call (the flow: of one direction - both run the same GEMMs), in launch order:
    (name, conv, M, N, K_total, Cin, taps, has_mask, has_resid, writes_planes).  The planes pointers are carved in both precisions,
    so writes_planes holds for an exact-fp32 call too."""
    c, M, out = FAMILIES[family][case], B * T, []
    if family == "te":
        C = c["hidden"]
        if c["gin"]:
            out.append(("spk", False, B, C, c["gin"], c["gin"], 1, False, False, False))
        _stack(out, "", M, C, c["filter"], c["layers"], c["kernel"])
        out.append(("proj", False, M, 2 * c["inter"], C, C, 1, True, False, False))
    elif family == "flow":
        half, H = c["channels"] // 2, c["hidden"]
        for k in range(c["flows"]):
            _stack(out, f"{k}.", M, half, half, 2, 3)  # pre_transformer: Encoder(half, half, n_heads=2, n_layers=2, kernel_size=3)
            out.append((f"{k}.pre", False, M, H, half, half, 1, True, False, True))
            _wn(out, f"{k}.", M, B, H, c["wn_layers"], c["kernel"], c["gin"])
            out.append((f"{k}.post", False, M, half, H, H, 1, True, False, False))
    else:
        H, Sp = c["hidden"], spec_pad(c["spec"])
        out.append(("pre", False, M, H, Sp, Sp, 1, True, False, True))
        _wn(out, "", M, B, H, c["layers"], c["kernel"], c["gin"])
        out.append(("proj", False, M, 2 * c["inter"], H, H, 1, True, False, False))
    assert all(g[6] & 1 and g[4] == g[5] * g[6] for g in out)
    return out


def always_exact(name):
    """`cond` and `spk` run under kExact whatever the call's precision"""
    return name.endswith("cond") or name == "spk"


def tiles_of(family, case, layout, precision):
    """[(gemm, tile name, (k per stage, stages))] of one call"""
    B, T, _ = layout
    return [(g,) + gemm_tile("f32" if always_exact(g[0]) else precision, g[1], g[2], g[3], g[4]) for g in gemm_list(family, case, B, T)]


# ---------------------------------------------------------------------------------------------------------------------------
# modules, inputs, the sampled oracle
# ---------------------------------------------------------------------------------------------------------------------------
def make(ns, fam, name):
    """The case's module from namespace `ns` (the reference's `models` or torch_tts_amd.vits2), filled from its seed and gain."""
    c = FAMILIES[fam][name]
    if fam == "te":
        mod = ns.TextEncoder(N_VOCAB, c["inter"], c["hidden"], c["filter"], c["heads"], c["layers"], c["kernel"], 0.1, gin_channels=c["gin"]).eval()
        if c["gin"]:
            mod.encoder.cond_layer_idx = c["cond"]
    elif fam == "flow":
        mod = ns.ResidualCouplingTransformersBlock(c["channels"], c["hidden"], c["kernel"], 1, c["wn_layers"], n_flows=c["flows"],
                                                   gin_channels=c["gin"], use_transformer_flows=True).eval()
    else:
        mod = ns.PosteriorEncoder(c["spec"], c["inter"], c["hidden"], c["kernel"], 1, c["layers"], gin_channels=c["gin"]).eval()
    recipes.fill_by_key(mod, c["seed"], gain=c["gain"])
    return mod


def mask_of(layout):
    B, T, lengths = layout
    return V.sequence_mask(torch.tensor(lengths), T).unsqueeze(1).float()


def inputs(fam, name, layout):
    """The seeded inputs of a case at a layout (as the corner table's: ids of the whole range; z with zero padded frames; y with
    padded frames NOT zero).  The switch layouts cut theirs from the longer side's, so both sides see the same frames."""
    c = FAMILIES[fam][name]
    B, T, lengths = layout
    gen_T = T if layout not in SWITCH_LAYOUTS else 2048 if T <= 2048 else 10881
    seed = c["seed"] * 100 + B
    i = dict(lengths=torch.tensor(lengths), g=recipes.seeded_randn(7000 + seed, B, c["gin"], 1) if c["gin"] else None)
    if fam == "te":
        i["ids"] = recipes.seeded_ids(seed, N_VOCAB, B, gen_T)[:, :T].contiguous()
    elif fam == "flow":
        i["z"] = recipes.seeded_randn(seed, B, c["channels"], gen_T)[:, :, :T].contiguous() * mask_of(layout)
    else:
        i["y"] = recipes.seeded_randn(seed, B, c["spec"], gen_T)[:, :, :T].contiguous()
        i["eps"] = recipes.seeded_randn(9000 + seed, B, c["inter"], gen_T)[:, :, :T].contiguous()
    return i


def oracle_utterances(name, layout):
    """All utterances up to LARGE_ROWS rows; beyond, hip_helpers.sample_utterances' choice: the first, the last (the ragged row tile),
    the ones holding row 2048 and the fp32 switch row where the batch has them, and two seeded others."""
    B, T, _ = layout
    if B * T <= LARGE_ROWS:
        return list(range(B))
    return sample_utterances(B, T, [r for r in (ROW_SWITCH_SPLIT, ROW_SWITCH_F32 - 1) if r < B * T], k_random=2, seed=B)


def rows_of(i, rows):
    return {k: (v if v is None else v[rows]) for k, v in i.items()}


def restatement(fam, name, sd, i, layout_T, dtype=torch.float64):
    """oracle.vits2_oracle.text_encoder / flow_reverse and test_vc_host.flow_forward / posterior_encoder on a state dict (CPU) and
    inputs `i` (any subset of a layout's utterances), evaluated in `dtype` -> the case's outputs [B, C, T] by name."""
    c = FAMILIES[fam][name]
    g = None if i["g"] is None else i["g"].to(dtype)
    if fam == "te":
        d = V.Vits2Dims(n_vocab=N_VOCAB, inter_channels=c["inter"], hidden_channels=c["hidden"], filter_channels=c["filter"], n_heads=c["heads"],
                        n_layers=c["layers"], kernel_size=c["kernel"], window_size=WINDOW, gin_channels=c["gin"], cond_layer_idx=c["cond"])
        x, m, logs, _ = V.text_encoder(i["ids"], i["lengths"], {f"enc_p.{k}": v.to(dtype) for k, v in sd.items()}, d, g=g)
        return dict(x=x, m=m, logs=logs)
    mask = V.sequence_mask(i["lengths"], layout_T).unsqueeze(1).to(dtype)
    if fam == "flow":
        d = flow_dims(c["channels"], c["hidden"], c["kernel"], c["wn_layers"], c["flows"], c["gin"])
        wts = {f"flow.{k}": v.to(dtype) for k, v in sd.items() if "post_transformer" not in k}
        z = i["z"].to(dtype)
        return dict(rev=V.flow_reverse(z, mask, wts, d, g=g), fwd=flow_forward(z, mask, wts, d, g=g))
    z, m, logs, _ = posterior_encoder({k: v.to(dtype) for k, v in sd.items()}, i["y"].to(dtype), i["lengths"], g, i["eps"].to(dtype), c["layers"], c["kernel"])
    return dict(z=z, m=m, logs=logs)


def state(mod):
    return {k: v.detach().clone().cpu() for k, v in mod.state_dict().items()}


@functools.lru_cache(maxsize=None)
def drop_in_state(fam, name):
    from torch_tts_amd import vits2

    return state(make(vits2, fam, name))


@functools.lru_cache(maxsize=None)
def refs(fam, name, li):
    """-> (the layout's inputs, the sampled utterances, the fp64 restatement on them) - computed once, shared, never changed"""
    layout = LAYOUTS[name][li]
    i = inputs(fam, name, layout)
    rows = oracle_utterances(name, layout)
    with torch.no_grad():
        return i, rows, restatement(fam, name, drop_in_state(fam, name), rows_of(i, rows), layout[1])


# ---------------------------------------------------------------------------------------------------------------------------
# "the tests would notice": the state-dict keys of the probed GEMM's weight, and a state dict with part of it zeroed
# ---------------------------------------------------------------------------------------------------------------------------
PROBES = {  # tile -> (family, case, layout index, precision, gemm name, state-dict prefix of its conv)
    "split/128x128": ("te", "W48", 0, "split_f16", "w1.0", "encoder.ffn_layers.0.conv_1"),
    "f32/64x64": ("flow", "RF", 1, "f32", "0.in.0", "flows.0.enc.in_layers.0"),
    "split/lean64": ("post", "L168", 0, "split_f16", "pre", "pre"),
}


def zeroed(sd, prefix, k_from=None, n_from=None):
    """sd with the conv `prefix`'s weight zeroed for K index >= k_from (the kernel's K order: tap-major, k = tap * Cin + c) or for
    output rows >= n_from (and their bias).  A weight-normed conv keeps every other element's effective value: weight_g is
    rescaled by the row norms' ratio."""
    sd = dict(sd)
    key = prefix + (".weight_v" if prefix + ".weight_v" in sd else ".weight")
    w = sd[key].clone()  # [N, Cin, taps]
    N, Cin, taps = w.shape
    before = w.flatten(1).norm(dim=1)
    if k_from is not None:
        k = torch.arange(taps)[None, :] * Cin + torch.arange(Cin)[:, None]  # [Cin, taps]
        assert k_from < taps * Cin
        w[:, k >= k_from] = 0
    if n_from is not None:
        assert n_from < N
        w[n_from:] = 0
        b = sd[prefix + ".bias"].clone()
        b[n_from:] = 0
        sd[prefix + ".bias"] = b
    sd[key] = w
    if key.endswith("weight_v"):
        after = w.flatten(1).norm(dim=1)
        keep = after > 0
        g = sd[prefix + ".weight_g"].clone()
        g[keep] = g[keep] * (after[keep] / before[keep]).view(-1, 1, 1)
        w[~keep] = 1.0  # (a zero row has no direction: any v with gain 0 is the zero row)
        g[~keep] = 0
        sd[prefix + ".weight_g"] = g
    return sd
