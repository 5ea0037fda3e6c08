"""Host-side checks of tests/vits2_tile_cases.py (the VITS2 row GEMMs on every tile and K-walk length): the two restatements pinned to
the source text (launch_gemm_cfg's conditions and TileCfgs, gemm_generic's fallback and its 13 call sites); the census - which tile
edge, walk length, switch side and mixed chain the case table reaches, computed from gemm_list x gemm_tile, printed and asserted;
the fp64 restatements (the oracles of tests/test_vits2_tiles_hip.py) against the reference's own outputs at these dims
(tests/golden/make_golden_vits2_tiles.py) and, at each case's real shape, against their own fp32 evaluation, both within half of
the bar the kernels are held to, so that the bar judges the kernels; and that the bar would notice a K stage or a ragged column
tile that a GEMM on each large-M tile dropped.  No GPU needed."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import vits2_attention_cases as A
import vits2_tile_cases as K
from torch_tts_amd import vits2

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RTOL, ATOL = 1e-4, 1e-5  # the bar of tests/test_vits2_hip.py and tests/test_vc_hip.py against fp64
RATIO_MAX = 0.5
PRECISIONS = ("f32", "split_f16")
RUN_IDS = [K.run_id(r) for r in K.RUNS]


def _src(name):
    return open(os.path.join(ROOT, "torch-tts_amd", "csrc", name)).read()


def ratio_close(a, b):
    """a against the fp64 b as a fraction of the rtol / atol bar"""
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a.double() - b.double()).abs() / (ATOL + RTOL * b.double().abs())).max())


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements are the sources
# ---------------------------------------------------------------------------------------------------------------------------
def tile_of_cfg(text, prec):
    """(BM, BN, k per stage, stages) of a `TileCfg<WM, WN, WK, S, PREC = PREC_F32, AUXB = 0, TM = 1, TN = 1, HK = 0>` by gemm_tile.h's
    rules: BM = 32 WM TM, BN = 32 WN TN, ROWB = HK ? 64 WK : 128 WK bytes per tile row, KT = ROWB / element bytes"""
    args = re.fullmatch(r"TileCfg<(.*)>", text).group(1).replace("(PREC == PREC_BF16 ? 5 : 4)", "4").split(", ")
    args = [{"PREC": prec}.get(a, a) for a in args] + ["PREC_F32", "0", "1", "1", "0"][len(args) - 4:]
    WM, WN, WK, S = (int(a) for a in args[:4])
    TM, TN, HK = (int(a) for a in args[6:9])
    rowb = 64 * WK if HK else 128 * WK
    return 32 * WM * TM, 32 * WN * TN, rowb // (4 if args[4] == "PREC_F32" else 2), S


def test_the_restated_dispatch_is_the_sources():
    gemm, tile, v = _src("decode_kernels.hip"), _src("gemm_tile.h"), _src("vits2.hip")
    body = gemm[gemm.index("static void launch_gemm_cfg("): gemm.index("static void launch_gemm_dil(")]
    # the three condition lines (postnet_corner_cases.shared_tile, which gemm_tile builds on) and the lean tile's
    assert "const long tiles_big = (long)((a.M + 63) / 64) * ((a.N + 63) / 64);" in body
    assert "if (a.N >= 128 && a.M >= 2048) {" in body
    assert "if (PREC != PREC_F32 || (a.fixed_tile != 1 && a.M >= 64 && tiles_big >= 512)) {" in body
    assert "if constexpr (PREC == PREC_F16S && AK == A_PLAIN && EK == EPI_GENERIC) {" in body
    assert "if (lean_skinny && a.K <= 256 && a.M >= 2048) {" in body
    assert 'static const bool lean_skinny = getenv("TTSDEC_NO_LEAN_SKINNY") == nullptr;' in body
    # each branch's TileCfg, in the order of the branches (the first is the EPI_PLAIN split-K tile, not ours)
    cfgs = re.findall(r"using Cfg = (TileCfg<[^;]*>);", body)
    assert cfgs == ["TileCfg<1, 1, 2, 4, PREC_F16S>", "TileCfg<2, 2, 1, 4, PREC_F16S, 0, 1, 1, 1>", "TileCfg<2, 2, 1, 2, PREC, 0, 2, 2, 0>",
                    "TileCfg<2, 2, 1, (PREC == PREC_BF16 ? 5 : 4), PREC>", "TileCfg<1, 1, 4, 4>"]
    for rule in ("static constexpr int EB = (PREC == PREC_F32) ? 4 : 2;", "static constexpr int BM = 32 * WM * TM;", "static constexpr int BN = 32 * WN * TN;",
                 "static constexpr int ROWB = HK ? 64 * WK : 128 * WK;", "static constexpr int KT = ROWB / EB;", "static constexpr int STAGES = S;",
                 "template <int WM, int WN, int WK, int S, int PREC = PREC_F32, int AUXB = 0, int TM = 1, int TN = 1, int HK = 0>"):
        assert rule in tile, rule
    assert K.TILES == {"split/lean64": tile_of_cfg(cfgs[1], "PREC_F16S"), "split/128x128": tile_of_cfg(cfgs[2], "PREC_F16S"),
                       "split/64x64": tile_of_cfg(cfgs[3], "PREC_F16S"), "f32/64x64": tile_of_cfg(cfgs[3], "PREC_F32"),
                       "f32/32x32k4": tile_of_cfg(cfgs[4], "PREC_F32")}
    assert set(K.LARGE_TILES) == set(K.TILES) - {"split/64x64", "f32/32x32k4"}
    # gemm_generic
    assert "  const bool split = cx.split && !(K & 7);" in v and "  const int K = l.K;" in v
    assert "  if (l.taps > 1) launch_gemm<A_CONV, EPI_GENERIC>(g, st);\n  else launch_gemm<A_PLAIN, EPI_GENERIC>(g, st);" in v
    assert v.count("gemm_generic(") == 14  # 13 calls + the definition: a new call site fails here until gemm_list knows it
    assert v.count("gemm_generic(kExact, ") == 2  # cond, spk
    assert "h->spec_pad = (int)up((size_t)dims->spec_channels, 8);" in v and "L.pre = wk.lin(d.hidden_channels, spec_pad);" in v
    assert "if (e.out_pl != nullptr) set_output(g, PREC_F16S, e.out_pl, (size_t)M * l.N);" in v  # (whatever the precision: writes_planes)


def test_gemm_tile_at_its_edges():
    t = lambda *a: K.gemm_tile(*a)[0]  # noqa: E731
    assert K.gemm_tile("split_f16", True, 2107, 136, 72) == ("split/128x128", (64, 2))
    assert K.gemm_tile("f32", True, 10881, 136, 72) == ("f32/64x64", (32, 4))
    assert [t("split_f16", False, m, 72, 256) for m in (2047, 2048)] == ["split/64x64", "split/lean64"]
    assert [t("split_f16", False, 2048, n, 264) for n in (127, 128)] == ["split/64x64", "split/128x128"]  # K > 256: off the lean tile
    assert [t("split_f16", True, m, 272, 408) for m in (2047, 2048)] == ["split/64x64", "split/128x128"]
    assert [t("f32", False, m, 136, 136) for m in (10880, 10881)] == ["f32/32x32k4", "f32/64x64"]
    assert [t("f32", False, m, 40, 20) for m in (32704, 32705)] == ["f32/32x32k4", "f32/64x64"]
    assert t("split_f16", False, 2107, 144, 132) == "f32/32x32k4" and t("split_f16", True, 10881, 136, 5 * 132) == "f32/64x64"  # K & 7
    assert t("f32", False, 63, 4096, 8) == "f32/32x32k4"
    # gemm_list: the counts of the call sites per call
    n = lambda fam, name: len(K.gemm_list(fam, name, 3, 37))  # noqa: E731
    assert n("te", "W8") == 4 + 1 and n("te", "X3") == 1 + 3 * 4 + 1 and n("flow", "RF") == 2 * (2 * 4 + 1 + 2 * 2 + 1)
    assert n("post", "RQ") == 1 + 1 + 2 * 2 + 1 and n("post", "N1") == 4
    assert [K.spec_pad(s) for s in K.LEAN_SPECS.values()] == [24, 40, 72, 104, 136, 168] and K.spec_pad(8) == 8


# ---------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------
EDGES = ("N % BN", "M % BM", "K % k-stage", "mask @ partial", "resid @ partial", "planes @ partial")


def census():
    """-> {tile: {feature: [where]}} over every GEMM of every run in both precisions, {tile: set of walk lengths}, and per call
    the set of tiles"""
    feats = {t: {e: [] for e in EDGES + ("conv Cin straddles",)} for t in K.TILES}
    walks = {t: set() for t in K.TILES}
    calls = {}
    for fam, name, li in K.RUNS:
        layout = K.LAYOUTS[name][li]
        for prec in PRECISIONS:
            for g, tile, (kps, S) in K.tiles_of(fam, name, layout, prec):
                gname, conv, M, N, Kt, Cin, taps, has_mask, has_resid, planes = g
                BM, BN = K.TILES[tile][:2]
                where = f"{K.run_id((fam, name, li))}/{prec}/{gname}"
                calls.setdefault((fam, name, li, prec), []).append((gname, tile, M))
                walks[tile].add(-(-Kt // kps))
                partial = bool(N % BN or M % BM)
                for e, hit in zip(EDGES, (N % BN, M % BM, Kt % kps, has_mask and partial, has_resid and partial, planes and partial)):
                    if hit:
                        feats[tile][e].append(where)
                if conv and kps % Cin and Cin % kps:
                    feats[tile]["conv Cin straddles"].append(where)
    return feats, walks, calls


def test_census():
    feats, walks, calls = census()
    print("\ntile            " + "".join(f"{e:>20}" for e in EDGES + ("conv Cin straddles",)) + "   walk lengths (stages)")
    for t in K.TILES:
        print(f"{t:16}" + "".join(f"{len(feats[t][e]):>20}" for e in feats[t]) + f"   {sorted(walks[t])}")
    for t in K.LARGE_TILES:
        for e in EDGES:
            assert feats[t][e], (t, e)
            print(f"{t:16}{e:18} e.g. {feats[t][e][0]}")
    for t in ("f32/64x64", "split/128x128"):  # the two large tiles that convs reach (the lean tile is A_PLAIN's)
        assert feats[t]["conv Cin straddles"], t
        print(f"{t:16}{'conv Cin straddles':18} e.g. {feats[t]['conv Cin straddles'][0]}")
    assert not feats["split/lean64"]["conv Cin straddles"]
    S = {t: K.TILES[t][3] for t in K.TILES}
    for t in ("f32/64x64", "split/lean64"):
        assert walks[t] >= {1, 2, S[t] - 1, S[t], S[t] + 1}, (t, walks[t])
    assert walks["split/128x128"] >= {1, 2, 3} and S["split/128x128"] == 2  # S - 1, S, S + 1
    # mixed chains: a split-fp16 call in which a layer fell back to exact fp32 (K & 7) beside split layers
    mixed = {}
    for (fam, name, li, prec), gs in calls.items():
        body = [(g, t) for g, t, M in gs if not K.always_exact(g)]
        if prec == "split_f16" and {t.split("/")[0] for _, t in body} == {"f32", "split"}:
            mixed[(name, li)] = {t for _, t in body}
    print("mixed chains:", {K.run_id(("", n, li)): sorted(t) for (n, li), t in mixed.items()})
    for small in ("split/64x64", "f32/32x32k4"):
        assert any(small in ts and ts & set(K.LARGE_TILES) for ts in mixed.values()), small
    assert any({"f32/64x64", "split/128x128"} <= ts for ts in mixed.values())  # an exact layer on a LARGE tile feeds planes to a split one
    x2 = dict((g, t) for g, t, _ in calls[("te", "X2", 1, "split_f16")])
    assert (x2["w1.0"], x2["w2.0"], x2["w1.1"]) == ("f32/64x64", "split/128x128", "f32/64x64")
    x2 = dict((g, t) for g, t, _ in calls[("te", "X2", 0, "split_f16")])
    assert (x2["w1.0"], x2["w2.0"], x2["w1.1"]) == ("f32/32x32k4", "split/128x128", "f32/32x32k4")
    # the switches: the same module on both sides
    sw = {(li, prec): dict((g, t) for g, t, _ in calls[("post", K.SWITCH_CASE, li, prec)]) for li in range(4) for prec in PRECISIONS}
    assert [K.LAYOUTS[K.SWITCH_CASE][li][:2] for li in range(4)] == [(1, 2047), (1, 2048), (1, 10880), (1, 10881)]
    assert set(sw[(0, "split_f16")].values()) == {"split/64x64"}
    assert (sw[(1, "split_f16")]["in.0"], sw[(1, "split_f16")]["pre"], sw[(1, "split_f16")]["rs.0"]) == ("split/128x128", "split/lean64", "split/lean64")
    for g in ("pre", "rs.0", "proj"):  # N = 136
        assert (sw[(2, "f32")][g], sw[(3, "f32")][g]) == ("f32/32x32k4", "f32/64x64"), g
    print("switches:", {f"{K.LAYOUTS[K.SWITCH_CASE][li][1]}/{prec}": sorted(set(v.values())) for (li, prec), v in sw.items()})
    # every utterance boundary lies strictly inside a row tile of every tile its call runs on
    for (fam, name, li, prec), gs in calls.items():
        B, T, lengths = K.LAYOUTS[name][li]
        assert (B == 1 or T % 64) and len(lengths) == B and max(lengths) <= T  # (one utterance: no boundary)
        for g, t, M in gs:
            if M == B * T:
                assert all((b * T) % K.TILES[t][0] for b in range(1, B)), (name, li, g, t)
    for name, layouts in K.LAYOUTS.items():  # lengths: T, 1 and a value in between (the switches: one utterance)
        for B, T, lengths in layouts:
            assert B == 1 or ({T, 1} <= set(lengths) and any(1 < n < T for n in lengths) and lengths[-1] == T), (name, B, T)


def test_the_walk_series_walk_what_the_table_says():
    w1 = lambda n, li, prec: [x for x in K.tiles_of("te", n, K.LAYOUTS[n][li], prec) if x[0][0] == "w1.0"][0]  # noqa: E731
    names = ["W8", "W16", "W24", "W40", "W48"]
    assert [w1(n, 0, "split_f16")[0][4] for n in names] == [24, 48, 72, 120, 144]
    assert [(w1(n, 0, "split_f16")[1], -(-w1(n, 0, "split_f16")[0][4] // 64)) for n in names] == list(zip(["split/128x128"] * 5, [1, 1, 2, 2, 3]))
    assert [(w1(n, 1, "f32")[1], -(-w1(n, 1, "f32")[0][4] // 32)) for n in names] == list(zip(["f32/64x64"] * 5, [1, 2, 3, 4, 5]))
    for n in names:  # wqkv and wo on the lean tile, w2 (N < 128) on the split 64 x 64 tile
        t = dict((g[0], tile) for g, tile, _ in K.tiles_of("te", n, K.LAYOUTS[n][0], "split_f16"))
        assert (t["wqkv.0"], t["wo.0"], t["w2.0"], t["proj"]) == ("split/lean64", "split/lean64", "split/64x64", "split/lean64")
    pre = [K.tiles_of("post", n, K.LAYOUTS[n][0], "split_f16")[0] for n in K.LEAN_SPECS]
    assert [(g[0], t, -(-g[4] // kps), g[4] % kps != 0) for g, t, (kps, S) in pre] == [("pre", "split/lean64", nk, True) for nk in (1, 2, 3, 4, 5, 6)]
    assert K.L2107[0] * K.L2107[1] == 2107 and K.L10881[0] * K.L10881[1] == 10881 == 170 * 64 + 1 and K.L32705[0] * K.L32705[1] == 32705 == 511 * 64 + 1
    n1 = K.tiles_of("post", "N1", K.L32705, "f32")
    assert [(g[3], t) for g, t, _ in n1] == [(20, "f32/64x64"), (40, "f32/64x64"), (20, "f32/64x64"), (24, "f32/64x64")]
    # the sequence lengths stay inside what the attention kernels take at these head widths (a ValueError otherwise)
    for fam, name, li in K.RUNS:
        c, (B, T, _) = K.FAMILIES[fam][name], K.LAYOUTS[name][li]
        if fam == "te":
            A.mha_choice(T, c["hidden"] // c["heads"], K.WINDOW, "split_f16", c["hidden"])
        elif fam == "flow":
            A.mha_choice(T, c["channels"] // 4, None, "split_f16", c["channels"] // 2)


def test_the_sample_holds_the_rows_that_matter():
    for fam, name, li in K.RUNS:
        B, T, _ = K.LAYOUTS[name][li]
        rows = K.oracle_utterances(name, K.LAYOUTS[name][li])
        if B * T <= K.LARGE_ROWS:
            assert rows == list(range(B))
            continue
        assert len(rows) == len(set(rows)) <= 6 and rows[0] == 0 and rows[-1] == B - 1
        assert K.ROW_SWITCH_SPLIT // T in rows and (B * T < K.ROW_SWITCH_F32 or (K.ROW_SWITCH_F32 - 1) // T in rows)
        assert len(rows) >= min(B, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements are the reference at these dims
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_golden():
    z = np.load(os.path.join(HERE, "golden", "vits2_tiles.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "vits2_tiles_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def test_tables_are_the_recorded_ones():
    g, meta = load_golden()
    assert (meta["ratio_max"], meta["stride"], tuple(meta["layout"][:2]), tuple(meta["layout"][2])) == (RATIO_MAX, K.STRIDE, K.SMALL[:2], K.SMALL[2])
    for fam, table in K.FAMILIES.items():
        assert {n: {k: c[k] for k in table[n]} for n, c in meta[fam].items()} == table, fam
    assert len({c["seed"] for t in K.FAMILIES.values() for c in t.values()}) == len(K.CASES)
    assert os.path.getsize(os.path.join(HERE, "golden", "vits2_tiles.npz")) <= os.path.getsize(os.path.join(HERE, "golden", "vits2_dims_corners.npz"))


@pytest.mark.parametrize("fam,name", K.CASES, ids=[n for _, n in K.CASES])
def test_restatement_matches_the_reference(fam, name):
    """The fp64 restatement on the drop-in's seeded state dict against the reference's fp32 outputs at the small layout: within half
    of the bar, and no further than the golden script measured over every element (the file keeps each thirteenth)."""
    g, meta = load_golden()
    rec = meta[fam][name]
    assert len(K.make(vits2, fam, name).state_dict()) == rec["n_tensors"]
    with torch.no_grad():
        ref = K.restatement(fam, name, K.drop_in_state(fam, name), K.inputs(fam, name, K.SMALL), K.SMALL[1])
    assert rec["ratio"] == max(rec["ratios"].values()) <= RATIO_MAX
    for k in K.OUTPUTS[fam]:
        got, want = g[f"{fam}/{name}/{k}"], ref[k].reshape(-1)[::K.STRIDE]
        assert list(ref[k].shape) == rec["shapes"][k] and got.shape == want.shape and got.dtype == torch.float32, (name, k)
        r = ratio_close(got, want)
        print(f"{name} {k}: the reference's fp32 at {r:.3f} of the bar from the fp64 restatement")
        assert r <= RATIO_MAX and r <= rec["ratios"][k] * (1 + 1e-3) + 1e-6, (name, k, r)
        assert 0.2 < rec["abs_max"][k] < 16.0 and bool(got.abs().max() > 0.2), (name, k)  # (neither faded nor blown up)
        for b, n in enumerate(K.SMALL[2]):
            assert float(ref[k][b, :, n:].abs().sum()) == 0.0 and bool((ref[k][b, :, :n] != 0).any()), (name, k, b)


# ---------------------------------------------------------------------------------------------------------------------------
# the bar judges the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", K.RUNS, ids=RUN_IDS)
def test_margin(run):
    """A condition on the inputs, not a measurement: at the case's real shape, on the sampled utterances, the restatement evaluated
    in fp32 stays within half of the bar from its fp64 evaluation."""
    fam, name, li = run
    i, rows, ref = K.refs(fam, name, li)
    with torch.no_grad():
        f32 = K.restatement(fam, name, K.drop_in_state(fam, name), K.rows_of(i, rows), K.LAYOUTS[name][li][1], torch.float32)
    ratios = {k: ratio_close(f32[k], ref[k]) for k in K.OUTPUTS[fam]}
    print(f"{K.run_id(run)} ({len(rows)} utterances): fp32 restatement at " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + " of the bar;"
          + " largest |.| " + ", ".join(f"{k} {float(ref[k].abs().max()):.2f}" for k in K.OUTPUTS[fam]))
    assert all(f32[k].dtype == torch.float32 and ref[k].dtype == torch.float64 for k in ratios)
    assert max(ratios.values()) <= RATIO_MAX, ratios


# ---------------------------------------------------------------------------------------------------------------------------
# the tests would notice
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(K.PROBES))
def test_a_dropped_k_stage_or_column_tile_is_far_outside_the_bar(tile):
    """One GEMM on each large-M tile: with the weight columns of its last K stage zeroed in the state dict, and separately the
    weight rows and bias of its last, ragged column tile, some output element of the sampled utterances moves by more than 10 x
    the bar - a case that fails this is too forgiving to judge that GEMM."""
    fam, name, li, prec, gname, prefix = K.PROBES[tile]
    (g, got_tile, (kps, S)), = [x for x in K.tiles_of(fam, name, K.LAYOUTS[name][li], prec) if x[0][0] == gname]
    assert got_tile == tile
    _, _, M, N, Kt, Cin, taps, _, _, _ = g
    BN = K.TILES[tile][1]
    k_from, n_from = (-(-Kt // kps) - 1) * kps, N // BN * BN
    assert 0 < k_from < Kt and 0 < n_from < N
    i, rows, ref = K.refs(fam, name, li)
    sd = K.drop_in_state(fam, name)
    w = sd[prefix + (".weight_v" if prefix + ".weight_v" in sd else ".weight")]
    assert w.shape[0] == N and w.shape[2] == taps and Kt - 8 < w.shape[1] * w.shape[2] <= Kt  # (`pre`: K is the spec padded to 8)
    assert k_from < w.shape[1] * w.shape[2]  # (the stage holds real columns, not only `pre`'s zero padding)
    for what, kw in (("last K stage", dict(k_from=k_from)), ("last column tile", dict(n_from=n_from))):
        with torch.no_grad():
            moved = K.restatement(fam, name, K.zeroed(sd, prefix, **kw), K.rows_of(i, rows), K.LAYOUTS[name][li][1])
        d = max(ratio_close(moved[k], ref[k]) for k in K.OUTPUTS[fam])
        print(f"{tile} {K.run_id((fam, name, li))} {gname}: zeroing its {what} (k >= {k_from} of {Kt} | n >= {n_from} of {N}) moves an output by {d:.0f} x the bar")
        assert d > 10.0, (tile, what, d)


def test_zeroed_keeps_the_rest_of_a_weight_normed_conv():
    sd = K.drop_in_state("flow", "RF")
    p = "flows.0.enc.in_layers.0"
    eff = lambda s: torch._weight_norm(s[p + ".weight_v"], s[p + ".weight_g"], 0)  # noqa: E731
    a, b, c = eff(sd), eff(K.zeroed(sd, p, k_from=352)), eff(K.zeroed(sd, p, n_from=128))
    kk = torch.arange(5)[None, :] * 72 + torch.arange(72)[:, None]
    assert bool((b[:, kk >= 352] == 0).all()) and torch.allclose(b[:, kk < 352], a[:, kk < 352], rtol=1e-6, atol=0) and int((kk >= 352).sum()) == 8
    assert bool((c[128:] == 0).all()) and torch.equal(c[:128], a[:128])


# ---------------------------------------------------------------------------------------------------------------------------
# create accepts every case
# ---------------------------------------------------------------------------------------------------------------------------
def test_create_accepts_every_case():
    for fam, name in K.CASES:
        mod = K.make(vits2, fam, name)
        eng = vits2.PostEngine(mod._cfg, None) if fam == "post" else vits2.VitsEngine(mod._dims(), None)
        try:
            assert eng.num_weight_tensors() == len(mod.weight_tensors()), name
            for B, T, _ in K.LAYOUTS[name]:
                for prec in PRECISIONS:
                    eng.set_precision(prec)
                    fn = (eng._lib.ttspost_workspace_bytes if fam == "post" else eng._lib.ttsvits_text_encoder_workspace_bytes if fam == "te"
                          else eng._lib.ttsvits_flow_workspace_bytes)
                    assert int(fn(eng._h, B, T)) > 0, (name, B, T)
        finally:
            eng.close()
