"""Host-side checks of the dims corners of tests/postnet_corner_cases.py (MelPostnet, MelPostnet2, Encoder2): the fp64 oracle -
oracle/tacotron_oracle.py on .double() weights and inputs, the reference of tests/test_postnet_corners_hip.py - against the
reference's own outputs at these dims (tests/golden/make_golden_postnet_corners.py) under the project's bar, rtol 1e-4 / atol 1e-5;
that the fp32 oracle lies within half of that bar at every case and shape, so the bar judges the kernels and not the case; that the
case table reaches the kernels, schedules, tiles and fallbacks its comments claim (by restatement, pinned to the source text);
that hip_helpers.postnet_bf16_emulation with the padding taken from the weights is what it was at 5 taps, and that a conv which
leaks one tap across an utterance's edge is far outside the bf16 bar; and that the modules' out-of-range dims are refused at create.
No GPU needed."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import hip_helpers as H
import postnet_corner_cases as K
import torch_tts_amd as T
from oracle import tacotron_oracle as O
from torch_tts_amd import _lib
from torch_tts_amd.encoder import EncoderEngine

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RTOL, ATOL = 1e-4, 1e-5
RATIO_MAX = 0.5
BF16_BAR = 8e-3  # test_hip_parity.test_postnet_bf16_vs_its_own_rounding_emulated_on_the_cpu's
CUS = 256        # an MI355X's; the schedules restated here are those of that device
FORCED = ("M1", "M2", "M3", "M4")  # the cases whose layers conv256 takes when forced


@functools.lru_cache(maxsize=None)
def load_golden():
    z = np.load(os.path.join(HERE, "golden", "postnet_corners.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "postnet_corners_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def ratio_close(a, b):
    """a against the fp64 b as a fraction of the rtol / atol bar (make_golden_postnet_corners.ratio_close)."""
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a.double() - b.double()).abs() / (ATOL + RTOL * b.double().abs())).max())


@functools.lru_cache(maxsize=None)
def case_weights(name):
    return K.weights(name)


@functools.lru_cache(maxsize=None)
def postnet_ref(name, B, T, cus=CUS):
    """-> (x [B, T, d] fp32, the utterances the oracle ran, its fp64 result on them) - computed once, shared, never changed"""
    x = K.postnet_input(name, B, T)
    rows = K.oracle_utterances(name, B, T, cus)
    return x, rows, K.postnet_oracle(name, x[rows], case_weights(name), torch.float64)


@functools.lru_cache(maxsize=None)
def encoder_ref(name, i):
    ids, lengths = K.encoder_input(name, i)
    return ids, lengths, K.encoder_oracle(name, ids, lengths, case_weights(name), torch.float64)


def _same_ratio(got, recorded, what):
    """The ratio the golden script measured is the one this machine measures (both are fp32-vs-fp64 differences), and it is
    within half of the bar."""
    assert recorded <= RATIO_MAX, (what, recorded)
    assert got == pytest.approx(recorded, rel=1e-3, abs=1e-6), (what, got, recorded)


def test_tables_are_the_recorded_ones():
    g, meta = load_golden()
    assert meta["ratio_max"] == RATIO_MAX and meta["max_elements"] == K.GOLDEN_MAX_ELEMENTS
    names = list(K.MEL_CASES) + list(K.MEL2_CASES) + list(K.ENC_CASES)
    assert meta["dims"] == {n: list(K.case(n)["dims"]) for n in names} and meta["seeds"] == {n: K.case(n)["seed"] for n in names}
    assert len({K.case(n)["seed"] for n in names}) == len(names)
    want = [f"{n}/B{B}T{T}" for n, B, T in K.postnet_shapes(golden_only=True)]
    assert list(meta["post"]) == want and list(meta["enc"]) == [f"{n}/{i}" for n in K.ENC_CASES for i in range(len(K.ENC_SHAPES))]
    # every shape but the large ones is recorded (by the element count: M10 (7, 301) holds as many elements as Q5 (7, 301))
    left_out = [s for s in K.postnet_shapes() if s not in K.postnet_shapes(golden_only=True)]
    assert left_out == [("M2", 128, 600), ("M3", 40, 600), ("M10", 7, 301), ("M10", 19, 577), ("Q5", 7, 301)]
    for n, B, T_ in K.postnet_shapes(golden_only=True):  # the inputs are the table's recipe on this machine too
        assert torch.equal(K.postnet_input(n, B, T_).reshape(-1)[:: meta["stride"]], g[f"post/{n}/B{B}T{T_}/x13"]), (n, B, T_)
    for n in K.ENC_CASES:
        for i, (B, L, lengths) in enumerate(K.ENC_SHAPES):
            ids, lens = K.encoder_input(n, i)
            assert torch.equal(ids, g[f"enc/{n}/{i}/ids"]) and torch.equal(lens, g[f"enc/{n}/{i}/lengths"]) and lens.tolist() == lengths
            assert ids.shape == (B, L) and int(ids.max()) < K.case(n)["dims"][0]
            assert all(bool((ids[b, :m] > 0).all()) and not bool(ids[b, m:].any()) for b, m in enumerate(lengths))


@pytest.mark.parametrize("name,B,T_", K.postnet_shapes(golden_only=True))
def test_fp64_oracle_matches_the_reference_postnets(name, B, T_):
    g, meta = load_golden()
    key = f"{name}/B{B}T{T_}"
    x, rows, ref = postnet_ref(name, B, T_)
    got = g[f"post/{key}/y"]
    assert rows == list(range(B)) and ref.dtype == torch.float64 and list(got.shape) == meta["post"][key]["shape"] == [B, T_, K.case(name)["dims"][0]]
    r = ratio_close(got, ref)
    print(f"{key}: the reference's fp32 at {r:.3f} of the bar from the fp64 oracle")
    assert r <= 1.0, (key, r)
    _same_ratio(r, meta["post"][key]["ratio"], key)
    assert meta["post"][key]["y_minus_x_rms"] > 0.05  # (the Postnet does something at these weights)


@pytest.mark.parametrize("name", list(K.ENC_CASES))
def test_fp64_oracle_matches_the_reference_encoder(name):
    g, meta = load_golden()
    for i, (B, L, lengths) in enumerate(K.ENC_SHAPES):
        ids, lens, ref = encoder_ref(name, i)
        got = g[f"enc/{name}/{i}/memory"]
        assert ref.dtype == torch.float64 and list(got.shape) == meta["enc"][f"{name}/{i}"]["shape"] == [B, max(lengths), K.case(name)["dims"][2]]
        r = ratio_close(got, ref)
        print(f"{name}/{i}: the reference's fp32 at {r:.3f} of the bar from the fp64 oracle")
        assert r <= 1.0, (name, i, r)
        _same_ratio(r, meta["enc"][f"{name}/{i}"]["ratio"], f"{name}/{i}")
        for b, n in enumerate(lengths):
            assert not bool(got[b, n:].any()) and not bool(ref[b, n:].any()) and float(ref[b, :n].abs().min()) > 0


def test_encoder_oracle_keeps_the_weights_dtype():
    """O.encoder2's output buffer follows the weights: an fp64 run is not rounded to fp32 at the end, an fp32 run is what it was."""
    ids, lens, ref = encoder_ref("E3", 0)
    f32 = K.encoder_oracle("E3", ids, lens, case_weights("E3"))
    assert f32.dtype == torch.float32 and ref.dtype == torch.float64
    assert not torch.equal(ref, ref.float().double()), "the fp64 result holds fp32 values only"
    assert 0 < ratio_close(f32, ref) <= RATIO_MAX


@pytest.mark.parametrize("name,B,T_", K.postnet_shapes())
def test_margin_postnets(name, B, T_):
    """A condition on the inputs, not a measurement: the fp32 oracle within half of the bar from the fp64 oracle (at the three
    large shapes on the utterances the GPU test compares)."""
    x, rows, ref = postnet_ref(name, B, T_)
    r = ratio_close(K.postnet_oracle(name, x[rows], case_weights(name)), ref)
    print(f"{name} ({B}, {T_}): fp32 oracle at {r:.3f} of the bar")
    assert r <= RATIO_MAX, (name, B, T_, r)


@pytest.mark.parametrize("name", list(K.ENC_CASES))
def test_margin_encoder(name):
    for i in range(len(K.ENC_SHAPES)):
        ids, lens, ref = encoder_ref(name, i)
        r = ratio_close(K.encoder_oracle(name, ids, lens, case_weights(name)), ref)
        print(f"{name}/{i}: fp32 oracle at {r:.3f} of the bar")
        assert r <= RATIO_MAX, (name, i, r)


# ---------------------------------------------------------------------------------------------------------------------------
# the table reaches what its comments claim
# ---------------------------------------------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(ROOT, "torch-tts_amd", "csrc", name)).read()


def test_the_restated_predicates_are_the_sources():
    api, enc, gemm, c256 = _src("api.hip"), _src("encoder.hip"), _src("decode_kernels.hip"), _src("conv256.hip")
    assert "if (!((d.d_mel | d.postnet_hidden) & 7)) {" in api                                # K.stays_fp32, the Postnets
    assert "const bool split = h->precision == TTSDEC_PREC_SPLIT_F16 && !(E & 7);" in enc     # K.stays_fp32, Encoder2
    assert "constexpr int kMaxPostnetLayers = 8;" in api
    assert "if (d.postnet_kernel < 1 || !(d.postnet_kernel & 1)) return TTSDEC_ERR_DIMS;" in api
    assert "if (d.postnet_hidden <= 0 || (d.postnet_hidden & 3)) return TTSDEC_ERR_DIMS;" in api
    assert "(d.d_emb & 3) || d.d_out <= 0 || (d.d_out & 7)) return TTSDEC_ERR_DIMS;" in enc
    body = gemm[gemm.index("static void launch_gemm_cfg("): gemm.index("static void launch_gemm_dil(")]  # K.shared_tile
    assert "const long tiles_big = (long)((a.M + 63) / 64) * ((a.N + 63) / 64);" in body
    assert "if (a.N >= 128 && a.M >= 2048) {" in body
    assert "if (PREC != PREC_F32 || (a.fixed_tile != 1 && a.M >= 64 && tiles_big >= 512)) {" in body
    assert "|| !(taps & 1) || taps > 15) return false;" in c256                                 # H.conv256_schedule quotes the rest
    # conv256 is tried for exact fp32 and bf16 only: split-fp16 stays on the shared tile at every dims
    assert api.count("launch_conv256_") == 2 and "prec == PREC_F32 &&\n        launch_conv256_f32(" in api and "prec == PREC_BF16 && launch_conv256_bf16(" in api


def _schedules(name, B, T_, elem_bytes, force=True):
    return [H.conv256_schedule(B * T_, CUS, Cin=cin, N=n, taps=taps, elem_bytes=elem_bytes, force=force) for cin, n, taps in K.conv_layers(name)]


def test_conv256_takes_what_the_table_says():
    for name in FORCED:
        for B, T_ in K.MEL_CASES[name]["shapes"]:
            for eb in (4, 2):
                s = _schedules(name, B, T_, eb)
                assert all(x is not None for x in s[1:]), (name, B, T_, eb)  # the hidden -> hidden layers
                # layer 0: M2's only (d_mel = 128: whole 128-byte row pieces in fp32 and in bf16); 80 mel channels never
                assert (s[0] is not None) == (name == "M2"), (name, eb)
    # forced at the small shapes only: unforced the library keeps the shared tile there, and takes conv256 at the large ones
    for name in FORCED:
        for B, T_ in K.MEL_CASES[name]["shapes"]:
            unforced = _schedules(name, B, T_, 4, force=False)[1]
            assert (unforced is not None) == (B * T_ > K.LARGE_ROWS), (name, B, T_)
    for shape in (("M2", 128, 600), ("M3", 40, 600)):
        for eb in (4, 2):
            for s in _schedules(*shape, eb, force=False)[1:]:
                assert s["full"] > 0 and s["n_short"] > 0 and 0 < s["full"] * 256 < shape[1] * shape[2], (shape, s)  # whole tiles, then short ones
        rows = K.oracle_utterances(*shape)
        assert len(rows) == 5 and rows[0] == 0 and rows[-1] == shape[1] - 1
        assert _schedules(*shape, 4, force=False)[1]["full"] * 256 // shape[2] in rows
    assert _schedules("M2", 128, 600, 4, force=False)[0]["full"] == 256 and _schedules("M3", 40, 600, 4, force=False)[1]["full"] == 85
    for B, T_ in K.MEL_CASES["M5"]["shapes"]:  # 17 taps: refused, forced or not, in both element sizes
        assert all(s is None for eb in (4, 2) for s in _schedules("M5", B, T_, eb)), (B, T_)
    assert K.MEL_CASES["M3"]["dims"][1] // 256 == 3 and K.MEL_CASES["M2"]["dims"][1] // 256 == 1  # column tiles
    assert [K.taps_of(n) for n in FORCED + ("M5",)] == [1, 3, 7, 15, 17]
    # M4's and M5's short utterances: every row's window is clipped on both sides (T < taps / 2)
    assert all(T_ < K.taps_of("M4") // 2 for _, T_ in K.MEL_CASES["M4"]["shapes"][:2]) and K.MEL_CASES["M5"]["shapes"][1][1] < 17 // 2


def test_fallbacks_and_tiles_are_what_the_table_says():
    assert [n for n in list(K.MEL_CASES) + list(K.MEL2_CASES) if K.stays_fp32(n)] == ["M6", "M7", "M8", "Q1", "Q2"]
    assert [n for n in K.ENC_CASES if K.stays_fp32(n)] == ["E1", "E2", "E3"]
    assert not K.stays_fp32("M9") and not K.stays_fp32("Q3") and not K.stays_fp32("M10")
    d = K.MEL_CASES["M7"]["dims"]
    assert d[0] % 8 == 4 and d[0] % 32 and d[1] % 32 and d[3] == 8 and K.MEL_CASES["M6"]["dims"][1] % 8 == 4
    # M10, hidden 136: one full 128-column tile plus 8 columns, or two full 64-column tiles plus 8
    N = K.MEL_CASES["M10"]["dims"][1]
    assert N == 128 + 8 == 2 * 64 + 8
    assert K.shared_tile("bf16", 7 * 301, N) == K.shared_tile("split_f16", 7 * 301, N) == "128x128" and K.shared_tile("f32", 7 * 301, N) == "32x32"
    assert K.shared_tile("f32", 19 * 577, N) == "64x64" and ((19 * 577 + 63) // 64, (N + 63) // 64) == (172, 3)
    assert K.shared_tile("f32", 19 * 577, 80) == "32x32"  # (the fc layer, 172 x 2 tiles)
    assert K.shared_tile("split_f16", 7 * 301, K.MEL2_CASES["Q5"]["dims"][1]) == "128x128"
    # one utterance of 301 frames alone stays on the fp32 tile of the batch of 7; in the 16-bit modes it does not
    assert K.shared_tile("f32", 301, N) == K.shared_tile("f32", 7 * 301, N) and K.shared_tile("bf16", 301, N) != K.shared_tile("bf16", 7 * 301, N)


def test_ragged_lengths_hold_the_edges():
    assert list(K.RAGGED_SHAPES) == ["M4", "M5", "M7", "M10", "Q2", "Q3"] and K.RAGGED_SHAPES["M10"] == (7, 301)
    for name, (B, T_) in K.RAGGED_SHAPES.items():
        x, lengths = K.ragged_input(name)
        half = K.taps_of(name) // 2
        assert len(lengths) == B and {T_, 0, 1, max(half - 1, 0)} <= set(lengths) and any(half < n < T_ for n in lengths), (name, lengths)
        assert all(bool((x[b, n:] == 1e3).all()) and bool((x[b, :n].abs() < 10).all()) for b, n in enumerate(lengths))
        # the batch and each utterance alone stay on one fp32 tile; in the 16-bit modes only M10's batch changes it (128 x 128)
        N = K.case(name)["dims"][1]
        assert K.shared_tile("f32", B * T_, N) == K.shared_tile("f32", 1, N) == "32x32"
        assert (K.shared_tile("bf16", B * T_, N) != K.shared_tile("bf16", T_, N)) == (name == "M10")


def test_create_accepts_every_case():
    """ttsdec_create / ttsenc_create return OK at every case's dims (a Handle raises otherwise); the tensor counts are the
    modules'; the workspaces are positive."""
    for name, table in [(n, t) for t in (K.MEL_CASES, K.MEL2_CASES) for n in t]:
        m = K.make_module(T, name)
        eng = T.Engine(m.engine_dims(), None)
        try:
            assert eng.num_weight_tensors() == len(m.weight_tensors()), name
            for B, T_ in table[name]["shapes"]:
                assert eng.postnet_workspace_bytes(B, T_) > 0
        finally:
            eng.close()
    for name in K.ENC_CASES:
        alphabet, d_emb, d_out = K.case(name)["dims"]
        m = K.make_module(T, name)
        eng = EncoderEngine(dict(alphabet_size=alphabet, d_emb=d_emb, d_out=d_out, conv_kernel=5, bn_eps=1e-5), None)
        try:
            assert eng.num_weight_tensors() == len(m.weight_tensors()), name
            for B, L, _ in K.ENC_SHAPES:
                assert int(eng._lib.ttsenc_workspace_bytes(eng._h, B, L)) > 0
        finally:
            eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the bf16 emulation
# ---------------------------------------------------------------------------------------------------------------------------
def _emulation_at_five_taps(y, pw, num_layers):
    """hip_helpers.postnet_bf16_emulation as it stood while it hard-coded padding=2."""
    def rb(x):
        return x.to(torch.bfloat16).to(torch.float32)

    xc = rb(y).transpose(1, 2)
    for i in range(num_layers):
        xc = torch.nn.functional.conv1d(xc, rb(pw[f"conv.{i}.0.weight"]), None, padding=2)
        inv = 1.0 / torch.sqrt(pw[f"conv.{i}.1.running_var"] + 1e-5)
        alpha = pw[f"conv.{i}.1.weight"] * inv
        beta = pw[f"conv.{i}.1.bias"] - pw[f"conv.{i}.1.running_mean"] * alpha
        xc = rb(O.isru(xc * alpha[None, :, None] + beta[None, :, None]))
    return y + torch.nn.functional.linear(xc.transpose(1, 2), rb(pw["fc_out.weight"]))


def test_bf16_emulation_is_unchanged_at_five_taps():
    for d_mel, hidden, layers, shape, seed in ((80, 512, 3, (5, 131), 9), (80, 64, 3, (3, 5), 9), (8, 8, 3, (3, 37), 109)):
        pw = O.random_postnet_weights(d_mel, hidden, layers, seed=seed)
        y = torch.randn(*shape, d_mel, generator=torch.Generator().manual_seed(2))
        got = H.postnet_bf16_emulation(y, pw, layers)
        assert got.dtype == torch.float32 and torch.equal(got, _emulation_at_five_taps(y, pw, layers)), (d_mel, hidden)


BF16_CASES = [n for n in K.MEL_CASES if not K.stays_fp32(n)]  # the MelPostnet cases whose bf16 request takes the planes


def test_bf16_cases_are_the_tables():
    assert BF16_CASES == ["M1", "M2", "M3", "M4", "M5", "M9", "M10"]


@pytest.mark.parametrize("name", [n for n in BF16_CASES if K.taps_of(n) > 1])
def test_a_tap_leaked_across_an_utterance_edge_is_far_outside_the_bf16_bar(name):
    """The deliberately wrong emulation (postnet_bf16_emulation(leak=True): the last frame of every utterance also gets one tap
    from the frame that follows it in the flattened batch) differs from the right one by at least 10 x the bf16 bar, at every
    shape: the bar of the GPU tests cannot hide such a leak in bf16's own error."""
    pw, layers = case_weights(name), K.layers_of(name)
    for B, T_ in K.MEL_CASES[name]["shapes"]:
        x, rows, _ = postnet_ref(name, B, T_)
        good = H.postnet_bf16_emulation(x[rows], pw, layers)
        d = (H.postnet_bf16_emulation(x[rows], pw, layers, leak=True) - good)
        print(f"{name} ({B}, {T_}): leaked tap moves the result by {float(d.abs().max()):.3f} (bar {BF16_BAR})")
        assert float(d.abs().max()) >= 10 * BF16_BAR, (name, B, T_)
        if T_ > 2 * K.taps_of(name):  # ... and it is the LAST frames that move: the first ones are out of its reach
            assert not bool(d[:, 0].any()) and bool(d[:, -1].any())


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _refused(make_dims, cls=None):
    """Building the handle for a module's dims raises ERR_DIMS (the engine-dims path of tests/test_host_logic.py: the module's own
    engine_dims() through the engine class, host only) - no handle exists afterwards that could misbehave later."""
    with pytest.raises(NotImplementedError) as ei:
        (cls or T.Engine)(make_dims(), None)
    assert isinstance(ei.value, _lib.TtsdecError) and ei.value.code == _lib.ERR_DIMS


def test_modules_with_dims_outside_the_librarys_are_refused():
    _refused(lambda: T.MelPostnet(80, dim_hidden=512, kernel_size=4, num_layers=3).engine_dims())   # an even kernel
    _refused(lambda: T.MelPostnet(80, dim_hidden=6, kernel_size=5, num_layers=3).engine_dims())     # hidden % 4
    _refused(lambda: T.MelPostnet(80, dim_hidden=512, kernel_size=5, num_layers=9).engine_dims())   # more than kMaxPostnetLayers
    _refused(lambda: T.MelPostnet2(80, dim_hidden=6, num_layers=3).engine_dims())
    _refused(lambda: T.MelPostnet2(80, dim_hidden=128, num_layers=9).engine_dims())
    # no layer at all: the module has no BatchNorm to read its eps from and says so before any handle is made; the dims themselves
    # (postnet_layers = 0) are a decoder-only handle, whose ttsdec_postnet answers ERR_DIMS (test_host_logic.py)
    for make in (lambda: T.MelPostnet(80, dim_hidden=512, kernel_size=5, num_layers=0), lambda: T.MelPostnet2(80, dim_hidden=128, num_layers=0)):
        with pytest.raises(IndexError):
            make().engine_dims()
    e = T.Engine(T.EngineDims(postnet_layers=0), None)
    try:
        assert e.postnet_workspace_bytes(2, 9) == 0
        assert _lib.load().ttsdec_postnet(e._h, 256, 1, 1, 0, 256, 256, 0, None) == _lib.ERR_DIMS
    finally:
        e.close()

    def enc_dims(**kw):
        m = T.Encoder2(40, **kw)
        return dict(alphabet_size=m.emb.num_embeddings, d_emb=m.dim_emb, d_out=m.dim_out, conv_kernel=5, bn_eps=float(m.conv[1].eps))

    _refused(lambda: enc_dims(dim_emb=6, dim_out=64), EncoderEngine)
    _refused(lambda: enc_dims(dim_emb=32, dim_out=12), EncoderEngine)
