"""GPU parity at the corners of the dims that ttsdec_create accepts for MelPostnet / MelPostnet2 and ttsenc_create for Encoder2
(tests/postnet_corner_cases.py): every case and shape through the drop-in modules against the fp64 oracle on the CPU (the same
fp32 weights and inputs in .double(); tests/test_postnet_corners_host.py shows that it is the reference at these dims and that the
fp32 oracle is within half of the bar), under the project's bar rtol 1e-4 / atol 1e-5 in exact fp32 and split-fp16; the 16-bit
requests that must stay on exact fp32, bit for bit; conv256 forced at its untested instantiations; bf16 against the CPU
emulation of its own roundings; ragged batches; rows alone and twice; the carved workspaces.

MEASURED on an MI355X (256 CUs), from this module's printout.  Worst |err| / (atol + rtol |ref|) against the fp64 oracle:

  case (B, T)        f32    split_f16 | case (B, T)        f32    split_f16 | case (B, T)       f32    split_f16
  M1  (3, 57)        0.110  0.096     | M5  (2, 40)        0.247  0.106     | Q1 (2, 9)         0.004  0.004
  M2  (3, 131)       0.110  0.076     | M5  (3, 7)         0.068  0.056     | Q1 (2, 1)         0.000  0.000
  M2  (2, 1)         0.026  0.014     | M6  (3, 37)        0.048  0.048     | Q2 (3, 37)        0.033  0.033
  M2  (128, 600)     0.212  0.081     | M7  (3, 37)        0.111  0.111     | Q2 (2, 2)         0.002  0.002
  M3  (2, 150)       0.294  0.110     | M7  (2, 3)         0.009  0.009     | Q3 (3, 37)        0.101  0.056
  M3  (40, 600)      0.401  0.161     | M8  (2, 9)         0.007  0.007     | Q4 (3, 131)       0.076  0.061
  M4  (3, 5)         0.054  0.029     | M9  (3, 37)        0.041  0.029     | Q5 (7, 301)       0.138  0.101
  M4  (2, 1)         0.017  0.009     | M10 (7, 301)       0.089  0.091     |
  M4  (2, 40)        0.151  0.107     | M10 (19, 577)      0.123  0.077     |
  (M2 (128, 600) on utterances 0, 43, 82, 109, 127; M3 (40, 600) on 0, 12, 36, 38, 39; M10 (19, 577) on 0, 5, 17, 18)

  Encoder2, worst of the three shapes, f32 / split_f16:  E1 0.010 / 0.010   E2 0.030 / 0.030   E3 0.065 / 0.065   E4 0.011 / 0.010

  conv256 forced, exact fp32 against the fp64 oracle (and how many elements differ in at least one bit from the unforced result);
  bf16 against the emulation, max abs err (beside it the CPU yardstick, the emulation summed in fp64 against fp32), bar 8e-3:
  M1 (3, 57)    0.146  (12 484 of 13 680 differ)    2.4e-3  (1.9e-3)
  M2 (3, 131)   0.152  (45 978 of 50 304)           2.2e-3  (2.4e-3)
  M2 (2, 1)     0.036  (210 of 256)                 3.6e-7  (2.4e-7)
  M3 (2, 150)   0.277  (22 934 of 24 000)           2.2e-3  (2.3e-3)
  M4 (3, 5)     0.072  (1076 of 1200)               4.8e-7  (2.4e-7)
  M4 (2, 1)     0.013  (103 of 160)                 2.4e-7  (2.4e-7)
  M4 (2, 40)    0.224  (6063 of 6400)               1.4e-3  (5.2e-4)
  M5 (17 taps) forced is bit-equal to M5 unforced at both shapes, in fp32 and in bf16.
  bf16 where the library itself takes conv256: M2 (128, 600) 3.3e-3 (2.8e-3), M3 (40, 600) 2.6e-3 (2.7e-3).

  bf16 on the shared tile, max abs err against the emulation (yardstick) and the fraction of rtol = atol = 3e-2 against the fp64 oracle:
  M9 (3, 37) 3.0e-8 (2.4e-7) 0.443    M10 (7, 301) 2.8e-3 (2.6e-3) 0.563    M5 (2, 40) 5.8e-4 (1.5e-3) 0.465    M5 (3, 7) 3.2e-5 (2.0e-6) 0.302

  Ragged batches: every row bit-equal to the utterance alone in every mode run, M10's 16-bit modes across the 128 x 128 and the
  64 x 64 tile included; rows alone at most 0.214 of the fp32 bar (M4 f32 forced conv256) and 0.322 of the bf16 bar (M10).
"""
import pytest
import torch

import hip_helpers as H
import postnet_corner_cases as K
import torch_tts_amd as T
from test_postnet_corners_host import ATOL, BF16_BAR, BF16_CASES, FORCED, RTOL, case_weights, encoder_ref, postnet_ref, ratio_close
from torch_tts_amd.engine import Engine, Handle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POSTNETS = list(K.MEL_CASES) + list(K.MEL2_CASES)
BF16_ORACLE_TOL = 3e-2  # rtol = atol, test_hip_parity.test_postnet_low_precision_modes_vs_oracle's
_built = {}  # case -> the module on the GPU, shared by the tests of this module


@pytest.fixture(scope="module", autouse=True)
def _drop_modules():
    yield
    _built.clear()


def module(name):
    if name not in _built:
        _built[name] = K.make_module(T, name).to(DEV).eval()
    return _built[name]


def run(name, x, mode, lengths=None):
    """The case's Postnet on x [B, T, d] (a CPU tensor) in `mode`; the result on the CPU."""
    m = module(name)
    m.precision = mode
    try:
        with torch.no_grad():
            return m(x.to(DEV), lengths=lengths).cpu()
    finally:
        m.precision = "f32"


def run_encoder(name, ids, lengths, mode):
    m = module(name)
    m.precision = mode
    try:
        with torch.no_grad():
            return m(ids.to(DEV), lengths).cpu()
    finally:
        m.precision = "f32"


def check_bar(got, ref, what):
    """got against the fp64 ref at rtol 1e-4 / atol 1e-5; the worst fraction of the bar is printed first."""
    r = ratio_close(got, ref)
    print(f"{what}: worst |err| / (atol + rtol |ref|) = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.3f} of the bar"
    return r


def check_bf16(got, emu, what, yardstick=None):
    err = float((got - emu).abs().max())
    y = "" if yardstick is None else f"; CPU yardstick (the emulation summed in fp64 against fp32) {float((yardstick - emu).abs().max()):.2e}"
    print(f"{what}: max abs err vs the bf16 emulation {err:.3e} (bar {BF16_BAR}){y}")
    assert err < BF16_BAR, f"{what}: {err:.3e}"


def emulation(name, x, **kw):
    return H.postnet_bf16_emulation(x, case_weights(name), K.layers_of(name), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# parity: every case and shape, exact fp32 and split-fp16
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "split_f16"])
@pytest.mark.parametrize("name,B,T_", K.postnet_shapes())
def test_postnet_parity(name, B, T_, mode):
    """The whole batch runs on the GPU; the oracle's utterances are all of them, or at the three large shapes the sample of
    postnet_corner_cases.oracle_utterances for this device's CU count."""
    x, rows, ref = postnet_ref(name, B, T_, H.device_cus())
    out = run(name, x, mode)
    assert out.shape == x.shape
    check_bar(out[rows], ref, f"{name} ({B}, {T_}) {mode}" + (f" utterances {rows}" if len(rows) < B else ""))


@pytest.mark.parametrize("name,B,T_", [("M2", 128, 600), ("M3", 40, 600)])
def test_bf16_where_the_library_itself_takes_conv256(name, B, T_):
    """Whole 256-row tiles, then short ones, with Cin != N (M2's layer 0), one column tile (M2) and three (M3), 3 and 7 taps."""
    x, rows, _ = postnet_ref(name, B, T_, H.device_cus())
    check_bf16(run(name, x, "bf16")[rows], emulation(name, x[rows]), f"{name} ({B}, {T_}) bf16 utterances {rows}", emulation(name, x[rows], acc=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# a 16-bit request that cannot take the planes is the exact fp32 path, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in POSTNETS if K.stays_fp32(n)])
def test_postnet_fallback_is_the_fp32_path(name):
    assert name in ("M6", "M7", "M8", "Q1", "Q2")
    for B, T_ in K.case(name)["shapes"]:
        x, _, _ = postnet_ref(name, B, T_)
        f32 = run(name, x, "f32")
        assert torch.equal(run(name, x, "split_f16"), f32), f"{name} ({B}, {T_}): split_f16 is not the fp32 path"
        assert torch.equal(run(name, x, "bf16"), f32), f"{name} ({B}, {T_}): bf16 is not the fp32 path"


@pytest.mark.parametrize("name", ["M9", "Q3"])
def test_the_smallest_dims_with_whole_columns_take_the_planes(name):
    B, T_ = K.case(name)["shapes"][0]
    x, _, _ = postnet_ref(name, B, T_)
    f32 = run(name, x, "f32")
    assert not torch.equal(run(name, x, "split_f16"), f32), f"{name}: split_f16 gave the fp32 path's bits"
    assert not torch.equal(run(name, x, "bf16"), f32), f"{name}: bf16 gave the fp32 path's bits"


# ---------------------------------------------------------------------------------------------------------------------------
# conv256 at its untested instantiations (TTSDEC_CONV256_FORCE=1)
# ---------------------------------------------------------------------------------------------------------------------------
def small_shapes(name):
    return [(B, T_) for B, T_ in K.MEL_CASES[name]["shapes"] if B * T_ <= K.LARGE_ROWS]


@pytest.mark.parametrize("name", FORCED)
def test_forced_conv256(name, monkeypatch):
    """1, 3, 7 and 15 taps; Cin = 128 != N (M2's layer 0); one, two and three column tiles; utterances shorter than taps / 2.
    Exact fp32 against the fp64 oracle at the fp32 bar, bf16 against the emulation; and the forced fp32 result differs in at least
    one bit from the unforced one (another kernel, another summation order over K >= 384) - the library has no query for which
    kernel a call took, so this is how the test knows that the switch did something."""
    cus = H.device_cus()
    for B, T_ in small_shapes(name):
        for eb in (4, 2):  # on this device too: forced, conv256 takes every hidden -> hidden layer; unforced, none at this size
            for c, n, t in K.conv_layers(name)[1:]:
                assert H.conv256_schedule(B * T_, cus, Cin=c, N=n, taps=t, elem_bytes=eb, force=True) is not None, (name, B, T_, eb)
                assert H.conv256_schedule(B * T_, cus, Cin=c, N=n, taps=t, elem_bytes=eb) is None, (name, B, T_, eb)
        x, rows, ref = postnet_ref(name, B, T_)
        plain = run(name, x, "f32")
        with monkeypatch.context() as mp:
            mp.setenv("TTSDEC_CONV256_FORCE", "1")
            forced, forced_bf16 = run(name, x, "f32"), run(name, x, "bf16")
        what = f"{name} ({B}, {T_}) forced conv256"
        check_bar(forced, ref, what + " f32")
        n_diff = int((forced != plain).sum())
        print(f"{what} f32: {n_diff} of {forced.numel()} elements differ in at least one bit from the unforced result")
        check_bf16(forced_bf16, emulation(name, x), what + " bf16", emulation(name, x, acc=torch.float64))
        assert n_diff > 0, f"{what}: bit-equal to the unforced result - the shared tile ran, or both kernels sum in one order"


def test_17_taps_stay_on_the_shared_tile_when_forced(monkeypatch):
    for B, T_ in K.MEL_CASES["M5"]["shapes"]:
        x, _, _ = postnet_ref("M5", B, T_)
        plain = {mode: run("M5", x, mode) for mode in ("f32", "bf16")}
        with monkeypatch.context() as mp:
            mp.setenv("TTSDEC_CONV256_FORCE", "1")
            for mode in ("f32", "bf16"):
                assert torch.equal(run("M5", x, mode), plain[mode]), f"M5 ({B}, {T_}) {mode}: forced differs from unforced"


# ---------------------------------------------------------------------------------------------------------------------------
# bf16 on the shared tile
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,T_", [("M9", 3, 37), ("M10", 7, 301)] + [("M5", B, T_) for B, T_ in K.MEL_CASES["M5"]["shapes"]])
def test_bf16_on_the_shared_tile(name, B, T_):
    """M9: one 16-byte column per tap; M10: the 128 x 128 tile with a ragged last column tile; M5: 17 taps.  Against the emulation
    at its bar and against the fp64 oracle at the project's rtol = atol = 3e-2 for bf16."""
    x, rows, ref = postnet_ref(name, B, T_)
    out = run(name, x, "bf16")
    check_bf16(out, emulation(name, x), f"{name} ({B}, {T_}) bf16", emulation(name, x, acc=torch.float64))
    r = float(((out.double() - ref).abs() / (BF16_ORACLE_TOL + BF16_ORACLE_TOL * ref.abs())).max())
    print(f"{name} ({B}, {T_}) bf16: {r:.3f} of rtol = atol = {BF16_ORACLE_TOL} against the fp64 oracle")
    assert r <= 1.0, (name, r)


# ---------------------------------------------------------------------------------------------------------------------------
# ragged batches
# ---------------------------------------------------------------------------------------------------------------------------
def _ragged(name, mode, what):
    x, lengths = K.ragged_input(name)
    B, T_ = K.RAGGED_SHAPES[name]
    out = run(name, x, mode, lengths=torch.tensor(lengths, device=DEV))
    assert torch.equal(out, run(name, x, mode, lengths=lengths)), what + ": a host list of lengths gives other bits"
    bf16 = mode == "bf16" and not K.stays_fp32(name)
    worst = 0.0
    for b, n in enumerate(lengths):
        assert not bool(out[b, n:].any()), f"{what} row {b}: not zero from its length {n} on"
        if not n:
            continue
        alone = run(name, x[b : b + 1, :n], mode)
        assert torch.equal(out[b, :n], alone[0]), f"{what} row {b} ({n} frames): not the bits of the utterance alone"
        assert bool(torch.isfinite(alone).all()), f"{what} row {b}"
        if bf16 and name in K.MEL_CASES:
            worst = max(worst, float((alone - emulation(name, x[b : b + 1, :n])).abs().max()) / BF16_BAR)
        elif bf16:  # MelPostnet2 has no emulation of its bf16 arithmetic: the figure against the fp64 oracle is printed, not asserted
            ref = K.postnet_oracle(name, x[b : b + 1, :n], case_weights(name), torch.float64)
            print(f"{what} row {b} alone: max |err| / (1 + |ref|) = {float(((alone.double() - ref).abs() / (1 + ref.abs())).max()):.2e} against the fp64 oracle")
        else:
            worst = max(worst, ratio_close(alone, K.postnet_oracle(name, x[b : b + 1, :n], case_weights(name), torch.float64)))
    if not bf16 or name in K.MEL_CASES:
        print(f"{what}: lengths {lengths}; rows alone at most {worst:.3f} of " + (f"{BF16_BAR} from the bf16 emulation" if bf16 else "the bar from the fp64 oracle"))
    assert worst <= 1.0, what


@pytest.mark.parametrize("name", list(K.RAGGED_SHAPES))
def test_ragged_batches(name, monkeypatch):
    """forward(x, lengths=) with lengths T, 0, 1, one below taps / 2 and one in between, 1e3 beyond each length: row b is, bit
    for bit, the module on x[b : b + 1, :n] alone, and exactly zero from n on.  (M10 in the 16-bit modes: the batch of 2107
    rows runs on the 128 x 128 tile, an utterance alone on the 64 x 64 one; both walk K in one order with one accumulator per
    output, so the bits agree across the two tiles - this test is what says so.)  Each utterance alone - shapes of 1 to T frames
    that no other test runs - is also held to the fp64 oracle at the fp32 bar (f32, split_f16) or to the bf16 emulation at its bar;
    MelPostnet2 has no emulation of its bf16 arithmetic, so Q3's bf16 rows are compared bit for bit only."""
    modes = ["f32"] + ([] if K.stays_fp32(name) else ["split_f16", "bf16"])
    for mode in modes:
        _ragged(name, mode, f"{name} ragged {mode}")
    if name == "M4":
        monkeypatch.setenv("TTSDEC_CONV256_FORCE", "1")
        for mode in ("f32", "bf16"):
            _ragged(name, mode, f"{name} ragged {mode} forced conv256")


# ---------------------------------------------------------------------------------------------------------------------------
# rows alone and twice
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POSTNETS)
def test_postnet_rows_alone_and_twice(name):
    """Twice the same bits in every mode.  One utterance alone gives its row of the batch bit for bit in exact fp32 at the case's
    first shape, where the batch and the utterance both run every layer on the 32 x 32 tile that splits K over four waves
    (asserted by restatement; conv256 is not taken unforced at these sizes) - a batch that changes the tile launch_gemm_cfg picks
    changes the summation order, as the existing tests say, and is not compared bit for bit."""
    B, T_ = K.case(name)["shapes"][0]
    d, hidden = K.case(name)["dims"][:2]
    x, _, _ = postnet_ref(name, B, T_)
    for mode in ("f32", "split_f16", "bf16"):
        assert torch.equal(run(name, x, mode), run(name, x, mode)), f"{name} {mode}: two identical calls differ"
    for N in (hidden, d):
        assert K.shared_tile("f32", B * T_, N) == K.shared_tile("f32", T_, N) == "32x32", name
    if name in K.MEL_CASES:
        assert all(H.conv256_schedule(M, H.device_cus(), Cin=c, N=n, taps=t, elem_bytes=4) is None for M in (B * T_, T_) for c, n, t in K.conv_layers(name))
    batch = run(name, x, "f32")
    for b in sorted({0, B - 1}):
        assert torch.equal(run(name, x[b : b + 1], "f32")[0], batch[b]), f"{name}: row {b} alone differs from its row of the batch"


# ---------------------------------------------------------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("M7", "f32"), ("Q3", "f32"), ("M9", "split_f16"), ("Q3", "split_f16")])
def test_postnet_workspace_fits(name, mode, monkeypatch):
    x, _, _ = postnet_ref(name, 3, 37)
    H.assert_workspace_fits(monkeypatch, Engine, "postnet_workspace", lambda eng, B, T_: eng.postnet_workspace_bytes(B, T_), lambda: run(name, x, mode))


@pytest.mark.parametrize("mode", ["f32", "split_f16"])
def test_encoder_workspace_fits(mode, monkeypatch):
    ids, lengths, _ = encoder_ref("E3", 0)
    H.assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, kind, nbytes: nbytes, lambda: run_encoder("E3", ids, lengths, mode))


# ---------------------------------------------------------------------------------------------------------------------------
# Encoder2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "split_f16"])
@pytest.mark.parametrize("name", list(K.ENC_CASES))
def test_encoder_parity(name, mode):
    for i, (B, L, lengths) in enumerate(K.ENC_SHAPES):
        ids, lens, ref = encoder_ref(name, i)
        out = run_encoder(name, ids, lens, mode)
        assert out.shape == (B, max(lengths), K.case(name)["dims"][2]) == ref.shape, (name, i, out.shape)
        check_bar(out, ref, f"{name} (B, L, lengths) = {K.ENC_SHAPES[i]} {mode}")
        for b, n in enumerate(lengths):
            assert not bool(out[b, n:].ne(0).any()), f"{name}/{i} row {b}: not zero past its length"
        assert torch.equal(out, run_encoder(name, ids, lens, mode)), f"{name}/{i} {mode}: two identical calls differ"


@pytest.mark.parametrize("name", list(K.ENC_CASES))
def test_encoder_fallback_and_rows_alone(name):
    """d_emb % 8 == 4 (E1, E2, E3): a split-fp16 request is the exact fp32 path bit for bit.  Row 0 alone - its row of ids as it
    stands, so the convs see the same padded columns - gives its row of the batch (1 and 3 utterances: the same tiles)."""
    ids, lens, _ = encoder_ref(name, 0)
    f32 = run_encoder(name, ids, lens, "f32")
    if K.stays_fp32(name):
        assert name in ("E1", "E2", "E3")
        for i in range(len(K.ENC_SHAPES)):
            ids_i, lens_i, _ = encoder_ref(name, i)
            assert torch.equal(run_encoder(name, ids_i, lens_i, "split_f16"), run_encoder(name, ids_i, lens_i, "f32")), f"{name}/{i}: split_f16 is not the fp32 path"
    for b in (0, 2):
        n = int(lens[b])
        alone = run_encoder(name, ids[b : b + 1], lens[b : b + 1], "f32")
        assert alone.shape == (1, n, f32.shape[2]) and torch.equal(alone[0], f32[b, :n]), f"{name}: row {b} alone differs from its row of the batch"
