"""CPU proof that the cases of tests/vits2_attention_cases.py are what tests/test_vits2_attention_hip.py takes them for: the
restated flash algorithm is exact, the `scaled` and `ramp` inputs move the lazy running maximum where they claim to, every case is
well conditioned at the project's bar, the planted rescale faults would be seen, and the restated dispatch switches kernels at
the lengths and windows worked out by hand below.  No GPU, no native library."""
import pytest
import torch

import vits2_attention_cases as A

F32, F64 = torch.float32, torch.float64
_ids = A.spec_id


def _moves(case):
    q, k, _, m = case.layer0_qkv()
    return A.lazy_max_moves(A.base2_scores(q, k, m), case.T)  # [tile, B, head, query]


def _query_units(out, ref):
    """per (utterance, query): max over heads and channels of err / (atol + rtol |ref|)  ->  [B, T]"""
    return ((out - ref).abs() / (A.ATOL + A.RTOL * ref.abs())).amax(-1).amax(1)


# ---- flash_emulation itself ----
def test_flash_emulation_without_a_fault_is_the_exact_softmax():
    """fp64, 1e-12: masked queries (every score -1e4: uniform), fully masked key tiles, a ragged last tile, one key, scores far
    apart (moves at every tile) and close together (none)."""
    g = torch.Generator().manual_seed(1)
    for T, lens, scale in ((300, (300, 223, 1), 6.0), (75, (75, 33, 32), 1.0), (33, (33, 1, 17), 20.0), (1, (1, 1, 1), 3.0), (32, (32, 31, 5), 0.1)):
        B, h, dk = len(lens), 2, 16
        q = torch.randn(B, h, T, dk, generator=g, dtype=F64) * scale
        k, v = torch.randn(B, h, T, dk, generator=g, dtype=F64), torch.randn(B, h, T, dk, generator=g, dtype=F64)
        mask = A.V.sequence_mask(torch.tensor(lens), T).unsqueeze(1).double()
        ref = A.exact_attention(q, k, v, mask)
        out = A.flash_emulation(q, k, v, mask)
        assert torch.isfinite(out).all()
        assert float((out - ref).abs().max()) <= 1e-12, (T, float((out - ref).abs().max()))
        # a masked query attends uniformly over all T keys
        b = len(lens) - 1
        if lens[b] < T:
            assert float((out[b, :, lens[b]:] - v[b].mean(1, keepdim=True)).abs().max()) <= 1e-12


def test_flash_emulation_faults_change_a_two_tile_result():
    g = torch.Generator().manual_seed(2)
    T, dk = 64, 16
    q, k, v = (torch.randn(1, 1, T, dk, generator=g, dtype=F64) for _ in range(3))
    k[..., 32:, :] += 3 * q.mean(2, keepdim=True)  # (second tile: larger scores for most queries)
    q = q * 6
    mask = torch.ones(1, 1, T, dtype=F64)
    assert A.lazy_max_moves(A.base2_scores(q, k, mask), T)[1].any()
    ref = A.exact_attention(q, k, v, mask)
    for f in A.FAULTS:
        assert float((A.flash_emulation(q, k, v, mask, f) - ref).abs().max()) > 1e-3, f


def test_lazy_max_moves_on_a_hand_made_row():
    # tiles of 32 keys: maxima 0, 8 (not MORE than 8 above: stays), 8.5 (moves: m = 8.5), 16 (7.5 above: stays), 17 (moves), ragged 1 key 30
    s = torch.full((1, 161), -50.0, dtype=F64)
    for j, val in ((3, 0.0), (40, 8.0), (95, 8.5), (100, 16.0), (130, 17.0), (160, 30.0)):
        s[0, j] = val
    assert A.lazy_max_moves(s, 161)[:, 0].tolist() == [False, False, True, False, True, True]
    assert A.lazy_max_moves(s, 160)[:, 0].tolist() == [False, False, True, False, True]  # key 160 does not exist


# ---- coverage: what the flash cases make the kernel do ----
@pytest.mark.parametrize("channels", A.FLASH_CHANNELS)
def test_scaled_moves_the_lazy_maximum_where_the_gpu_test_needs_it(channels):
    case = A.flow_case("scaled", channels)
    assert case.T == 300 and case.lengths == (300, 223) and case.choice("split_f16") == f"flash<{channels // 4}>"
    mv = _moves(case)
    assert mv.shape == (10, 2, 2, 300)
    full, short = mv[:, 0, :, :300], mv[:, 1, :, :223]
    per_tile = full.sum((1, 2)).tolist()
    print(f"scaled {channels}: moves per tile {per_tile} (full), {short.sum((1, 2)).tolist()} (length 223), max per query {int(mv.sum(0).max())}")
    assert all(n >= 1 for n in per_tile[1:]), per_tile  # a move at each of tiles 1..9, the ragged tile 9 (12 keys) among them
    assert int(short[7:].sum()) == 0 and int(short[1:7].sum()) > 0  # none at the fully masked tiles of the short utterance
    assert int(mv[:, 1, :, 223:].sum()) == 0  # masked queries: every score is the fill value
    per_query = full.sum(0)
    assert bool((per_query == 0).any()) and bool((per_query >= 2).any())
    # some 32-query group (one wave's queries) where at one tile some lanes move and others do not: alpha is per lane
    groups = torch.nn.functional.pad(full, (0, 20)).unflatten(-1, (-1, 32))[..., :9, :]  # (the 9 whole groups)
    assert bool((groups.any(-1) & ~groups.all(-1)).any())


@pytest.mark.parametrize("channels", A.FLASH_CHANNELS)
def test_ramp_moves_at_every_valid_tile_or_never(channels):
    up, down = A.flow_case("ascending", channels), A.flow_case("descending", channels)
    q, k, _, m = up.layer0_qkv()
    # the planted scores: slope * j nats for every valid query
    s = (q @ k.transpose(-1, -2))[0, :, :, :]
    want = A.ramp_slope(up.dk) * torch.arange(300, dtype=F64)
    assert A.ramp_slope(up.dk) in (0.5, 0.75) and float((s - want).abs().max()) <= 1e-5
    mu, md = _moves(up), _moves(down)
    for b, n in enumerate(up.lengths):
        valid_tiles = (n + 31) // 32
        assert bool((mu[:, b, :, :n].sum(0) == valid_tiles - 1).all()), (b, mu[:, b, :, :n].sum(0).unique())
        assert bool(mu[1:valid_tiles, b, :, :n].all())
        assert int(md[:, b].sum()) == 0
    assert int(mu[:, 1, :, 223:].sum()) == 0


# ---- conditioning: the fp32 oracle against its own fp64 run ----
@pytest.mark.parametrize("spec", A.FLOW_SPECS, ids=_ids)
def test_flow_cases_are_well_conditioned(spec):
    case = A.flow_case(*spec)
    u = A.bar_units(case.reference(F32), case.reference(F64))
    print(f"{case.name}: fp32 oracle vs fp64 oracle {u:.2f} of the bar")
    assert u <= 0.7, u


@pytest.mark.parametrize("spec", A.TEXT_SPECS, ids=_ids)
def test_text_cases_are_well_conditioned(spec):
    case = A.text(*spec)
    us = [A.bar_units(a, b) for a, b in zip(case.reference(F32), case.reference(F64))]
    print(f"{case.name}: fp32 oracle vs fp64 oracle {us} of the bar (x, m, logs)")
    assert max(us) <= 0.7, us


def test_the_scale_of_six_is_about_as_far_as_the_conditioning_goes():
    """s = 12 at 256 channels leaves the fp32 oracle itself outside 0.7 of the bar: the factor cannot simply be raised."""
    c = A.scaled(256, 12.0)
    assert A.bar_units(c.reference(F32), c.reference(F64)) > 0.7


# ---- discriminating power: what a planted fault does to the layer-0 attention output ----
@pytest.mark.parametrize("channels", A.FLASH_CHANNELS)
def test_planted_faults_would_be_seen(channels):
    """`scaled` sees every fault on at least 5 % of each utterance's valid queries, by more than 100 x rtol.  The ascending ramp sees
    the two faults that lose a factor, skip_lsum and skip_y, on EVERY valid query.  It cannot see the other two, and does not claim
    to: all queries of a group move together with one alpha (wave_uniform_alpha changes nothing), and with the same alpha at every
    full tile rescale_after_p only applies each tile's factor one tile late, which leaves every ratio y / lsum as it was up to the
    ragged tile's share (a few 1e-3) - `scaled`, where alpha differs from lane to lane and tile to tile, is the case that does."""
    case = A.flow_case("scaled", channels)
    q, k, v, m = case.layer0_qkv()
    ref = A.exact_attention(q, k, v, m)
    assert float((A.flash_emulation(q, k, v, m) - ref).abs().max()) <= 1e-12
    for f in A.FAULTS:
        u = _query_units(A.flash_emulation(q, k, v, m, f), ref)
        for b, n in enumerate(case.lengths):
            frac = float((u[b, :n] > 100).float().mean())
            print(f"scaled {channels} {f}: {frac:.2f} of utterance {b}'s valid queries off by > 100 rtol")
            assert frac >= 0.05, (f, b, frac)
        assert float(u[1, 224:].max()) <= 1e-6  # (masked queries never rescale; 223 shares its 32-query group with valid ones)
    case = A.flow_case("ascending", channels)
    q, k, v, m = case.layer0_qkv()
    ref = A.exact_attention(q, k, v, m)
    assert float((A.flash_emulation(q, k, v, m) - ref).abs().max()) <= 1e-12
    for f in ("skip_lsum", "skip_y"):
        u = _query_units(A.flash_emulation(q, k, v, m, f), ref)
        for b, n in enumerate(case.lengths):
            assert bool((u[b, :n] > 100).all()), (f, b, float(u[b, :n].min()))


@pytest.mark.parametrize("channels", A.FLASH_CHANNELS)
def test_planted_faults_reach_the_flow_output(channels):
    """What the GPU test compares is the flow's output, two attention layers, two FFNs and a WN behind the first attention.  The
    fp64 oracle with that attention's softmax-and-P V replaced by the faulty emulation ends more than 100 bars from the plain one
    (the GPU test allows 1) for every fault the case claims to see; with the emulation without a fault it ends where it was."""
    for kind, faults in (("scaled", A.FAULTS), ("ascending", ("skip_lsum", "skip_y"))):
        case = A.flow_case(kind, channels)
        assert A.bar_units(case.reference_with_fault(None), case.reference(F64)) <= 1e-3
        for f in faults:
            u = A.bar_units(case.reference_with_fault(f), case.reference(F64))
            print(f"{kind} {channels} {f}: flow output {u:.0f} bars off")
            assert u > 100, (kind, f, u)


# ---- the restated dispatch at its boundaries ----
def test_mha_choice_at_the_lds_boundaries():
    """150 KiB = 153 600 bytes = 38 400 floats.
    Text encoder, dk 96, window 4: S 32 (T | 1) + R 32 * 33 + rinv 32 floats.  T = 1165: 37 280 + 1 088 = 38 368 <= 38 400: mfma.
      T = 1166: T | 1 = 1167: 37 344 + 1 088 = 38 432 > 38 400: scalar, whose 16 * 96 + 64 * 97 + 2 * 9 * 96 + 16 * 1166 = 28 128 floats fit.
    Flow, dk 48, no window: 32 (T | 1) + 32.  T = 1199: 38 368 + 32 = 38 400: mfma (the limit itself).  T = 1200: 1201 * 32 + 32 = 38 464: scalar."""
    assert A.mha_mfma_lds_bytes(1165, 96, 4) == 153472 and A.mha_mfma_lds_bytes(1166, 96, 4) == 153728
    assert A.mha_lds_bytes(1166, 96, 4) == 112512
    assert A.mha_mfma_lds_bytes(1199, 48, -1) == 153600 and A.mha_mfma_lds_bytes(1200, 48, -1) == 153856
    for prec in ("f32", "split_f16"):
        assert A.mha_choice(1165, 96, 4, prec, 192) == "mfma<48>"
        assert A.mha_choice(1166, 96, 4, prec, 192) == "scalar"
    assert A.mha_choice(1199, 48, None, "f32", 96) == "mfma<24>"
    assert A.mha_choice(1200, 48, None, "f32", 96) == "scalar"
    assert A.mha_choice(1200, 48, -1, "split_f16", 96) == "flash<48>"  # (the flash kernel holds no score tile)
    assert A.mha_choice(1300, 48, None, "f32", 96) == "scalar"  # test_flow_reverse_long_sequence_uses_the_scalar_attention_fallback
    # short sequences: the reduction buffer 4 * 32 * (dk + 1) + 9 * dk floats is the larger part
    assert A.mha_mfma_lds_bytes(1, 96, 4) == (4 * 32 * 97 + 9 * 96) * 4
    # the scalar kernel's own limit: 16 T floats of scores.  dk 32, no window: 512 + 2 112 + 16 T <= 38 400 up to T = 2 236
    assert A.mha_choice(2236, 32, None, "f32", 64) == "scalar"
    with pytest.raises(ValueError):
        A.mha_choice(2237, 32, None, "f32", 64)
    with pytest.raises(ValueError):
        A.mha_choice(10, 260, None, "f32", 520)


def test_mha_choice_by_window_width_and_precision():
    assert A.mha_choice(100, 16, 15, "f32", 32) == "mfma<8>"  # nrel = 31: finish<31>
    assert A.mha_choice(100, 16, 16, "f32", 32) == "scalar"
    assert A.mha_choice(100, 16, 0, "split_f16", 32) == "mfma<8>"  # a window of 0 is still a window: no flash
    got = {dk: (A.mha_choice(300, dk, None, "f32", 2 * dk), A.mha_choice(300, dk, None, "split_f16", 2 * dk)) for dk in (8, 16, 32, 48, 64, 96)}
    assert got == {8: ("mfma<4>", "mfma<4>"), 16: ("mfma<8>", "flash<16>"), 32: ("scalar", "flash<32>"), 48: ("mfma<24>", "flash<48>"),
                   64: ("scalar", "flash<64>"), 96: ("mfma<48>", "mfma<48>")}
    assert {dk: A.mha_choice(300, dk, 4, "split_f16", 2 * dk) for dk in (8, 16, 32, 48, 96)} == {8: "mfma<4>", 16: "mfma<8>", 32: "scalar",
                                                                                                 48: "mfma<24>", 96: "mfma<48>"}
    assert A.flash_grid_order(2, 2) == "plain" and A.flash_grid_order(3, 2) == "plain" and A.flash_grid_order(4, 2) == "remap"


def test_the_case_lists_name_every_instantiation():
    """Together the GPU cases reach every attention kernel the library builds, each in the situation DESIGN.md's table lists."""
    split = A.FLASH_MAIN + A.FLASH_REMAP + A.FLASH_SHORT + A.EXACT_SPLIT
    flow = {(A.flow_case(*s).choice("split_f16"), "split_f16") for s in split} | {(A.flow_case(*s).choice("f32"), "f32") for s in A.EXACT_F32}
    text = {(A.text(*s).choice(p), p) for s in A.TEXT_SPECS for p in ("f32", "split_f16")}
    assert {c for c, _ in flow} == {"flash<16>", "flash<32>", "flash<48>", "flash<64>", "mfma<4>", "mfma<8>", "mfma<24>", "mfma<48>", "scalar"}
    assert {c for c, _ in text} == {"mfma<4>", "mfma<8>", "mfma<24>", "mfma<48>", "scalar"}
    assert ("mfma<4>", "split_f16") in flow and ("mfma<48>", "split_f16") in flow
