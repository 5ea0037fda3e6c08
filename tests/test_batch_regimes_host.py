"""The input conditions of the batch-regime GPU tests (test_batch_regimes_hip.py, and the cases of test_hip_parity.py that
batch_regime_cases.py restates), checked on the CPU: a GPU test must not pass because its inputs let it."""
import pytest
import torch

import batch_regime_cases as C

DECODE_CASES = C.REGIME_EDGES + C.F32_QUERY_ROLE_EDGES + C.STANDALONE_64x8 + [C.ISOLATION]


def test_every_regime_edge_has_a_case():
    """Both sides of every boundary of the section-6 table (csrc/api.hip overlap_level / query_role, csrc/fused_kernels.hip
    lean_kind, csrc/decode_kernels.hip launch_lstm), one case each."""
    have = {(c.prec, c.B) for c in C.REGIME_EDGES}
    assert have == {("split_f16", b) for b in (32, 33, 64, 65, 384, 385)} | {("f32", b) for b in (32, 33, 96, 97, 128, 129)}
    assert len(have) == len(C.REGIME_EDGES)
    assert [(c.prec, c.B) for c in C.F32_QUERY_ROLE_EDGES] == [("f32", b) for b in (191, 192, 256, 257)]
    for c in C.REGIME_EDGES + C.F32_QUERY_ROLE_EDGES:
        if c.prec == "f32":
            assert (c.names == C.LEVEL1) == (97 <= c.B <= 128), c  # overlap_level: level 1 from 97 to 128 only
            assert (c.names == C.TWO) == (192 <= c.B <= 256), c    # query_role: exact fp32 from 192 to 256
        else:
            assert (c.names == C.TWO) == (64 <= c.B <= 384), c     # query_role: split-fp16 from 64 to 384
    assert {(c.prec, c.B) for c in C.STANDALONE_64x8} == {(p, b) for p in ("f32", "split_f16") for b in (96, 128)}
    assert all(c.options == "overlap=0" and c.names == C.LEVEL0 for c in C.STANDALONE_64x8)
    assert 97 <= C.ISOLATION.B <= 128 and C.ISOLATION.B % 64 and C.isolation_rows(C.ISOLATION.B) == [0, 64, C.ISOLATION.B - 1]
    assert 100 in C.OPTION_MATRIX_B and 96 < 100 <= 128  # above kLean8MaxRowsF32, inside launch_lstm's 64 x 8 branch


@pytest.mark.parametrize("case", DECODE_CASES, ids=lambda c: c.id)
def test_reduced_dims_case_tolerates_no_row(case):
    mem, masks, (oy, os_, ow) = C.decode_inputs(case)
    lens = C.case_lengths(case)
    assert len(lens) == case.B and lens[-2:] == [4, 1] and max(lens) == C.L_MEM
    assert mem.shape == (case.B, C.L_MEM, C.REDUCED["d_ctx"]) and masks.shape[0] == C.T_STEPS >= 15
    assert oy.shape == (case.B, C.T_STEPS, C.REDUCED["d_mel"]), "the oracle's stop rule must not fire: all steps are compared"
    assert float(os_.min()) > -2.0 + 0.5
    gap = C.top2_gap(ow)
    assert gap >= C.MIN_TOP2_GAP, f"{case.id}: a row's two largest weights are {gap:.2e} apart: assert_argmax would tolerate it"


@pytest.mark.parametrize("B", C.OPTION_MATRIX_B)
def test_option_matrix_case_tolerates_no_row(B):
    oy, os_, ow = C.option_matrix_oracle(B)
    assert oy.shape[1] == C.T_STEPS
    assert C.top2_gap(ow) >= C.MIN_TOP2_GAP, (B, C.top2_gap(ow))


@pytest.mark.parametrize("B,L,T,lengths", C.LJSPEECH_CASES)
def test_ljspeech_dims_case_tolerates_no_row(B, L, T, lengths):
    oy, os_, ow = C.ljspeech_oracle(B, L, T, lengths)
    assert oy.shape == (B, T, 80)
    assert C.top2_gap(ow) >= C.MIN_TOP2_GAP, (B, C.top2_gap(ow))
    if lengths is not None:
        assert len(lengths) == B and max(lengths) == L and min(lengths) == 1 and lengths[64] < L  # ragged in both 64-row blocks


@pytest.mark.parametrize("B", C.TACO2_B)
def test_taco2_case_tolerates_no_row(B):
    *_, (oy, os_, ow) = C.taco2_inputs(B)
    assert oy.shape == (B, C.TACO2_T, 80)
    assert C.top2_gap(ow) >= C.MIN_TOP2_GAP, (B, C.top2_gap(ow))


@pytest.mark.parametrize("B, L", [(b, C.ENC_L) for b in C.ENC_B] + [(b, C.ENC_LJ_L) for b in C.ENC_LJ_B])
def test_encoder_length_sets(B, L):
    sets = C.enc_length_sets(B, L)
    assert [s[0] for s in sets] == ["full", "short"] and [s[1] for s in sets] == [L, L - 3]
    first_of_last_tile = ((B - 1) // 64) * 64
    assert first_of_last_tile not in (0, B - 1) or B in (193, 257)  # (193, 257: the last tile is its one row)
    for name, l_max, lens in sets:
        assert lens.shape == (B,) and lens.dtype == torch.int64
        assert int(lens.min()) >= 1, "pack_padded_sequence refuses a zero length"
        assert int(lens.max()) == l_max == int(lens[0])
        assert int(lens[B - 1]) == 1 and int(lens[first_of_last_tile]) == 1
        assert lens.unique().numel() >= min(l_max, 8), "lengths must be spread"
        alphabet = C.ENC_ALPHABET if L == C.ENC_L else C.ENC_LJ[0]
        l_max2, lens2, ids = C.enc_case(B, L, alphabet, name)
        assert l_max2 == l_max and torch.equal(lens, lens2) and ids.shape == (B, L)
        pad = torch.arange(L)[None, :] >= lens[:, None]
        assert bool((ids[pad] == 0).all()) and bool((ids[~pad] >= 1).all()) and int(ids.max()) < alphabet


def test_encoder_small_dims_reach_the_ragged_unit_tile():
    """H = d_out / 2 must be no multiple of 8 or 16 (the last unit block of both LSTM tiles is ragged) and satisfy what
    Encoder2.forward asks of the HIP path (d_emb % 4 == 0, d_out % 8 == 0 - else the module would run stock ops)."""
    for d_emb, d_out in C.ENC_SMALL_DIMS:
        H = d_out // 2
        assert H % 8 and H % 16 and d_emb % 4 == 0 and d_out % 8 == 0
    assert C.ENC_SMALL_DIMS[0][0] % 8 == 0 and C.ENC_SMALL_DIMS[1][0] % 8 != 0  # (split_f16 applies / falls to the fp32 GEMMs)
    assert C.ENC_SMALL_DIMS[0][1] // 2 < 32 < C.ENC_SMALL_DIMS[1][1] // 2  # K shorter / longer than one 128-byte K tile
