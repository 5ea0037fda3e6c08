"""Every batch-size regime of the decode step and of Encoder2 against the CPU oracle.

The tile an LSTM launch runs on and the launch sequence of a step are functions of the batch a call sees; the cases
(batch_regime_cases.py, whose input conditions test_batch_regimes_host.py checks on the CPU) sit on both sides of every boundary:
  A. the decode step of Taco2ProdDecoderCell at each edge of the section-6 table, the launch names of one step as the witness
     that a case ran in the regime it is named for; launch_lstm's 64 x 8 tile alone (overlap=0); row isolation at B = 112;
  B. Taco2DecoderCell (level 1 everywhere: lstm_dec is always launch_lstm's own tile) at 96 and 129 utterances;
  C. Encoder2 with the whole batch in one call - launch_lstm_pair's three tiles and their edges, ragged unit tiles, L_out < L.
The bar is the project's: 1e-4 relative (1e-5 absolute floor) against the oracle, attention argmax equal.  Each test prints the
largest relative error it saw ("regime ..." lines; the measure of test_hip_parity.py's _drift_report: the bar is 1e-4).

Why a broken branch cannot pass (csrc/step_bodies.h lstm_body, csrc/decode_kernels.hip launch_lstm / launch_lstm_pair):
  - a tile picked with the wrong grid (say 16-unit columns launched for an 8-unit tile, or 32-row blocks for a 64-row one) leaves
    units or rows unwritten or written twice from another K order: every case compares all B rows x all units with the oracle;
  - the ragged unit block: H = 20 and 36 end inside the last block of the 8- and the 16-unit tile.  A wrong BU in `unit < H` /
    LoaderWLstm::row_ok (r % BU) makes gate rows of units >= H read the NEXT gate's weights or lets their h land in the next
    row's first units - both change values that the comparison with the oracle covers;
  - the K tail: H = 20 is shorter than one K tile, H = 36 one 128-byte tile + 4; columns past K must read zeros, else h is off by O(1);
  - a swapped seq_reverse position (len - 1 - t), or seq_L used where seq_Lout belongs, moves the reverse half of every row
    longer than one token / every row of the L_out < L length set: the lengths are spread over [1, L] in every 64-row block;
  - an ended row that kept running would write past its length: the exactly-zero padding check covers every row;
  - rows leaking into each other inside a tile (row index mix-ups across the 32-row halves of a 64-row tile) change the three
    kept rows of the isolation checks, which sit at the first row, the last row and the first row of the last 64-row block;
  - the 97-128 decode regime on another launch sequence or tile than DESIGN.md names fails the launch-name assertion."""
import functools

import pytest
import torch

import batch_regime_cases as C
from oracle import tacotron_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = C.RTOL, C.ATOL


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import hip_helpers

    return hip_helpers


def _rel(a, b):
    """largest relative error, |a - b| / (ATOL / RTOL + |b|): test_hip_parity.py _drift_report's measure, whose bar is RTOL"""
    return float(((a - b).abs() / (ATOL / RTOL + b.abs())).max())


def _check_decode(H, what, got, want):
    (y, s, w, fired), (oy, os_, ow) = got, want
    assert not fired and y.shape == oy.shape and w.shape == ow.shape, what
    print(f"regime {what}: max rel err  y {_rel(y, oy):.2e}  s {_rel(s, os_):.2e}  w {_rel(w, ow):.2e}")
    H.assert_close(y, oy, RTOL, ATOL, "y " + what)
    H.assert_close(s, os_, RTOL, ATOL, "s " + what)
    H.assert_close(w, ow, RTOL, ATOL, "w " + what)
    H.assert_argmax(w, ow, "argmax " + what)
    assert torch.equal(w.argmax(-1), ow.argmax(-1)), what  # (no row of these cases is near a tie: test_batch_regimes_host.py)


def _fresh_decoder(H, case, monkeypatch):
    """A new module = a new handle, which reads TTSDEC_OPTIONS."""
    if case.options:
        monkeypatch.setenv("TTSDEC_OPTIONS", case.options)
    else:
        monkeypatch.delenv("TTSDEC_OPTIONS", raising=False)
    dec = H.make_decoder(C.reduced_dims(), C.reduced_weights())
    dec.precision = case.prec
    eng = dec.engine(torch.device("cuda:0"))
    for opt in filter(None, case.options.split(",")):
        k, v = opt.split("=")
        assert eng.get_option(k) == int(v), opt
    return dec, eng


def _step_names(eng, mem):
    """The launches of one step, by name.  (Beside a step with two-role launches ttsdec_profile_step also times each role on
    its own - "... (alone)": measurements, no part of the step.)"""
    from torch_tts_amd import _lib

    return {n for n in eng.profile_step(mem.cuda(), 1, _lib.DROPOUT_OFF, None, 0) if not n.endswith("(alone)")}


# --------------------------------------------------------------------------
# A. decode step, Taco2ProdDecoderCell
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REGIME_EDGES + C.F32_QUERY_ROLE_EDGES + C.STANDALONE_64x8, ids=lambda c: c.id)
def test_decode_step_at_each_regime_edge_vs_oracle(H, case, monkeypatch):
    mem, masks, want = C.decode_inputs(case)
    dec, eng = _fresh_decoder(H, case, monkeypatch)
    got = H.run_decoder_with_masks(dec, mem, masks, max_steps=C.T_STEPS - 1)
    assert eng.precision() == case.prec
    names = _step_names(eng, mem)
    print(f"regime {case.id}: {case.regime}: launches {sorted(names)}")
    assert names == set(case.names), (case.id, sorted(names), sorted(case.names))
    _check_decode(H, case.id, got, want)
    again = H.run_decoder_with_masks(dec, mem, masks, max_steps=C.T_STEPS - 1)
    for n, a, b in zip("ysw", got, again):
        assert torch.equal(a, b), f"{case.id}: {n} differs between two identical calls"


def test_rows_do_not_interact_inside_the_97_to_128_regime(H, monkeypatch):
    """Exact fp32, B = 112 (two 64-row blocks, the second ragged): the memory and masks of every row but the first, the last
    and row 64 are replaced; those three rows must come out bit for bit as before (same batch, so the same tiles and K order)."""
    case = C.ISOLATION
    mem, masks, want = C.decode_inputs(case)
    dec, eng = _fresh_decoder(H, case, monkeypatch)
    got = H.run_decoder_with_masks(dec, mem, masks, max_steps=C.T_STEPS - 1)
    assert _step_names(eng, mem) == set(case.names)
    _check_decode(H, case.id + " (isolation)", got, want)
    keep = C.isolation_rows(case.B)
    dims = C.reduced_dims()
    mem2 = O.synthetic_memory(case.B, C.L_MEM, dims.d_ctx, lengths=[C.L_MEM - (b % 5) for b in range(case.B)], seed=31)
    masks2 = O.synthetic_masks(C.T_STEPS, case.B, dims.d_pre, seed=32)
    mem2[keep] = mem[keep]
    masks2[:, :, keep] = masks[:, :, keep]
    got2 = H.run_decoder_with_masks(dec, mem2, masks2, max_steps=C.T_STEPS - 1)
    assert not got2[3]
    others = [b for b in range(case.B) if b not in keep]
    for n, a, b in zip("ysw", got, got2):
        assert torch.equal(a[keep], b[keep]), f"{n}: rows {keep} changed with the other rows' inputs"
        assert not torch.equal(a[others], b[others]), n


# --------------------------------------------------------------------------
# B. Taco2DecoderCell above 95 utterances
# --------------------------------------------------------------------------
@pytest.mark.parametrize("B", C.TACO2_B)
@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_taco2_cell_standalone_lstm_tiles_vs_oracle(H, prec, B, monkeypatch):
    """config-rdh dims (K = 1536 for lstm_dec), 4 steps: B = 96 runs lstm_dec on launch_lstm's 64 x 8 tile (K over two waves),
    B = 129 on its 64 x 16 tile with a one-row last block."""
    monkeypatch.delenv("TTSDEC_OPTIONS", raising=False)
    wts, mem, m0, m1, want = C.taco2_inputs(B)
    dec = H.make_taco2_decoder(O.DecoderDims(**C.TACO2), wts)
    dec.precision = prec
    got = H.run_decoder_with_masks(dec, mem, H.flat_masks(m0, m1), max_steps=C.TACO2_T - 1)
    eng = dec.engine(torch.device("cuda:0"))
    assert eng.precision() == prec
    names = _step_names(eng, mem)
    print(f"regime taco2-{prec}-B{B}: launches {sorted(names)}")
    assert names == set(C.TACO2_NAMES), names  # lstm_dec is a launch of its own
    _check_decode(H, f"taco2-{prec}-B{B}", got, want)


# --------------------------------------------------------------------------
# C. Encoder2, the whole batch in one call
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoder(alphabet, d_emb, d_out):
    import torch_tts_amd as T

    wts = C.enc_small_weights(d_emb, d_out) if alphabet == C.ENC_ALPHABET else C.enc_lj_weights()
    enc = T.Encoder2(alphabet, dim_out=d_out, dim_emb=d_emb)
    missing, unexpected = enc.load_state_dict(wts, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    return enc.cuda().eval(), wts


def _run_encoder(enc, prec, ids, lens):
    enc.precision = prec
    try:
        with torch.no_grad():
            out = enc(ids.cuda(), lens)
        assert enc.use_hip and enc._engines.engines(), "the HIP path must have run"
        return out.cpu()
    finally:
        enc.precision = "f32"


def _assert_padding_is_zero(out, lens, what):
    pad = torch.arange(out.shape[1])[None, :] >= lens[:, None]
    assert not bool(out[pad].ne(0).any()), f"{what}: rows past an utterance's length must be exactly zero (rnn.py:126)"


@pytest.mark.parametrize("B", C.ENC_B)
@pytest.mark.parametrize("d_emb, d_out", C.ENC_SMALL_DIMS)
def test_encoder2_at_every_lstm_pair_tile_vs_oracle(H, d_emb, d_out, B):
    """Every row against the oracle, both precision settings, lengths that fill the id matrix and lengths that stop 3 short
    of it; twice the same bits; and the first row, the last and the first row of the last 64-row tile reproduce their bits when
    every other row's ids and length are rewritten."""
    enc, wts = _encoder(C.ENC_ALPHABET, d_emb, d_out)
    L = C.ENC_L
    keep = C.isolation_rows(B)
    for kind in ("full", "short"):
        l_max, lens, ids = C.enc_case(B, L, C.ENC_ALPHABET, kind)
        ref = O.encoder2(ids, lens, wts)
        # the other rows rewritten: other ids, other lengths (the same maximum or not: neither is an input of a kept row)
        lens2 = torch.randint(1, l_max + 1, (B,), generator=torch.Generator().manual_seed(400 + B))
        lens2[keep] = lens[keep]
        ids2 = C.enc_ids(B, L, lens2, C.ENC_ALPHABET, seed=500 + B)
        ids2[keep] = ids[keep]
        for prec in ("f32", "split_f16"):
            what = f"encoder2 E={d_emb} H={d_out // 2} B={B} {kind} {prec}"
            out = _run_encoder(enc, prec, ids, lens)
            assert out.shape == (B, l_max, d_out) == ref.shape, what
            print(f"regime {what}: max rel err {_rel(out, ref):.2e}")
            H.assert_close(out, ref, RTOL, ATOL, what)
            _assert_padding_is_zero(out, lens, what)
            assert torch.equal(out, _run_encoder(enc, prec, ids, lens)), what + ": two identical calls differ"
            out2 = _run_encoder(enc, prec, ids2, lens2)
            assert out2.shape == out.shape  # (row 0 keeps the maximum length)
            assert torch.equal(out[keep], out2[keep]), what + f": rows {keep} changed with the other rows' inputs"


@functools.lru_cache(maxsize=None)
def _lj_encoder_case(B, kind):
    """(lens, ids, sample, the oracle's memory of the sample)"""
    L = C.ENC_LJ_L
    l_max, lens, ids = C.enc_case(B, L, C.ENC_LJ[0], kind)
    import hip_helpers as Hh

    sample = sorted(set(Hh.sample_utterances(B, L, Hh.last_tile_rows(B * L, 64, 128), k_random=2)) | set(C.enc_forced_rows(B)))
    s = torch.tensor(sample)
    return l_max, lens, ids, sample, O.encoder2(ids[s], lens[s], C.enc_lj_weights())


@pytest.mark.parametrize("B", C.ENC_LJ_B)
@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_encoder2_ljspeech_dims_whole_batch_vs_oracle(H, prec, B):
    """LJSpeech dims (K = 256 deep recurrence), L = 22: 96 utterances run the BiLSTM on the 64 x 8 pair tile, 192 on the 64 x 16
    one (and put the fp32 convs on the 64 x 64 GEMM tile: 66 x 8 tiles >= 512).  The whole batch runs; a sample is compared."""
    enc, _ = _encoder(*C.ENC_LJ)
    for kind in ("full", "short"):
        l_max, lens, ids, sample, ref = _lj_encoder_case(B, kind)
        what = f"encoder2 LJSpeech dims B={B} {kind} {prec}"
        out = _run_encoder(enc, prec, ids, lens)
        assert out.shape == (B, l_max, C.ENC_LJ[2]) and ref.shape[1] == l_max, what
        print(f"regime {what}: utterances {sample}, lengths {lens[sample].tolist()}: max rel err {_rel(out[sample], ref):.2e}")
        H.assert_close(out[sample], ref, RTOL, ATOL, what)
        _assert_padding_is_zero(out, lens, what)


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_encoder2_whole_batch_agrees_with_its_64_row_slices(H, prec):
    """What a user's Tacotron.forward runs (192 texts in one call: the 64 x 16 pair tile) against what the rest of the suite
    and bench.py run (slices of 64: the 32-row tile).  Other tiles, other summation order: equal at the bar, not bitwise."""
    enc, _ = _encoder(*C.ENC_LJ)
    B = 192
    l_max, lens, ids, _, _ = _lj_encoder_case(B, "full")
    whole = _run_encoder(enc, prec, ids, lens)
    sliced = torch.zeros_like(whole)
    for i in range(0, B, 64):
        part = _run_encoder(enc, prec, ids[i : i + 64], lens[i : i + 64])
        assert part.shape[1] == int(lens[i : i + 64].max())
        sliced[i : i + 64, : part.shape[1]] = part
    print(f"regime encoder2 LJSpeech dims B=192 whole vs 3 x 64 {prec}: max rel err {_rel(whole, sliced):.2e}")
    H.assert_close(whole, sliced, RTOL, ATOL, f"whole batch vs slices ({prec})")
