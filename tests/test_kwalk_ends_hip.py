"""The three ends of gemm_tile's K walk (csrc/gemm_tile.h) - the prologue that puts min(nk, S-1) tiles in flight, the gate in
front of a segment another role produces, and the peeled tail that issues nothing and waits with descending counts - at every
walk length and gate position at which they take another path, against the CPU oracle.

  A. Walk length around the ring depth.  ttsdec_postnet at hidden widths whose conv GEMMs walk 1, 2, S-2, S-1, S and S+1 K tiles
     on each of the three tiles these shapes run on (K = 5 * hidden):
         exact fp32   32 x 32 tile, K over four waves: 128 k per tile, S = 4    hidden  8 16 32 48 64 72 96 112 -> 1 1 2 2 3 3 4 5 tiles
         split-fp16   64 x 64 tile:                     64 k per tile, S = 4    ->                                  1 2 3 4 5 6 8 9
         bf16         64 x 64 tile:                     64 k per tile, S = 5    ->                                  1 2 3 4 5 6 8 9
     (the first conv walks K = 400 and the final projection K = hidden beside them).  A tail that waits one tile too few reads a
     stage whose DMA has not landed (stale or half-written operands: errors of O(1)); a prologue that issues past a short walk
     overwrites a tile not yet read.  Utterances of 1, 2 and 5 frames: every row is at an utterance edge, so the per-row k
     window (conv padding) path runs on every tile.
  B. Position of the gated segment: the Taco2Prod decode step, 18 steps (the captured-graph path), at dims that put the first
     tile of the gated segment inside the prologue tiles, exactly at tile S-1, behind it, make it one tile long, and make the
     segment lengths no multiples of the K tile (40, 48, 56) - one batch size per regime of DESIGN.md section 6's table.
     Two identical calls and the graph=0 path must give the same bits; overlap=0 (no gate at all) must agree within the bar.
  C. Gate closed (B = 64) and open (B = 256) on arrival at LJSpeech dims: no range_err / gave_up bit in T_out.
  D. Dead launches: a 40-step call whose stop rule fires at step 2, and a call whose n_steps ends inside a graph replay - the
     launches past the end issue their prologue, drain it and write nothing.

The bar is the project's: 1e-4 relative with a 1e-5 floor against the oracle, attention argmax equal; bf16 against the bf16
emulation of tests/hip_helpers.py at the bound the existing Postnet tests use."""
import faulthandler
import functools

import pytest
import torch

import batch_regime_cases as C
from oracle import tacotron_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = C.RTOL, C.ATOL
WALL_CLOCK_LIMIT_S = 120  # a call that hangs ends the process with a traceback instead of the session's time limit


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import hip_helpers

    return hip_helpers


def _rel(a, b):
    return float(((a - b).abs() / (ATOL / RTOL + b.abs())).max())


# --------------------------------------------------------------------------
# A. walk length around the ring depth
# --------------------------------------------------------------------------
POSTNET_HIDDEN = (8, 16, 32, 48, 64, 72, 96, 112)


# (tests/test_kwalk_ends_host.py checks on the CPU that these widths give every walk length on the tiles the dispatcher picks)
@pytest.mark.parametrize("hidden", POSTNET_HIDDEN)
def test_postnet_walks_of_every_length_around_the_ring_depth(H, hidden):
    pw = O.random_postnet_weights(80, hidden, 3, seed=9)
    pn = H.make_postnet(80, hidden, 3, pw)
    for T in (1, 2, 5):
        y = torch.randn(3, T, 80, generator=torch.Generator().manual_seed(100 + T))
        ref = O.mel_postnet(y, pw, 3)
        emu = H.postnet_bf16_emulation(y, pw, 3)
        for mode in ("f32", "split_f16", "bf16"):
            pn.precision = mode
            with torch.no_grad():
                out = pn(y.cuda()).cpu()
                again = pn(y.cuda()).cpu()
            what = f"postnet hidden={hidden} T={T} {mode}"
            assert torch.equal(out, again), what + ": two identical calls differ"
            if mode == "bf16":
                err = float((out - emu).abs().max())
                print(f"{what}: max abs err vs bf16 emulation {err:.3e}")
                assert err < 8e-3, (what, err)
            else:
                print(f"{what}: max rel err {_rel(out, ref):.2e}")
                H.assert_close(out, ref, RTOL, ATOL, what)


# --------------------------------------------------------------------------
# B. position of the gated segment
# --------------------------------------------------------------------------
# lstm_att walks [ctx | h_att | x_pre] with x_pre (d_pre wide) gated, lstm_dec [h_att | h_dec | ctx] with ctx gated; the lean
# tiles have 32 k per tile (the 32-row fp32 one 64) and S = 5, the stand-alone small tile 128 k and S = 4.
GATE_DIMS = {
    "inside-prologue": dict(d_mel=80, d_pre=128, d_ctx=32, h_att=32, h_dec=64),   # gate at tile 2 (lstm_att), 3 (lstm_dec)
    "at-S-1": dict(d_mel=80, d_pre=128, d_ctx=64, h_att=64, h_dec=64),            # gate at tile 4 = S - 1 in both
    "behind": C.REDUCED,                                                          # gate at tile 6 / 10
    "one-tile": dict(d_mel=80, d_pre=32, d_ctx=32, h_att=96, h_dec=64),           # the gated segment is one tile in both
    "ragged": dict(d_mel=80, d_pre=128, d_ctx=40, h_att=48, h_dec=56),            # no segment a multiple of the K tile
}
GATE_B = (3, 40, 100, 150, 200, 257)  # one per regime of DESIGN.md section 6
T_STEPS, L_MEM = C.T_STEPS, C.L_MEM


@functools.lru_cache(maxsize=None)
def _gate_case(name, B):
    dims = O.DecoderDims(**GATE_DIMS[name])
    wts = O.random_decoder_weights(dims, seed=C.REDUCED_WEIGHT_SEED, nonzero_init_state=True)
    mem = O.synthetic_memory(B, L_MEM, dims.d_ctx, lengths=[L_MEM] * (B - 2) + [4, 1], seed=7)
    masks = O.synthetic_masks(T_STEPS, B, dims.d_pre, seed=9)
    return dims, wts, mem, masks, O.decode(wts, dims, mem, max_steps=T_STEPS - 1, masks=masks)


def _decoder(H, dims, wts, prec, options, monkeypatch, stop_threshold=-2.0):
    """A new module = a new handle, which reads TTSDEC_OPTIONS."""
    with monkeypatch.context() as mp:
        if options:
            mp.setenv("TTSDEC_OPTIONS", options)
        else:
            mp.delenv("TTSDEC_OPTIONS", raising=False)
        dec = H.make_decoder(dims, wts, stop_threshold=stop_threshold)
        dec.precision = prec
        eng = dec.engine(torch.device("cuda:0"))
        for opt in filter(None, options.split(",")):
            k, v = opt.split("=")
            assert eng.get_option(k) == int(v), opt
    return dec


@pytest.mark.parametrize("B", GATE_B)
@pytest.mark.parametrize("name", sorted(GATE_DIMS))
def test_gated_segment_at_every_position_vs_oracle(H, name, B, monkeypatch):
    dims, wts, mem, masks, (oy, os_, ow) = _gate_case(name, B)
    gap = C.top2_gap(ow)
    for prec in ("f32", "split_f16"):
        what = f"gate {name} B={B} {prec}"
        dec = _decoder(H, dims, wts, prec, "", monkeypatch)
        y, s, w, fired = H.run_decoder_with_masks(dec, mem, masks, max_steps=T_STEPS - 1)
        assert not fired and y.shape == oy.shape and w.shape == ow.shape, what
        print(f"{what}: max rel err  y {_rel(y, oy):.2e}  s {_rel(s, os_):.2e}  w {_rel(w, ow):.2e}  (oracle top-2 gap {gap:.1e})")
        H.assert_close(y, oy, RTOL, ATOL, "y " + what)
        H.assert_close(s, os_, RTOL, ATOL, "s " + what)
        H.assert_close(w, ow, RTOL, ATOL, "w " + what)
        H.assert_argmax(w, ow, "argmax " + what)
        again = H.run_decoder_with_masks(dec, mem, masks, max_steps=T_STEPS - 1)
        for n, a, b in zip("ysw", (y, s, w), again):
            assert torch.equal(a, b), f"{what}: {n} differs between two identical calls"
        serial = H.run_decoder_with_masks(_decoder(H, dims, wts, prec, "graph=0", monkeypatch), mem, masks, max_steps=T_STEPS - 1)
        for n, a, b in zip("ysw", (y, s, w), serial):
            assert torch.equal(a, b), f"{what}: {n} differs between the captured graph and graph=0"
        y0, s0, w0, fired0 = H.run_decoder_with_masks(_decoder(H, dims, wts, prec, "overlap=0", monkeypatch), mem, masks, max_steps=T_STEPS - 1)
        assert not fired0, what
        H.assert_close(y0, y, RTOL, ATOL, "y overlap=0 vs default, " + what)
        H.assert_close(s0, s, RTOL, ATOL, "s overlap=0 vs default, " + what)
        H.assert_close(w0, w, RTOL, ATOL, "w overlap=0 vs default, " + what)
        H.assert_argmax(w0, ow, "argmax overlap=0 " + what)


# --------------------------------------------------------------------------
# C. gate closed and gate open on arrival
# --------------------------------------------------------------------------
@pytest.mark.parametrize("B", (64, 256))
def test_ljspeech_dims_gate_closed_and_open_on_arrival(H, B, monkeypatch):
    """At B = 64 the LSTM role reaches its gate before the producers have signalled (the blocking poll and its barrier run),
    at B = 256 after (the gate is open on arrival)."""
    dims = O.DecoderDims()
    wts = O.random_decoder_weights(dims, seed=42, nonzero_init_state=True)
    L, T = 33, 6
    mem = O.synthetic_memory(B, L, dims.d_ctx, seed=1234)
    masks = O.synthetic_masks(T, B, dims.d_pre, seed=123)
    oy, os_, ow = O.decode(wts, dims, mem, max_steps=T - 1, masks=masks)
    for prec in ("f32", "split_f16"):
        what = f"LJSpeech dims B={B} {prec}"
        dec = _decoder(H, dims, wts, prec, "", monkeypatch)
        y, s, w, flags = _decode_raw(dec, mem, masks, T)
        assert flags == [T, 0], (what, flags)  # all steps done; no stop, no range_err (bit 1), no gave_up (bit 2)
        s = s.unsqueeze(2)
        print(f"{what}: max rel err  y {_rel(y, oy):.2e}  s {_rel(s, os_):.2e}  w {_rel(w, ow):.2e}")
        H.assert_close(y, oy, RTOL, ATOL, "y " + what)
        H.assert_close(s, os_, RTOL, ATOL, "s " + what)
        H.assert_close(w, ow, RTOL, ATOL, "w " + what)
        H.assert_argmax(w, ow, "argmax " + what)


# --------------------------------------------------------------------------
# D. dead launches
# --------------------------------------------------------------------------
def _decode_raw(dec, mem, masks, n_steps, check_stop=True):
    """ttsdec_decode into ZEROED outputs, under a wall-clock limit: (y, s, w, T_out) with everything the call did not write 0."""
    from torch_tts_amd import _lib

    dev = torch.device("cuda:0")
    B, L, _ = mem.shape
    eng = dec.engine(dev)
    y = torch.zeros(B, n_steps, dec.dim_mel, device=dev)
    s = torch.zeros(B, n_steps, device=dev)
    w = torch.zeros(B, n_steps, L, device=dev)
    t_out = torch.zeros(2, dtype=torch.int32, device=dev)
    faulthandler.dump_traceback_later(WALL_CLOCK_LIMIT_S, exit=True)
    try:
        eng.decode(mem.to(dev), t_begin=0, n_steps=n_steps, stop_threshold=float(dec.stop_threshold), check_stop=check_stop,
                   dropout_mode=_lib.DROPOUT_MASKS, masks=masks[:n_steps].to(dev).contiguous(), seed=0, teacher=None, teacher_flags=None,
                   y=y, s=s, w=w, t_out=t_out)
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()
    return y.cpu(), s.cpu(), w.cpu(), t_out.tolist()


DEAD_B, DEAD_T = 100, 40  # 40 steps = one whole graph replay of 30 slots and 10 of the next


@functools.lru_cache(maxsize=None)
def _stop_at_step_2():
    """(weights, memory, masks, threshold): the batch-global stop rule fires first at step 2 - the batch minimum of the stop
    logit at step 2 lies at least 2e-2 below those of steps 0 and 1 (two hundred times the bar), the threshold half-way between.
    Chosen on the oracle: the first weight seed (and sign of fc_stop) whose model has such a step.  With the suite's seed 21 the
    initial state gives step 0 the widest spread of the logit, so its extremes are at step 0."""
    dims = C.reduced_dims()
    mem = O.synthetic_memory(DEAD_B, L_MEM, dims.d_ctx, lengths=[L_MEM] * (DEAD_B - 2) + [4, 1], seed=7)
    masks = O.synthetic_masks(DEAD_T, DEAD_B, dims.d_pre, seed=9)
    for seed in range(C.REDUCED_WEIGHT_SEED, C.REDUCED_WEIGHT_SEED + 20):
        base = O.random_decoder_weights(dims, seed=seed, nonzero_init_state=True)
        for sign in (1.0, -1.0):
            wts = {k: (v * sign if "fc_stop" in k else v) for k, v in base.items()}
            _, s3, _ = O.decode(wts, dims, mem, max_steps=2, masks=masks)
            m = s3.reshape(DEAD_B, 3).amin(dim=0)
            if m[2] < min(m[0], m[1]) - 2e-2:
                return wts, mem, masks, float((m[2] + min(m[0], m[1])) / 2)
    raise AssertionError("no model whose stop logit has its first record minimum at step 2")


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_call_whose_stop_rule_fires_at_step_2_of_40(H, prec, monkeypatch):
    dims = C.reduced_dims()
    wts, mem, masks, thr = _stop_at_step_2()
    oy, os_, ow = O.decode(wts, dims, mem, max_steps=DEAD_T - 1, stop_threshold=thr, masks=masks)
    assert oy.shape[1] == 3  # steps 0, 1, 2
    got = {}
    for options in ("", "graph=0"):
        dec = _decoder(H, dims, wts, prec, options, monkeypatch, stop_threshold=thr)
        y, s, w, flags = _decode_raw(dec, mem, masks, DEAD_T)
        assert flags == [3, 1], (prec, options, flags)  # three steps produced, the stop rule fired, no other bit
        H.assert_close(y[:, :3], oy, RTOL, ATOL, f"y ({prec} {options})")
        H.assert_close(s[:, :3].unsqueeze(2), os_, RTOL, ATOL, f"s ({prec} {options})")
        H.assert_close(w[:, :3], ow, RTOL, ATOL, f"w ({prec} {options})")
        H.assert_argmax(w[:, :3], ow, f"argmax ({prec} {options})")
        got[options] = (y, s, w)
    for n, a, b in zip("ysw", got[""], got["graph=0"]):
        assert torch.equal(a, b), f"{n}: the captured graph's 37 dead steps and graph=0 left different outputs ({prec})"


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_call_whose_steps_end_inside_a_graph_replay(H, prec, monkeypatch):
    dims = C.reduced_dims()
    mem, _, _ = C.reduced_inputs(DEAD_B, 7, 9)
    masks = O.synthetic_masks(DEAD_T, DEAD_B, dims.d_pre, seed=9)
    oy, os_, ow = O.decode(C.reduced_weights(), dims, mem, max_steps=DEAD_T - 1, masks=masks)
    assert oy.shape[1] == DEAD_T
    got = {}
    for options in ("", "graph=0"):
        dec = _decoder(H, dims, C.reduced_weights(), prec, options, monkeypatch)
        y, s, w, flags = _decode_raw(dec, mem, masks, DEAD_T)
        assert flags == [DEAD_T, 0], (prec, options, flags)
        H.assert_close(y, oy, RTOL, ATOL, f"y ({prec} {options})")
        H.assert_close(s.unsqueeze(2), os_, RTOL, ATOL, f"s ({prec} {options})")
        H.assert_close(w, ow, RTOL, ATOL, f"w ({prec} {options})")
        H.assert_argmax(w, ow, f"argmax ({prec} {options})")
        got[options] = (y, s, w)
    for n, a, b in zip("ysw", got[""], got["graph=0"]):
        assert torch.equal(a, b), f"{n}: two replays (20 dead slots in the second) and graph=0 left different outputs ({prec})"
