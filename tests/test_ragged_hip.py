"""Batched synthesis on the GPU: the per-utterance stop rule (Decoder.forward_each / ttsdec_decode_each), the Postnet with lengths
(ttsdec_postnet_ragged) and Tacotron.synthesize, against the CPU oracle run once over each batch (ragged_cases.py; rows never
interact, so that run is every row's result alone) and, bit for bit, against the batch-global path on the same device."""
import pytest
import torch

import hip_helpers as H
import ragged_cases as R
import torch_tts_amd as T
from oracle import tacotron_oracle as O
from torch_tts_amd import _lib

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5  # test_hip_parity.py's
DEV = torch.device("cuda:0")
PRECS = ["f32", "split_f16"]


def _decoder(case, prec, thr=None, make=H.make_decoder, dropout="philox"):
    dec = make(case.dims, case.wts, stop_threshold=case.thr if thr is None else thr)
    dec.precision, dec.dropout_source, dec.dropout_seed = prec, dropout, R.PHILOX_SEED
    dec.max_decoder_steps = R.T  # every case ends by step T - 3; a decode that missed its stop ends here instead of never
    return dec


def _each(dec, mem, max_steps=0):
    with torch.no_grad():
        y, s, w, lengths, stopped = dec.forward_each(mem.to(DEV), None, max_steps)
    assert lengths.dtype == torch.int64 and stopped.dtype == torch.bool and lengths.is_cuda and stopped.is_cuda
    return y.cpu(), s.cpu(), w.cpu(), lengths.cpu(), stopped.cpu()


def _expected(case, thr, max_steps=0, rows=slice(None)):
    """(steps run, lengths in frames, stopped) of the per-utterance rule on the oracle's logits."""
    tb, _ = R.stop_steps(case.s[rows], thr)
    n = int(tb.max()) + 1 if not max_steps else min(int(tb.max()), max_steps) + 1
    assert n <= R.T
    stopped = tb < n
    return n, torch.where(stopped, (tb + 1) * case.dims.r, torch.full_like(tb, n * case.dims.r)), stopped


def _check_vs_oracle(out, case, thr, what, max_steps=0, rows=slice(None)):
    """lengths / stopped exactly; y, s, w of each row up to its length at RTOL / ATOL, attention argmax; zeros past it."""
    y, s, w, lengths, stopped = out
    r = case.dims.r
    n, want_len, want_stopped = _expected(case, thr, max_steps, rows)
    assert lengths.tolist() == want_len.tolist(), (what, lengths.tolist(), want_len.tolist())
    assert stopped.tolist() == want_stopped.tolist(), what
    nb = want_len.numel()
    assert y.shape == (nb, n * r, 80) and s.shape == (nb, n * r) and w.shape == (nb, n, R.L), (what, y.shape, s.shape, w.shape)
    live = torch.arange(n * r)[None, :] < want_len[:, None]          # [B, frames]
    live_w = torch.arange(n)[None, :] < (want_len // r)[:, None]     # [B, steps]
    assert not bool(y[~live].any()) and not bool(s[~live].any()) and not bool(w[~live_w].any()), f"{what}: not zero past a row's length"
    oy, os_, ow = case.y[rows, : n * r], case.s[rows].reshape(nb, -1)[:, : n * r], case.w[rows, :n]
    H.assert_close(y, oy * live[:, :, None], RTOL, ATOL, "y " + what)
    H.assert_close(s, os_ * live, RTOL, ATOL, "s " + what)
    H.assert_close(w, ow * live_w[:, :, None], RTOL, ATOL, "w " + what)
    H.assert_argmax(w[live_w], ow[live_w], "argmax " + what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("r,d_pre", R.DECODE_CASES)
def test_each_parity_with_the_oracle(r, d_pre, prec):
    case = R.prod_case(r, d_pre)
    out = _each(_decoder(case, prec), case.mem)
    tb, _ = R.stop_steps(case.s, case.thr)
    assert out[0].shape[1] == (int(tb.max()) + 1) * r
    _check_vs_oracle(out, case, case.thr, f"r={r} d_pre={d_pre} {prec}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("r,d_pre", R.DECODE_CASES)
def test_each_is_bitwise_the_batch_global_arithmetic(r, d_pre, prec):
    """No tolerance: every row's prefix equals the same rows of forward(max_steps = t_all), whose rule never fires in time
    (threshold -1e30 there); a second call repeats the first bit for bit."""
    case = R.prod_case(r, d_pre)
    for dropout in ("off", "philox"):
        dec = _decoder(case, prec, dropout=dropout)
        y, s, w, lengths, stopped = _each(dec, case.mem)
        # (the case's stop steps are those of the Philox draws; without dropout the rows stop elsewhere, some perhaps never)
        assert bool(stopped.all()) if dropout == "philox" else lengths.unique().numel() >= 2
        again = _each(dec, case.mem)
        for a, b in zip((y, s, w, lengths, stopped), again):
            assert torch.equal(a, b), dropout
        ref = _decoder(case, prec, thr=-1e30, dropout=dropout)
        with torch.no_grad():
            fy, fs, fw = (t.cpu() for t in ref(case.mem.to(DEV), None, None, w.shape[1] - 1))
        assert fy.shape == y.shape and fs.shape[:2] == s.shape and fw.shape == w.shape
        live = torch.arange(y.shape[1])[None, :] < lengths[:, None]
        live_w = torch.arange(w.shape[1])[None, :] < (lengths // r)[:, None]
        assert torch.equal(y[live], fy[live]) and torch.equal(s[live], fs[:, :, 0][live]) and torch.equal(w[live_w], fw[live_w]), dropout


@pytest.mark.parametrize("prec", PRECS)
def test_each_chunked_then_another_batch_size(prec):
    """chunk_steps = 4, unbounded: rows stop in at least three different chunks (ragged_cases.conditions), so the stop steps and
    the count of stopped rows have to survive t_begin > 0; the result is the unchunked one.  Then the same module on the first
    five rows: the count starts again at t_begin = 0, and the call ends at THEIR last stop."""
    case = R.prod_case(1, 128)
    whole = _each(_decoder(case, prec), case.mem)
    dec = _decoder(case, prec)
    dec.chunk_steps = 4
    chunked = _each(dec, case.mem)
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
    few = slice(0, 5)
    tb, _ = R.stop_steps(case.s, case.thr)
    assert int(tb[few].max()) < int(tb.max())
    _check_vs_oracle(_each(dec, case.mem[few]), case, case.thr, f"5 rows after 37, {prec}", rows=few)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("r,d_pre", R.DECODE_CASES)
def test_each_cap(r, d_pre, prec):
    """max_steps below the largest stop step, and a threshold one row never reaches in T steps: rows that did not fire report
    stopped == False and lengths == (max_steps + 1) * r."""
    case = R.prod_case(r, d_pre)
    tb, _ = R.stop_steps(case.s, case.thr)
    cap = int(tb.max()) - 1
    out = _each(_decoder(case, prec), case.mem, max_steps=cap)
    assert not bool(out[4].all()) and out[3][~out[4]].tolist() == [(cap + 1) * r] * int((~out[4]).sum())
    _check_vs_oracle(out, case, case.thr, f"cap {cap}", max_steps=cap)
    out = _each(_decoder(case, prec, thr=case.thr_cap), case.mem, max_steps=R.T - 1)
    assert not bool(out[4].all()) and out[0].shape[1] == R.T * r
    _check_vs_oracle(out, case, case.thr_cap, "cap T - 1", max_steps=R.T - 1)


@pytest.mark.parametrize("prec", PRECS)
def test_each_of_one_utterance_is_forward(prec):
    """B = 1: each == any, bit for bit.  (Row 0 of the Taco2 case: its Philox draws are keyed by row index 0 alone as in the batch,
    so the oracle's row 0 still applies - it stops at step 4.)"""
    case = R.taco2_case()
    tb, _ = R.stop_steps(case.s, case.thr)
    assert 2 <= int(tb[0]) < R.T - 2
    mem = case.mem[:1]
    dec = _decoder(case, prec, make=H.make_taco2_decoder)
    out = _each(dec, mem)
    y, s, w, lengths, stopped = out
    with torch.no_grad():
        fy, fs, fw = (t.cpu() for t in dec(mem.to(DEV), None, None, 0))
    assert bool(stopped.all()) and lengths.tolist() == [y.shape[1]] == [int(tb[0]) + 1]
    assert torch.equal(y, fy) and torch.equal(s, fs[:, :, 0]) and torch.equal(w, fw)
    _check_vs_oracle(out, case, case.thr, f"B = 1 {prec}", rows=slice(0, 1))


_SEQUENCES = [
    {"overlap": 0}, {"overlap": 1}, {"overlap": 2}, {"head_proj": 0}, {"head_proj": 1}, {"proj_regw": 0}, {"proj_regw": 1},
    {"graph": 0}, {"graph": 1}, {"query_role": 0}, {"query_role": 1, "overlap": 2},
    {"head_proj": 1, "graph": 0}, {"overlap": 0, "head_proj": 0, "graph": 0},
]


@pytest.mark.parametrize("prec", PRECS)
def test_each_under_every_launch_sequence(prec):
    """The parity test at (r, d_pre) = (1, 128) under each launch sequence the options select, then the Taco2 cell, then a
    PreNet width outside the frame kernel's shapes.  The rule is evaluated at two sites:
      * phase F of the frame body (frame_body.h), for every shape the frame kernel covers (d_mel = 80, PreNet hidden 128 / 256) -
        as the stand-alone frame kernel (overlap = 0), as the frame role of the two-role launch (overlap = 1, 2), behind the
        projection role of the same launch (head_proj = 1), and as the end-of-call launch that finishes the call's last step (every
        sequence; with graph = 1 after a replayed graph, with graph = 0 after serial launches).  proj_regw and query_role change
        what feeds phase F and what runs beside it, not the site.  Both cells reach it.
      * the EPI_PROJ epilogue of the row GEMM (decode_kernels.hip), for every other shape: here d_pre = 64, r = 2.
    There is no third site: the projection roles (PROJ_STEP / PROJ_HEAD / PROJ_FINAL) write partial sums only."""
    case = R.prod_case(1, 128)
    for opt in _SEQUENCES:
        dec = _decoder(case, prec)
        eng = dec.engine(DEV)
        for k, v in opt.items():
            eng.set_option(k, v)
            assert eng.get_option(k) == v
        _check_vs_oracle(_each(dec, case.mem), case, case.thr, f"{prec} {opt}")
    t2 = R.taco2_case()
    _check_vs_oracle(_each(_decoder(t2, prec, make=H.make_taco2_decoder), t2.mem), t2, t2.thr, f"taco2 {prec}")
    dec = _decoder(t2, prec, make=H.make_taco2_decoder)
    dec.engine(DEV).set_option("overlap", 0)
    _check_vs_oracle(_each(dec, t2.mem), t2, t2.thr, f"taco2 overlap=0 {prec}")
    gp = R.gemm_proj_case()
    for opt in ({}, {"graph": 0}):
        dec = _decoder(gp, prec)
        for k, v in opt.items():
            dec.engine(DEV).set_option(k, v)
        _check_vs_oracle(_each(dec, gp.mem), gp, gp.thr, f"row-GEMM projection {prec} {opt}")


def test_decode_each_argument_rejection():
    case = R.prod_case(1, 128)
    eng = _decoder(case, "f32").engine(DEV)
    lib, h = _lib.load(), eng._h
    B, n = 3, 4
    mem = case.mem[:B].to(DEV).contiguous()
    y = torch.empty(B, n, 80, device=DEV); s = torch.empty(B, n, device=DEV); w = torch.empty(B, n, R.L, device=DEV)
    ss = torch.empty(B, dtype=torch.int32, device=DEV)
    t_out = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = eng.step_workspace(B, R.L)
    teacher = torch.zeros(B, n, 80, device=DEV)
    flags = torch.ones(n, dtype=torch.uint8, device=DEV)

    def call(t_begin=0, teacher=None, stop_steps=ss):
        return lib.ttsdec_decode_each(h, mem.data_ptr(), B, R.L, t_begin, n, n, -2.0, _lib.DROPOUT_OFF, None, 0,
                                      None if teacher is None else teacher.data_ptr(), n, flags.data_ptr(), y.data_ptr(), s.data_ptr(),
                                      w.data_ptr(), None if stop_steps is None else stop_steps.data_ptr(), t_out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), None)

    assert call(teacher=teacher) == _lib.ERR_INVALID_ARG
    assert call(stop_steps=None) == _lib.ERR_INVALID_ARG
    assert call(t_begin=1) == _lib.ERR_INVALID_ARG
    assert call() == 0
    torch.cuda.synchronize()
    assert t_out.tolist()[0] in range(1, n + 1)
    # the per-utterance mode is not reachable through ttsdec_decode, whose check_stop is a switch: 2 is the batch-global rule there
    assert lib.ttsdec_decode(h, mem.data_ptr(), B, R.L, 0, n, n, -2.0, 2, _lib.DROPOUT_OFF, None, 0, None, 0, None, y.data_ptr(),
                             s.data_ptr(), w.data_ptr(), t_out.data_ptr(), ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    # more utterances than the tail kernel's grid takes: said before any decode step runs, not after the last
    with pytest.raises(ValueError, match="65535"), torch.no_grad():
        _decoder(case, "f32").forward_each(torch.zeros(65536, 1, case.dims.d_ctx, device=DEV), None)
    # ttsdec_zero_tail: no lengths, entries that overlap
    assert lib.ttsdec_zero_tail(h, y.data_ptr(), None, B, n, n * 80, 80, 1, None) == _lib.ERR_INVALID_ARG
    assert lib.ttsdec_zero_tail(h, y.data_ptr(), ss.data_ptr(), B, n, n * 80 - 1, 80, 1, None) == _lib.ERR_INVALID_ARG


# --------------------------------------------------------------------------
# the Postnet with lengths
# --------------------------------------------------------------------------
POST_LENGTHS = [40, 17, 2, 0]  # 2 and 0: shorter than the conv's half width
_POST_TOL = {"f32": (RTOL, ATOL), "split_f16": (RTOL, ATOL), "bf16": (3e-2, 3e-2)}  # test_postnet_low_precision_modes_vs_oracle's
_POST = {}


def _postnet_case(kind):
    """(weights, y, per-row oracle results), computed once per Postnet type."""
    if kind not in _POST:
        pw = O.random_postnet_weights(80, 64, 3, seed=9) if kind == "mel" else O.random_postnet2_weights(80, 64, 3, seed=4)
        y = torch.randn(4, 40, 80, generator=torch.Generator().manual_seed(2))
        f = O.mel_postnet if kind == "mel" else O.mel_postnet2
        _POST[kind] = (pw, y, [f(y[b : b + 1, :n], pw, 3)[0] if n else y[b, :0] for b, n in enumerate(POST_LENGTHS)])
    return _POST[kind]


def _make_postnet(kind, pw, hidden=64):
    return H.make_postnet(80, hidden, 3, pw) if kind == "mel" else H.make_postnet2(80, hidden, 3, pw)


@pytest.mark.parametrize("mode", ["f32", "split_f16", "bf16"])
@pytest.mark.parametrize("kind", ["mel", "mel2"])
def test_postnet_with_lengths_vs_each_row_alone(kind, mode):
    pw, y, alone = _postnet_case(kind)
    pn = _make_postnet(kind, pw)
    pn.precision = mode
    rtol, atol = _POST_TOL[mode]
    garbage = y.clone()
    for b, n in enumerate(POST_LENGTHS):
        garbage[b, n:] = 1e3
    with torch.no_grad():
        out = pn(y.to(DEV), lengths=torch.tensor(POST_LENGTHS, device=DEV)).cpu()
        out_g = pn(garbage.to(DEV), lengths=POST_LENGTHS).cpu()  # (a host list is taken too)
    assert torch.equal(out, out_g), "what the input holds past a row's length changed the result"
    for b, n in enumerate(POST_LENGTHS):
        assert not bool(out[b, n:].any()), f"row {b}: not zero past its length"
        if n:
            err = float((out[b, :n] - alone[b]).abs().max())
            print(f"{kind} {mode} row {b} ({n} frames): max abs err {err:.3e}")
            H.assert_close(out[b, :n], alone[b], rtol, atol, f"{kind} {mode} row {b}")


@pytest.mark.parametrize("mode", ["f32", "split_f16", "bf16"])
@pytest.mark.parametrize("kind", ["mel", "mel2"])
def test_postnet_without_lengths_is_unchanged_and_full_lengths_agree(kind, mode):
    pw, y, _ = _postnet_case(kind)
    pn = _make_postnet(kind, pw)
    pn.precision = mode
    rtol, atol = _POST_TOL[mode]
    with torch.no_grad():
        plain = pn(y.to(DEV))
        assert torch.equal(pn(y.to(DEV), lengths=None), plain)
        full = pn(y.to(DEV), lengths=torch.full((4,), 40, device=DEV))
    H.assert_close(full.cpu(), plain.cpu(), rtol, atol, f"{kind} {mode} lengths = T")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_postnet_with_lengths_on_the_256_wide_conv_kernel(mode, monkeypatch):
    """The ragged path keeps conv256 for the hidden -> hidden layers (the mask pass runs between the same launches): hidden 512,
    4 x 128 frames under TTSDEC_CONV256_FORCE, one length that ends inside one of that schedule's row tiles and one that ends
    exactly on a tile edge.  (Like the existing forced-conv256 tests, this restates the library's schedule - hip_helpers
    .conv256_schedule - and trusts the switch: the library has no query for which conv kernel a call took, so that the 256-wide
    kernel really ran is not asserted here.  With the shared tile instead the test would still check the same results.)"""
    B, T_ = 4, 128
    sch = H.conv256_schedule(B * T_, H.device_cus(), elem_bytes=4 if mode == "f32" else 2, force=True)
    assert sch is not None and sch["full"] == 0 and sch["h"] >= 8
    h = sch["h"]  # rows per tile, from flattened row 0
    on_edge = next(n for n in range(T_ - 1, 8, -1) if (1 * T_ + n) % h == 0)
    inside = next(n for n in range(T_ // 2, T_) if (2 * T_ + n) % h not in (0, h - 1))
    lengths = [T_, on_edge, inside, 5]
    pw = O.random_postnet_weights(80, 512, 3, seed=9)
    y = torch.randn(B, T_, 80, generator=torch.Generator().manual_seed(3))
    for b, n in enumerate(lengths):
        y[b, n:] = 1e3
    pn = H.make_postnet(80, 512, 3, pw)
    pn.precision = mode
    monkeypatch.setenv("TTSDEC_CONV256_FORCE", "1")
    with torch.no_grad():
        out = pn(y.to(DEV), lengths=lengths).cpu()
    rtol, atol = _POST_TOL[mode]
    print(f"conv256 {mode}: tiles of {h} rows, lengths {lengths}")
    for b, n in enumerate(lengths):
        assert not bool(out[b, n:].any())
        H.assert_close(out[b, :n], O.mel_postnet(y[b : b + 1, :n], pw, 3)[0], rtol, atol, f"conv256 {mode} row {b}")


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
def test_synthesize_end_to_end():
    """Tacotron.synthesize on test_tacotron_forward_glue's config, 5 texts: every utterance's y_post up to its length is, within the
    Postnet's tolerance, what the same model gives for that utterance ALONE (a batch of one) run to its own stop step; then
    waveforms.

    One deviation from "alone", on purpose: the batch of one is given the utterance's row of token ids as it stands in the batch,
    all 21 columns with its padding zeros, and its own length - not the ids cut to that length.  The reference's Encoder2
    convolves over the padded columns (its convs take no lengths), so the memory of a text depends on the width it is padded to -
    by 1e-3, measured here - in the reference and in this library alike; cutting the ids would compare two different memories
    and say nothing about the decoder and the Postnet, which this test is about.  Everything after the encoder's convs IS the
    utterance alone: the encoder returns lengths[b] memory rows (19 for a text of 19, where the batch holds 21 with two zero
    rows), the decoder runs B = 1, and the Postnet sees n frames instead of T.  (Dropout off: both generators key their draws by
    the row's index in the batch.)  The threshold is chosen like ragged_cases': in the middle of a gap of the model's own stop
    logits, at least 1e-3 from each, fc_stop scaled by a power of two to open the gaps."""
    from test_griffinlim_host import frontend

    cfg = {
        "text": {"alphabet": "abcdefghijklmnopqrstuvwxyz '.,?!"},
        "audio": {"num_mels": 80},
        "model": {
            "encoder": {"dim_emb": 64, "dim_out": 512},
            "decoder": {"type": "tacotron2prod", "r": 1, "dim_pre": 256, "dim_att": 1024, "dim_rnn": [1024, 1024]},
            "postnet": {"type": "tacotron2", "dim_hidden": 512, "num_layers": 3},
        },
    }
    torch.manual_seed(0)
    model = T.build_tacotron(cfg).cuda().eval()
    model.decoder.dropout_source = "off"
    lens = [21, 19, 17, 20, 18]  # (all longer than the steps run: the attention cannot reach a text's end, where padding would show)
    lens_t = torch.tensor(lens).cuda()
    N = 14
    model.decoder.stop_threshold = -1e30
    thr = scale = None
    for seed in range(24):  # the first 5 texts whose stop logits a threshold separates (a random model's often run side by side)
        ids = torch.randint(1, 30, (5, 21), generator=torch.Generator().manual_seed(seed))
        for b, n in enumerate(lens):
            ids[b, n:] = 0
        ids = ids.cuda()
        with torch.no_grad():
            s0 = model(ids, lens_t, max_steps=N - 1)[2][:, :, 0].cpu()  # [5, N] stop logits, no rule
        for sc in (8.0, -8.0, 64.0, -64.0):
            for t in R._thresholds(s0 * sc):
                tb, _ = R.stop_steps((s0 * sc)[:, :, None], t)
                # (at least 2 frames each: an utterance of one frame has no samples)
                if int(tb.min()) >= 1 and int(tb.max()) <= N - 2 and tb.unique().numel() >= 3:
                    thr, scale = t, sc
                    break
            if thr is not None:
                break
        if thr is not None:
            break
    assert thr is not None, "no texts and threshold separate the 5 utterances' stop steps; change the model's seed"
    with torch.no_grad():
        model.decoder.fc_stop.weight.mul_(scale)
        model.decoder.fc_stop.bias.mul_(scale)
    model.decoder.invalidate()  # (an in-place edit of a parameter: the packed blob is stale)
    model.decoder.stop_threshold = thr
    tb, _ = R.stop_steps((s0 * scale)[:, :, None], thr)
    with torch.no_grad():
        y, y_post, s, out = model.synthesize(ids, lens_t)
    lengths = out["lengths"]
    assert lengths.tolist() == (tb + 1).tolist() and bool(out["stopped"].all())
    Tn = int(tb.max()) + 1
    assert y.shape == (5, Tn, 80) and y_post.shape == y.shape and s.shape == (5, Tn, 1) and out["w"].shape == (5, Tn, 21)
    for b, n in enumerate(lengths.tolist()):
        assert not bool(y_post[b, n:].any()) and not bool(y[b, n:].any())
        model.decoder.stop_threshold = -1e30
        with torch.no_grad():
            _, yp1, _, _ = model(ids[b : b + 1], lens_t[b : b + 1], max_steps=n - 1)
        assert yp1.shape == (1, n, 80)
        H.assert_close(y_post[b, :n].cpu(), yp1[0].cpu(), RTOL, ATOL, f"utterance {b} alone")
    fe = frontend(device=DEV)
    wave = T.audio.synth_audio_native(y_post, fe, lengths=lengths, generator=torch.Generator().manual_seed(1))
    hop = fe.config.hop_length
    assert wave.shape == (5, T.audio.wave_samples(Tn, hop)) and bool(torch.isfinite(wave).all())
    for b, n in enumerate(lengths.tolist()):
        m = T.audio.wave_samples(n, hop)
        assert float(wave[b, :m].abs().max()) > 0 and not bool(wave[b, m:].any())
