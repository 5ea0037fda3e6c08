"""The style encoders' HIP path (csrc/style.hip through torch-tts_amd/style.py) on the GPU.  The oracle is always the module's own
``_stock_forward`` in fp64 on the CPU, from the same fp32 weights and inputs - never the HIP path, never torch ops on the GPU.  The
bar is the project's RTOL 1e-4 / ATOL 1e-5; beside every HIP error the same stock forward in fp32 on the CPU is measured against
the oracle and printed, so the margin is on record (tests/test_style_host.py pins that one below a quarter of the bar for the
fixture's inputs).

Batch independence, bit for bit, is tested for lengths >= 2^K frames (K conv stages).  With zero padding a row of a batch and the
same utterance alone then agree exactly: the last LSTM step t' = len // 2^K - 1 reads input frames up to 2^K t' + 2^K - 1 <= len - 1
only, at every stage, so neither run's result touches anything beyond the utterance's end, and the k-order of every output is
fixed (the conv tiles are picked from the channel counts alone).  Below 2^K frames the clipped single step DOES read beyond the end,
where the batch holds relu(bn(bias)) from the padded frames of the stage before and the lone run holds the conv's zero padding:
the reference differs between the two in the same way (its convs are not masked either), so those lengths are checked against the
oracle, not against the lone run.  (Also outside the claim: batches that change the tile of the input-projection GEMM - 4096 rows
B * T' - or of the LSTM kernel - 96 rows.)"""
import copy
import functools

import pytest
import torch

import torch_tts_amd as T
from style_corner_cases import randomize
from test_style_host import CASES, _config, bar_ratio, case_inputs, make_module, stock_outputs
from torch_tts_amd import style as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RAGGED = (1, 63, 64, 127, 128)  # with T itself: one step by the clip, the last length of one step, the first of two, ...


def lengths_for(B, T_):
    pool = [T_] + [n for n in RAGGED if n <= T_]
    return torch.tensor([pool[b % len(pool)] for b in range(B)])


def padded_input(B, T_, n_mels, lengths, seed, garbage=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T_, n_mels, generator=g)
    if lengths is not None and not garbage:
        for b, n in enumerate(lengths.tolist()):
            x[b, n:] = 0
    return x


def hip_outputs(m_dev, x, lengths, eps=None):
    """{"enc_out", "x", "kl"} of ONE call of the HIP path; fails if the module would take the stock path."""
    xd = x.to(DEV)
    with torch.no_grad():
        assert m_dev._hip_ok(xd)
        enc_out, xo, kl = m_dev._hip_forward(xd, lengths, None if eps is None else eps.reshape(x.shape[0], -1).to(DEV).contiguous())
    out = {"enc_out": enc_out}
    if xo is not None:
        out["x"] = xo
    if kl is not None:
        out["kl"] = kl
    return out


def check(tag, m_cpu, x, lengths, eps, hip=None, m_dev=None):
    """HIP against the fp64 oracle, the fp32 CPU error printed beside it; returns the HIP outputs."""
    m_dev = m_dev if m_dev is not None else copy.deepcopy(m_cpu).to(DEV)
    hip = hip if hip is not None else hip_outputs(m_dev, x, lengths, eps)
    ref64 = stock_outputs(copy.deepcopy(m_cpu).double(), x, lengths, eps)
    ref32 = stock_outputs(m_cpu, x, lengths, eps)
    assert set(hip) == set(ref64)
    worst = 0.0
    for name, r64 in ref64.items():
        r64 = r64.reshape(hip[name].shape)
        e_hip, e_cpu = bar_ratio(hip[name], r64), bar_ratio(ref32[name].reshape(r64.shape), r64)
        print(f"{tag} {name}: HIP {e_hip:.4f} of the bar, fp32 CPU {e_cpu:.4f}, mean |ref| {float(r64.abs().mean()):.4f}")
        worst = max(worst, e_hip)
    assert worst <= 1.0, (tag, worst)
    return hip


@pytest.mark.parametrize("case", CASES)
def test_fixture_parity(case):
    m = make_module(case)
    x, lengths, eps = case_inputs(case)
    hip = check(case, m, x, lengths, eps)
    # ... and through the module's forward: the same bits, in the reference's output shapes
    md = copy.deepcopy(m).to(DEV)
    with torch.no_grad():
        if case == "enc":
            assert torch.equal(md(x.to(DEV), lengths), hip["enc_out"])
            check("enc, no lengths", m, x, None, None)
            return
        xo, extra = md(x.to(DEV), lengths, None if eps is None else eps.to(DEV))
    B = x.shape[0]
    assert xo.shape == (B, 1, md.style_dims()["d_emb"]) and torch.equal(xo[:, 0], hip["x"])
    if case == "gst":
        assert extra == {}
    else:
        assert extra["kl"].shape == ((B, 1, 8) if case == "gstvae" else (B, 16)) and torch.equal(extra["kl"].reshape(B, -1), hip["kl"])
    assert len(md._engines.engines()) == 1  # (the HIP path ran: there is no quiet fall-back)


@functools.lru_cache(maxsize=None)
def full_vae(n_mels):
    torch.manual_seed(100 + n_mels)
    return randomize(S.VAE(num_mels=n_mels, dim_vae=16), 7 + n_mels)


# full filter widths; the frequency axis ends at 2, 1 and 1 bins (80 -> 40 20 10 5 3 2; 13 -> 7 4 2 1 1 1; 8 -> 4 2 1 1 1 1), odd
# sizes on the way; T = 1 and 37 end at one step, 130 at 3, 200 at 4; B = 33 crosses a 32-row block of the LSTM and GEMM tiles
@pytest.mark.parametrize("n_mels,T_,B", [(80, 200, 33), (13, 130, 5), (8, 37, 33), (80, 1, 1), (13, 37, 1), (8, 200, 5), (80, 130, 5), (13, 1, 33)])
def test_shapes_where_the_indexing_can_go_wrong(n_mels, T_, B):
    m = full_vae(n_mels)
    md = copy.deepcopy(m).to(DEV)
    lengths = lengths_for(B, T_)
    x = padded_input(B, T_, n_mels, lengths, seed=T_ + B)
    eps = torch.randn(B, 16, generator=torch.Generator().manual_seed(B))
    check(f"[{n_mels} mels, T {T_}, B {B}]", m, x, lengths, eps, m_dev=md)
    if B <= 5:  # every row runs all T' steps
        check(f"[{n_mels} mels, T {T_}, B {B}, no lengths]", m, x, None, eps, m_dev=md)


def test_large_m_first_gemm_stage():
    """8 x 600 x 80: stage 1 has 24 000 rows (188 tiles of 128 x 32), stage 3 the 32 x 32 split-K tile over 1 520 rows."""
    m = full_vae(80)
    lengths = torch.tensor([600, 1, 63, 64, 127, 128, 599, 333])
    x = padded_input(8, 600, 80, lengths, seed=4)
    eps = torch.randn(8, 16, generator=torch.Generator().manual_seed(4))
    check("[8 x 600 x 80]", m, x, lengths, eps)


@pytest.mark.parametrize("B", [1, 5, 33])
def test_batch_independence_bit_for_bit(B):
    """Zero padding, lengths >= 64 (the module docstring says why): row b of the batch == the utterance alone, torch.equal."""
    for tag, m, n_mels in (("vae", full_vae(80), 80), ("gstvae", make_module("gstvae"), 20)):
        md = copy.deepcopy(m).to(DEV)
        d_vae = md.style_dims()["d_vae"]
        pool = (200, 64, 127, 128, 65, 191, 192, 100)
        lengths = torch.tensor([pool[b % len(pool)] for b in range(B)])
        x = padded_input(B, 200, n_mels, lengths, seed=B)
        eps = torch.randn(B, d_vae, generator=torch.Generator().manual_seed(B + 1))
        batch = hip_outputs(md, x, lengths, eps)
        for b in (range(B) if tag == "vae" or B <= 5 else (0, 1, 32)):
            n = int(lengths[b])
            alone = hip_outputs(md, x[b:b + 1, :n], lengths[b:b + 1], eps[b:b + 1])
            for name in batch:
                assert torch.equal(batch[name][b:b + 1], alone[name]), (tag, B, b, name)
    # the oracle agrees with what was compared (once, at the largest batch's inputs, is enough: the other tests hold the bar)
    if B == 5:
        check("batch of 5", m, x, lengths, eps, hip=batch)


def test_unmasked_convs_see_the_padded_frames():
    """Garbage beyond the lengths: the result still matches the oracle given the same garbage.  It changes the rows shorter than 64
    frames - their one clipped step reads beyond the end - and leaves every other row's bits alone (the module docstring's reach
    argument: from 64 frames on nothing beyond the end is read), so the full-width fixture, 130 and 70 frames, does not move at all."""
    for case in ("gst", "vae"):
        m = make_module(case)
        x0, lengths, eps = case_inputs(case)
        x = x0.clone()
        g = torch.Generator().manual_seed(9)
        for b, n in enumerate(lengths.tolist()):
            x[b, n:] = 3.0 * torch.randn(x.shape[1] - n, x.shape[2], generator=g)
        md = copy.deepcopy(m).to(DEV)
        dirty = check(case + " + garbage", m, x, lengths, eps, m_dev=md)
        clean = hip_outputs(md, x0, lengths, eps)
        short = [b for b, n in enumerate(lengths.tolist()) if n < 64]
        rest = [b for b, n in enumerate(lengths.tolist()) if n >= 64]
        assert len(short) == (2 if case == "gst" else 0)
        for name in dirty:
            assert torch.equal(dirty[name][rest], clean[name][rest]), (case, name)
            for b in short:
                assert not torch.equal(dirty[name][b], clean[name][b]), (case, name, b)


def test_lengths_determinism_and_input_layouts():
    m = full_vae(80)
    md = copy.deepcopy(m).to(DEV)
    B, T_ = 5, 130
    lengths = lengths_for(B, T_)
    x = padded_input(B, T_, 80, lengths, seed=2)
    eps = torch.randn(B, 16, generator=torch.Generator().manual_seed(2))
    first = hip_outputs(md, x, lengths, eps)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)  # noqa: E731
    assert same(first, hip_outputs(md, x, lengths, eps))                          # a second call
    assert same(first, hip_outputs(md, x, lengths.to(DEV), eps))                  # device lengths
    assert same(first, hip_outputs(md, x, lengths.tolist(), eps))                 # a list
    assert same(first, hip_outputs(md, x, lengths.to(torch.int32), eps))
    # a device-side length above T is clamped to the T' steps there are (documented in style.py): that row then runs as it does
    # without lengths (T' = 3 steps; its own length, 130 frames, gives 2), the other rows as before
    over = lengths.clone()
    over[0] = T_ + 500
    clamped, free = hip_outputs(md, x, over.to(DEV), eps), hip_outputs(md, x, None, eps)
    for k in first:
        assert torch.equal(clamped[k][0], free[k][0]) and not torch.equal(clamped[k][0], first[k][0]) and torch.equal(clamped[k][1:], first[k][1:])
    # a slice of a wider tensor goes through ldx as it lies; a time-major tensor through a copy
    wide = torch.randn(B, T_, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
    wide[:, :, 5:85] = x.to(DEV)
    xs = wide[:, :, 5:85]
    assert not xs.is_contiguous()
    with torch.no_grad():
        assert same(first, dict(zip(("enc_out", "x", "kl"), md._hip_forward(xs, lengths, eps.to(DEV)))))
        xt = x.transpose(0, 1).contiguous().to(DEV).transpose(0, 1)
        assert not xt.is_contiguous()
        assert same(first, dict(zip(("enc_out", "x", "kl"), md._hip_forward(xt, lengths, eps.to(DEV)))))
        # through forward: eps = None draws on the device (a different draw changes x and leaves kl alone)
        xo1, e1 = md(x.to(DEV), lengths)
        xo2, e2 = md(x.to(DEV), lengths)
        assert torch.equal(e1["kl"], first["kl"]) and torch.equal(e1["kl"], e2["kl"]) and not torch.equal(xo1, xo2)
        with pytest.raises(ValueError):
            md(x.to(DEV), torch.tensor([131, 5, 5, 5, 5]))
        # training mode and a wanted gradient both take the stock path, on the GPU as well
        assert not md.train()._hip_ok(x.to(DEV))
    assert not md.eval()._hip_ok(x.to(DEV))  # (grad enabled, parameters want one)
    with torch.no_grad():
        assert md._hip_ok(x.to(DEV)) and not md._hip_ok(x.to(DEV).double())


def test_end_to_end_through_build_tacotron():
    torch.manual_seed(0)
    model = randomize(T.build_tacotron(_config()), 12).to(DEV)
    model.decoder.dropout_source, model.decoder.dropout_seed = "philox", 3  # (the PreNet's always-on dropout: the same draw in both runs)
    ids = torch.tensor([[1, 2, 3, 4, 5, 6, 7], [3, 2, 1, 8, 0, 0, 0]], device=DEV)
    lens = torch.tensor([7, 4])
    xl = torch.tensor([150, 90])
    xref = padded_input(2, 150, 20, xl, seed=6)
    with torch.no_grad():
        torch.manual_seed(5)
        y, y_post, s, out = model(ids, lens, xref=xref.to(DEV), xref_lengths=xl, max_steps=20)
        torch.manual_seed(5)
        eps = torch.randn(2, 8, device=DEV)  # the draw VAE.forward made
        ref = stock_outputs(copy.deepcopy(model.refencoder).cpu().double(), xref, xl, eps.cpu())
        memory = model.encoder(ids, lens) + ref["x"].to(device=DEV, dtype=torch.float32)
        y_ref, s_ref, w_ref = model.decoder(memory, T.lengths_to_mask(lens).to(DEV), None, 20, p_no_forcing=0.1)
    assert y.shape == y_ref.shape and y.shape[1] == 21
    e_y, e_kl = bar_ratio(y, y_ref), bar_ratio(out["kl_loss"], ref["kl"].mean())
    print(f"end to end: y {e_y:.4f} of the bar, kl_loss {e_kl:.4f}; kl_loss = {float(out['kl_loss']):.4f}")
    assert e_y <= 1.0 and e_kl <= 1.0 and float(out["kl_loss"]) > 1e-2
    assert len(model.refencoder._engines.engines()) == 1
