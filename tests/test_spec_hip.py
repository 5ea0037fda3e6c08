"""GPU checks of the VITS2 spectrogram front-end (csrc/spec.hip through torch_tts_amd.mel_processing) against the reference's fp64
results of tests/golden/spec_small.npz and the restatement pinned in tests/test_spec_host.py.

Bars: the linear spectrogram is held, per frame, to max_bins |s - s64| / max_bins s64 <= 4 x the reference's own fp32 value of that
metric (spec_meta.json, per configuration) - another, equally careful fp32 summation order; the log-mel to |d| <= 1e-5 + 1e-4 |ref|,
the stage tolerance of tests/test_vc_hip.py.  The figures are printed before they are asserted."""
import math

import pytest
import torch

from test_spec_host import frame_err, golden_batch, load_golden, spec_to_mel_one, spectrogram_batch, spectrogram_one

pytestmark = pytest.mark.gpu
SR = 22050


def dev():
    return torch.device("cuda:0")


def MP():
    from torch_tts_amd import mel_processing

    return mel_processing


def mel_ok(m, ref64):
    d = (m.double().cpu() - ref64).abs()
    return bool((d <= 1e-5 + 1e-4 * ref64.abs()).all()), float(d.max())


def test_linear_spectrogram_against_fp64_golden():
    sd, meta = load_golden()
    for ci, c in enumerate(meta["configs"]):
        y, lens = golden_batch(sd, c, ci)
        spec, sl = MP().spectrogram_torch(y.to(dev()), c["n_fft"], SR, c["hop"], c["win"], lengths=lens)
        spec = spec.cpu()
        worst = 0.0
        for ui in range(3):
            s64 = torch.from_numpy(sd[f"c{ci}/u{ui}/spec64"])
            T = s64.shape[1]
            assert int(sl[ui]) == T
            worst = max(worst, frame_err(spec[ui, :, :T], s64))  # every bin of every valid frame
            assert not spec[ui, :, T:].any()
        print(f"spec config {ci} (n_fft {c['n_fft']}, hop {c['hop']}, win {c['win']}): HIP frame err {worst:.3e}, reference fp32 "
              f"{c['spec_frame_err']:.3e}, bar {4 * c['spec_frame_err']:.3e}")
        assert worst <= 4 * c["spec_frame_err"]


def test_log_mel_against_fp64_golden():
    sd, meta = load_golden()
    for ci, c in enumerate(meta["configs"]):
        y, lens = golden_batch(sd, c, ci)
        basis = torch.from_numpy(sd[f"basis/{c['n_fft']}"]).to(dev())
        a = (c["n_fft"], meta["n_mels"], SR)
        mel, sl = MP().mel_spectrogram_torch(y.to(dev()), *a, c["hop"], c["win"], 0.0, None, mel_basis=basis, lengths=lens)
        spec, _ = MP().spectrogram_torch(y.to(dev()), c["n_fft"], SR, c["hop"], c["win"], lengths=lens)
        mel2, sl2 = MP().spec_to_mel_torch(spec, *a, 0.0, None, mel_basis=basis, lengths=sl)
        assert torch.equal(sl, sl2)
        for ui in range(3):
            m64 = torch.from_numpy(sd[f"c{ci}/u{ui}/mel64"])
            T = m64.shape[1]
            for name, m in (("mel_spectrogram_torch", mel), ("spec_to_mel_torch", mel2)):
                ok, worst = mel_ok(m[ui, :, :T], m64)
                print(f"mel config {ci} utterance {ui} {name}: max |d| {worst:.3e} (reference fp32 {c['mel_abs_err']:.3e})")
                assert ok
                assert not m[ui, :, T:].any()
            ok, _ = mel_ok(mel[ui, :, :T], mel2[ui, :, :T].double().cpu())
            assert ok
        # the default basis is the recorded one
        mel3, _ = MP().mel_spectrogram_torch(y.to(dev()), *a, c["hop"], c["win"], 0.0, None, lengths=lens)
        assert torch.equal(mel3, mel)


def test_ragged_batch_equals_each_utterance_alone_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    for n_fft, hop, win, B in ((1024, 256, 1024, 5), (512, 100, 400, 3), (2048, 512, 2048, 2), (256, 64, 256, 64), (1024, 256, 1024, 1)):
        N = 6 * n_fft + 37
        lens = [N] + [int(v) for v in torch.randint(n_fft, N, (B - 1,), generator=g)]
        y = torch.rand(B, N, generator=g) * 1.6 - 0.8
        yd = y.to(dev())
        keep = yd.clone()
        basis = MP().default_mel_basis(n_fft, 80, SR, 0.0, None, dev())
        spec, sl = MP().spectrogram_torch(yd, n_fft, SR, hop, win, lengths=lens)
        mel, ml = MP().mel_spectrogram_torch(yd, n_fft, 80, SR, hop, win, 0.0, None, lengths=torch.tensor(lens, device=dev()))  # lengths on the device
        assert torch.equal(yd, keep)
        assert sl.tolist() == ml.tolist() == [MP().frame_count(n, n_fft, hop) for n in lens]
        again, _ = MP().spectrogram_torch(yd, n_fft, SR, hop, win, lengths=lens)
        assert torch.equal(spec, again)
        for b in range(B):
            alone = MP().spectrogram_torch(yd[b : b + 1, : lens[b]].contiguous(), n_fft, SR, hop, win)
            T = alone.shape[2]
            assert T == int(sl[b]) and torch.equal(spec[b, :, :T], alone[0]) and not spec[b, :, T:].any()
            alone_mel = MP().mel_spectrogram_torch(yd[b : b + 1, : lens[b]].contiguous(), n_fft, 80, SR, hop, win, 0.0, None, mel_basis=basis)
            assert torch.equal(mel[b, :, :T], alone_mel[0]) and not mel[b, :, T:].any()
        if B == 5:  # and the batch is the reference's per-utterance result
            ref, counts = spectrogram_batch(y.double(), lens, n_fft, hop, win)
            assert counts == sl.tolist()
            _, meta = load_golden()
            for b in range(B):
                assert frame_err(spec[b, :, : counts[b]].cpu(), ref[b, :, : counts[b]]) <= 4 * meta["configs"][0]["spec_frame_err"]


def test_status_word_refuses_short_utterances():
    y = torch.zeros(2, 4000, device=dev())
    with pytest.raises(ValueError):
        MP().spectrogram_torch(y, 1024, SR, 256, 1024, lengths=torch.tensor([4000, 384], device=dev()))  # len == pad
    with pytest.raises(ValueError):
        MP().spectrogram_torch(y, 1024, SR, 256, 1024, lengths=[4000, 384])
    with pytest.raises(ValueError):
        MP().spectrogram_torch(y, 1024, SR, 256, 1024, lengths=torch.tensor([4000, 4001], device=dev()))
    s, sl = MP().spectrogram_torch(y, 1024, SR, 256, 1024, lengths=torch.tensor([4000, 385], device=dev()))
    assert sl.tolist() == [15, 1]


def test_analytic_cases():
    _, meta = load_golden()
    bar = 4 * meta["configs"][0]["spec_frame_err"]
    n_fft, hop = 1024, 256
    pad = (n_fft - hop) // 2
    w = torch.hann_window(n_fft).double()
    N = 4 * n_fft
    # an impulse at offset p of frame 3: every bin sqrt(w[p]^2 + 1e-6)
    p = 300
    y = torch.zeros(1, N)
    y[0, 3 * hop + p - pad] = 1.0
    s = MP().spectrogram_torch(y.to(dev()), n_fft, SR, hop, n_fft).cpu()
    want = torch.sqrt(w[p] ** 2 + 1e-6).expand(n_fft // 2 + 1)
    e = frame_err(s[0, :, 3:4], want[:, None])
    print(f"impulse: frame err {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    # a unit cosine on bin k: sum(window) / 2 at k, half of that at k +- 1, the floor elsewhere
    k = 37
    t = torch.arange(N + 2 * pad, dtype=torch.float64) - pad
    y = torch.cos(2 * math.pi * k * t / n_fft)[pad : pad + N].to(torch.float32)[None]
    s = MP().spectrogram_torch(y.to(dev()), n_fft, SR, hop, n_fft).cpu()
    want = torch.full((n_fft // 2 + 1,), 1e-3, dtype=torch.float64)
    want[k] = torch.sqrt((w.sum() / 2) ** 2 + 1e-6)
    want[k - 1] = want[k + 1] = torch.sqrt((w.sum() / 4) ** 2 + 1e-6)
    e = frame_err(s[0, :, 4:8], want[:, None].expand(-1, 4))  # frames away from the reflected ends
    print(f"cosine: frame err {e:.3e}, bar {bar:.3e}")
    assert e <= bar
    # all-zero input: every bin exactly fp32 sqrt(1e-6); log-mel log(max(rowsum(basis) * sqrt(1e-6), 1e-5))
    z = torch.zeros(2, N, device=dev())
    s = MP().spectrogram_torch(z, n_fft, SR, hop, n_fft)
    floor = torch.sqrt(torch.tensor(1e-6, dtype=torch.float32))
    assert torch.equal(s, floor.to(dev()).expand_as(s))
    basis = MP().default_mel_basis(n_fft, 80, SR, 0.0, None, dev())
    m = MP().mel_spectrogram_torch(z, n_fft, 80, SR, hop, n_fft, 0.0, None)
    want = torch.log(torch.clamp(basis.double().cpu().sum(1) * float(floor), min=1e-5))[None, :, None].expand(2, -1, m.shape[2])
    ok, worst = mel_ok(m, want)
    print(f"zero input: log-mel max |d| {worst:.3e}")
    assert ok


def test_hop_longer_than_the_frame():
    """hop > n_fft: the frames do not overlap, the run's samples are loaded frame by frame and the negative padding crops both ends."""
    _, meta = load_golden()
    n_fft, hop, win = 256, 300, 200
    bar = 4 * meta["configs"][1]["spec_frame_err"]  # the n_fft = 256 configuration
    g = torch.Generator().manual_seed(13)
    y = torch.rand(2, 2500, generator=g) * 1.6 - 0.8
    lens = [2500, 1700]
    spec, sl = MP().spectrogram_torch(y.to(dev()), n_fft, SR, hop, win, lengths=lens)
    ref, counts = spectrogram_batch(y.double(), lens, n_fft, hop, win)
    assert counts == sl.tolist() == [8, 5] and spec.shape == ref.shape
    for b in range(2):
        e = frame_err(spec[b, :, : counts[b]].cpu(), ref[b, :, : counts[b]])
        print(f"n_fft {n_fft}, hop {hop}, win {win}, utterance {b}: frame err {e:.3e}, bar {bar:.3e}")
        assert e <= bar
        assert not spec[b, :, counts[b] :].any()


def test_benchmarked_shape():
    _, meta = load_golden()
    B, N, n_fft, hop = 64, 153600, 1024, 256
    g = torch.Generator().manual_seed(9)
    y = torch.rand(B, N, generator=g) * 1.8 - 0.9
    lens = [N] * B
    lens[7] = 100003
    yd = y.to(dev())
    spec, sl = MP().spectrogram_torch(yd, n_fft, SR, hop, n_fft, lengths=lens)
    mel, _ = MP().mel_spectrogram_torch(yd, n_fft, 80, SR, hop, n_fft, 0.0, None, lengths=lens)
    assert spec.shape == (B, 513, 600) and mel.shape == (B, 80, 600) and sl.tolist() == [MP().frame_count(n, n_fft, hop) for n in lens]
    basis = MP().default_mel_basis(n_fft, 80, SR, 0.0, None, dev()).cpu()
    for b in (7, 63):
        ref = spectrogram_one(y[b, : lens[b]].double(), n_fft, hop, n_fft)
        T = ref.shape[1]
        e = frame_err(spec[b, :, :T].cpu(), ref)
        ok, worst = mel_ok(mel[b, :, :T], spec_to_mel_one(ref, basis))
        print(f"benchmarked shape, utterance {b}: frame err {e:.3e}, log-mel max |d| {worst:.3e}")
        assert e <= 4 * meta["configs"][0]["spec_frame_err"] and ok
        assert not spec[b, :, T:].any() and not mel[b, :, T:].any()


@pytest.mark.parametrize("kind", ["linear", "mel"])
def test_from_audio_entry_points_equal_the_two_step_calls(kind):
    import torch_tts_amd as T
    from test_align_host import AlignNet
    from test_align_host import load_golden as align_golden
    from test_duration_host import randomize
    from test_vc_host import VcNet
    from test_vc_host import load_golden as vc_golden

    V = T.vits2
    n_fft, hop, n_mels = 256, 64, 80
    ch = n_fft // 2 + 1 if kind == "linear" else n_mels
    kw = dict(n_fft=n_fft, hop_size=hop, win_size=n_fft, sampling_rate=SR, n_mels=n_mels if kind == "mel" else None)
    front = (lambda w, l: V.spectrogram_torch(w, n_fft, SR, hop, n_fft, lengths=l)) if kind == "linear" else (
        lambda w, l: V.mel_spectrogram_torch(w, n_fft, n_mels, SR, hop, n_fft, 0.0, None, lengths=l))
    g = torch.Generator().manual_seed(11)
    wav = (torch.rand(2, 1500, generator=g) - 0.5).to(dev())
    wl = [1500, 1111]
    with torch.no_grad():
        _, vmeta = vc_golden()
        net = VcNet(dict(vmeta["net"], spec_channels=ch), 3, vmeta["vc"]["gin_channels"])
        for i, part in enumerate(("enc_q", "flow", "dec", "emb_g")):
            randomize(getattr(net, part), 40 + i)
        net = net.to(dev()).eval()
        y, yl = front(wav, wl)
        noise = torch.randn(2, net.enc_q.out_channels, y.shape[2], generator=g).to(dev())
        src, tgt = torch.tensor([0, 2], device=dev()), torch.tensor([1, 0], device=dev())
        a = V.voice_conversion_from_audio(net, wav, wl, src, tgt, noise=noise, **kw)
        b = V.voice_conversion(net, y, yl, src, tgt, noise=noise)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
        assert a[0].shape[0] == 2 and bool(a[0].abs().sum() > 0)

        _, ameta = align_golden()
        anet = AlignNet(dict(ameta["net"], spec_channels=ch), 3, ameta["model"]["gin_channels"])
        for i, part in enumerate(("enc_p", "enc_q", "flow", "emb_g")):
            randomize(getattr(anet, part), 50 + i)
        anet = anet.to(dev()).eval()
        x = torch.randint(0, ameta["net"]["n_vocab"], (2, 7), generator=g).to(dev())
        xl = torch.tensor([7, 5], device=dev())
        sid = torch.tensor([1, 2], device=dev())
        noise = torch.randn(2, anet.enc_q.out_channels, y.shape[2], generator=g).to(dev())
        a = V.forced_alignment_from_audio(anet, x, xl, wav, wl, sid, noise=noise, **kw)
        b = V.forced_alignment(anet, x, xl, y, yl, sid, noise=noise)
        assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
        assert a[1].sum(2).flatten().tolist() == [float(v) for v in yl.tolist()]  # every frame has a token
