"""The native mel -> waveform path on the GPU (csrc/griffinlim.hip through audio.mel_to_magnitude / griffinlim_native /
synth_audio_native) against audio.py's torch-op code run in fp64 on the CPU from the same inputs and the same initial phase.  The
margin of every bar is the same torch-op code run in fp32 on the CPU, computed here on the same inputs and printed before it is
asserted: 4 x for what is a count of roundings (mel inversion, one inverse, one iteration), 8 x for the drift of 32 iterations, which
is rounding error amplified by the iteration.  The HIP path is never compared with itself (except for bit-equality) nor with the
torch-op path on the GPU.  Parity with torchaudio itself stays unpinned (it is absent)."""
import math

import pytest
import torch

import torch_tts_amd as T
from test_griffinlim_host import frontend, gl_loop, magnitude_of, mel_chain, model_mel, random_start, voiced

pytestmark = pytest.mark.gpu
A = T.audio
DEV = torch.device("cuda:0")
CONFIGS = ((1024, 256, 120), (1024, 256, 600), (512, 128, 90), (2048, 512, 70))  # n_fft, hop, frames
# ... and an odd hop - the forward kernel's scalar first pass; the pairs need an even frame stride - whose 11 frames leave the
# 16-frame run partly filled (the one-pass tests only: the 32-iteration ones would add nothing on that branch)
ONE_PASS_CONFIGS = CONFIGS + ((256, 63, 11),)


def rel(w, w64):
    return float((w.double().cpu() - w64).abs().max() / w64.abs().max())


def frame_rel(r, r64):
    """max over frames of max_bins |d| / max_bins |r64|: [bins, T] complex each."""
    return float(((r.cpu().to(torch.complex128) - r64).abs().amax(0) / r64.abs().amax(0)).max())


def spec_input(n_fft, hop, frames, seed=1):
    """The magnitude spectrogram of the voiced signal, fp32 [bins, frames]: the input all three paths share."""
    return magnitude_of(voiced(hop * (frames - 1), seed), n_fft, hop).to(torch.float32)


def mel_input(frames, seed=2):
    """The normalised mel of the voiced signal [frames, 80] fp32 (1024 / 256)."""
    return model_mel(voiced(256 * (frames - 1), seed), frontend(dtype=torch.float64))


def test_mel_to_magnitude_against_the_fp64_chain():
    fe, fe64, feg = frontend(), frontend(dtype=torch.float64), frontend(device=DEV)
    lens = [120, 600, 77]
    y = torch.zeros(3, 600, 80)
    for b, n in enumerate(lens):
        y[b, :n] = mel_input(n, seed=20 + b)
    mag = feg.mel_to_magnitude(y.to(DEV), lens)
    assert mag.shape == (3, 513, 600) and mag.dtype == torch.float32
    for b, n in enumerate(lens):
        m64 = mel_chain(y[b, :n].double(), fe64)
        m32 = mel_chain(y[b, :n], fe)
        e32, e = rel(m32, m64), rel(mag[b, :, :n], m64)
        floor = float((mag[b, :, :n] < 1.5e-6).float().mean())
        print(f"mel -> magnitude, {n} frames: HIP {e:.3g}, torch fp32 gels {e32:.3g}, ratio {e / e32:.2f}; bins at the 1e-6 floor {floor:.2f}")
        assert e <= 4 * e32
        assert floor > 0.2  # the clamp of the dB round trip is kept: a zero of D is 1e-12, its magnitude 1e-6
        assert float(mag[b, :, n:].abs().max()) == 0.0 if n < 600 else True
    alone = feg.mel_to_magnitude(y[2, :77].to(DEV))
    assert torch.equal(alone, mag[2, :, :77])
    assert torch.equal(feg.mel_to_magnitude(y.to(DEV), torch.tensor(lens, device=DEV)), mag)


@pytest.mark.parametrize("n_fft,hop,frames", ONE_PASS_CONFIGS)
def test_inverse_stft_alone(n_fft, hop, frames):
    mag = spec_input(n_fft, hop, frames)
    ang = random_start(mag.shape, 5)
    w64 = gl_loop(mag.double(), ang, None, n_fft, hop, 0)[0]
    w32 = gl_loop(mag, ang, None, n_fft, hop, 0)[0]
    w, reb, ang_out = A.griffinlim_native(mag.to(DEV), n_fft, hop, n_fft, n_iter=0, angles=ang.to(DEV), return_state=True)
    assert w.shape == (hop * (frames - 1),) and torch.equal(ang_out.cpu(), ang) and float(reb.abs().max()) == 0.0
    e, e32 = rel(w, w64), rel(w32, w64)
    print(f"istft {n_fft} / {hop}, {frames} frames: HIP {e:.3g}, torch fp32 {e32:.3g}, ratio {e / e32:.2f}")
    assert e <= 4 * e32


@pytest.mark.parametrize("n_fft,hop,frames", ONE_PASS_CONFIGS)
def test_one_iteration_from_the_fp64_runs_own_state(n_fft, hop, frames):
    mags = {"spectrogram": spec_input(n_fft, hop, frames)}
    if n_fft == 1024:
        mags["inverted mel"] = mel_chain(mel_input(frames), frontend())
    for name, mag in mags.items():
        states = gl_loop(mag.double(), random_start(mag.shape, 6), None, n_fft, hop, 32, keep=(0, 1, 8, 31))[3]
        for k, (ang, tprev) in states.items():
            ang, tprev = ang.to(torch.complex64), tprev.to(torch.complex64)  # the state all three paths start from
            w64, r64, _, _ = gl_loop(mag.double(), ang, tprev, n_fft, hop, 1)
            w32, r32, _, _ = gl_loop(mag, ang, tprev, n_fft, hop, 1)
            w, r, _ = A.griffinlim_native(mag.to(DEV), n_fft, hop, n_fft, n_iter=1, angles=ang.to(DEV), tprev=tprev.to(DEV), return_state=True)
            er, er32, ew, ew32 = frame_rel(r, r64), frame_rel(r32, r64), rel(w, w64), rel(w32, w64)
            print(f"{n_fft} / {hop}, {frames} frames, {name}, iteration {k}: rebuilt HIP {er:.3g} torch fp32 {er32:.3g} (ratio {er / er32:.2f}); "
                  f"wave HIP {ew:.3g} torch fp32 {ew32:.3g} (ratio {ew / ew32:.2f})")
            assert er <= 4 * er32 and ew <= 4 * ew32  # (not the angles: a unit phasor of a near-zero bin is ill-conditioned)


def drift_case(mag, n_fft, hop, seed, what):
    ang = random_start(mag.shape, seed)
    w64 = gl_loop(mag.double(), ang, None, n_fft, hop, 32)[0]
    w32 = gl_loop(mag, ang, None, n_fft, hop, 32)[0]
    w = A.griffinlim_native(mag.to(DEV), n_fft, hop, n_fft, generator=torch.Generator().manual_seed(seed))
    d, d32 = rel(w, w64), rel(w32, w64)
    print(f"32 iterations, {what}: drift from fp64 HIP {d:.3g}, torch fp32 {d32:.3g}, ratio {d / d32:.2f}")
    return d, d32


@pytest.mark.parametrize("n_fft,hop,frames", CONFIGS)
def test_32_iterations_random_start_spectrogram(n_fft, hop, frames):
    d, d32 = drift_case(spec_input(n_fft, hop, frames), n_fft, hop, 7, f"spectrogram {n_fft} / {hop}, {frames} frames")
    assert d <= 8 * d32


@pytest.mark.parametrize("frames", (120, 600))
def test_32_iterations_random_start_inverted_mel(frames):
    d, d32 = drift_case(mel_chain(mel_input(frames), frontend()), 1024, 256, 8, f"inverted mel, {frames} frames")
    assert d <= 8 * d32


def test_spectral_convergence_on_the_three_tone_signal():
    t = torch.arange(22050) / 22050
    x = 0.5 * torch.sin(2 * math.pi * 440 * t) + 0.3 * torch.sin(2 * math.pi * 1200 * t) + 0.1 * torch.sin(2 * math.pi * 3100 * t)
    w = torch.hann_window(1024)
    S = torch.stft(x, 1024, 256, 1024, w, return_complex=True).abs()
    wave = A.griffinlim_native(S.to(DEV), 1024, 256, 1024, generator=torch.Generator().manual_seed(0)).cpu()
    S2 = torch.stft(wave, 1024, 256, 1024, w, return_complex=True).abs()
    n = min(S.shape[-1], S2.shape[-1])
    conv = float((S2[:, :n] - S[:, :n]).norm() / S[:, :n].norm())
    print(f"spectral convergence after 32 iterations: {conv:.4f}")
    assert conv < 0.15, conv


@pytest.mark.parametrize("B", (1, 5, 64))
def test_ragged_batch_is_each_utterance_alone_bit_for_bit(B):
    n_fft, hop, T_ = 1024, 256, 37
    g = torch.Generator().manual_seed(B)
    lens = [T_, 2, 3, 5, 36][:B] + [int(v) for v in torch.randint(2, T_ + 1, (max(B - 5, 0),), generator=g)]
    mag = (torch.rand(B, 513, T_, generator=g) * spec_input(n_fft, hop, T_)).to(DEV)
    ang = random_start((B, 513, T_), 9).to(DEV)
    wave, reb, a = A.griffinlim_native(mag, n_fft, hop, n_fft, n_iter=3, lengths=lens, angles=ang, normalize=True, return_state=True)
    assert wave.shape == (B, hop * (T_ - 1)) and bool(torch.isfinite(wave).all())
    for b, n in enumerate(lens):
        w1, r1, a1 = A.griffinlim_native(mag[b, :, :n].contiguous(), n_fft, hop, n_fft, n_iter=3, angles=ang[b, :, :n].contiguous(), normalize=True,
                                         return_state=True)
        L = hop * (n - 1)
        assert torch.equal(wave[b, :L], w1) and torch.equal(reb[b, :, :n], r1) and torch.equal(a[b, :, :n], a1), (b, n)
        assert abs(float(w1.abs().max()) - 1.0) < 1e-6
        if n < T_:  # exact zeros past each end
            assert float(wave[b, L:].abs().max()) == 0.0 and float(reb[b, :, n:].abs().max()) == 0.0 and float(a[b, :, n:].abs().max()) == 0.0
    on_dev = A.griffinlim_native(mag, n_fft, hop, n_fft, n_iter=3, lengths=torch.tensor(lens, device=DEV), angles=ang, normalize=True)
    assert torch.equal(on_dev, wave)
    if B == 5:  # lengths the host has not seen are refused through the status word
        with pytest.raises(ValueError, match="fewer than 2"):
            A.griffinlim_native(mag, n_fft, hop, n_fft, n_iter=1, lengths=torch.tensor([T_, 1, 3, 5, 36], device=DEV), angles=ang)
        with pytest.raises(ValueError, match="exceeds"):
            A.griffinlim_native(mag, n_fft, hop, n_fft, n_iter=1, lengths=torch.tensor([T_ + 1, 2, 3, 5, 36], device=DEV), angles=ang)
        with pytest.raises(ValueError, match="lengths"):
            A.griffinlim_native(mag, n_fft, hop, n_fft, lengths=[T_, 1, 3, 5, 36])


def test_synth_audio_native_against_the_fp64_chain():
    fe, fe64, feg = frontend(), frontend(dtype=torch.float64), frontend(device=DEV)
    lens = [120, 75, 33]
    y = torch.zeros(3, 120, 80)
    for b, n in enumerate(lens):
        y[b, :n] = mel_input(n, seed=30 + b)
    out = A.synth_audio_native(y.to(DEV), feg, lens, generator=torch.Generator().manual_seed(12))
    assert out.shape == (3, 256 * 119) and out.is_cuda
    start = random_start((3, 513, 120), 12)  # the two torch.rand calls of the batch
    for b, n in enumerate(lens):
        ang = start[b, :, :n]
        w64 = gl_loop(mel_chain(y[b, :n].double(), fe64), ang, None, 1024, 256, 32)[0]
        w32 = gl_loop(mel_chain(y[b, :n], fe), ang, None, 1024, 256, 32)[0]
        w64, w32 = w64 / w64.abs().max(), w32 / w32.abs().max()
        L = 256 * (n - 1)
        d, d32 = rel(out[b, :L], w64), rel(w32, w64)
        peak = float(out[b, :L].abs().max())
        print(f"synth_audio_native, utterance of {n} frames: drift from fp64 HIP {d:.3g}, torch fp32 {d32:.3g}, ratio {d / d32:.2f}; peak {peak!r}")
        assert abs(peak - 1.0) < 1e-6
        assert float(out[b, L:].abs().max()) == 0.0 if n < 120 else True
        assert d <= 8 * d32
    assert torch.equal(A.synth_audio_native(y.to(DEV), feg, torch.tensor(lens, device=DEV), generator=torch.Generator().manual_seed(12)), out)


def test_the_same_call_twice_is_equal():
    mag = spec_input(1024, 256, 120).to(DEV)
    for kw in (dict(generator=None, rand_init=False), dict(rand_init=True)):  # the all-ones start: supported, tested for determinism only
        gen = lambda: torch.Generator().manual_seed(4)  # noqa: E731
        a = A.griffinlim_native(mag, 1024, 256, 1024, **{"generator": gen(), **kw})
        b = A.griffinlim_native(mag, 1024, 256, 1024, **{"generator": gen(), **kw})
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    fe = frontend(device=DEV)
    y = mel_input(50).to(DEV)[None]
    assert torch.equal(fe.mel_to_magnitude(y), fe.mel_to_magnitude(y))
    with pytest.raises(NotImplementedError, match="exact fp32"):
        A.griffinlim_native(mag.double(), 1024, 256, 1024)
    with pytest.raises(ValueError, match="2 frames"):
        A.griffinlim_native(torch.zeros(1, 513, 1, device=DEV), 1024, 256, 1024)
