"""Host-side checks of the native mel -> waveform path (torch-tts_amd/audio.py ``mel_to_magnitude`` / ``griffinlim_native`` /
``synth_audio_native``, csrc/griffinlim.hip): the C-ABI declarations, exports and host-only refusals, the inverse basis P against
fp64 ``lstsq``, the sample / frame arithmetic, the Python refusals (all before any device work), and the restatement of
``audio.griffinlim``'s loop from a given state that tests/test_griffinlim_hip.py measures against.  No GPU."""
import math
import os
import re

import pytest
import torch

import torch_tts_amd as T
from torch_tts_amd import _lib

A = T.audio
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SR = 22050


# ---------------------------------------------------------------------------------------------------------------------------
# shared with the GPU tests: signals, and audio.py's torch-op code from an explicit state, in the dtype of its input
# ---------------------------------------------------------------------------------------------------------------------------
def voiced(n, seed):
    """sin(2 pi (200 + 300 t) t) * sin(2 pi 3 t)^2 + 0.05 randn, t in seconds at 22 050 Hz, peak-normalised (fp64)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SR
    x = torch.sin(2 * math.pi * (200 + 300 * t) * t) * torch.sin(2 * math.pi * 3 * t) ** 2 + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    return x / x.abs().max()


def frontend(n_fft=1024, hop=256, device=None, dtype=torch.float32):
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=SR, hop_length=hop, win_length=n_fft, num_mels=80, fmin=0, fmax=8000), device)
    fe.fb = fe.fb.to(dtype)
    return fe


def magnitude_of(x, n_fft, hop):
    """|STFT| of x (fp64) -> [bins, T], T = 1 + len(x) // hop."""
    w = torch.hann_window(n_fft, dtype=torch.float64)
    return torch.stft(x, n_fft, hop, n_fft, w, return_complex=True).abs()


def model_mel(x, fe64):
    """signal -> power spectrogram -> mel dB -> m_fwd: the normalised mel [T, n_mels] the model would emit, fp32."""
    S = magnitude_of(x, fe64.n_fft, fe64.config.hop_length).pow(2)
    return A.m_fwd(A.amplitude_to_db(fe64.stft_to_mels(S), 10, 1e-12, 0).mT).to(torch.float32)


def mel_chain(y, fe):
    """synth_audio + decode + griffinlim up to the loop: y [T, n_mels] -> magnitude [bins, T] in y's dtype (fe.fb of that dtype)."""
    return A.db_to_amplitude(fe.mel_inv(A.m_rev(y)), 1, 1).pow(0.5)


def gl_loop(mag, angles, tprev, n_fft, hop, n_iter, momentum=0.99, keep=()):
    """audio.griffinlim's loop from a given state (its lines after the start is drawn), in mag's dtype: -> wave, rebuilt (tprev),
    angles, and {k: (angles, tprev) before iteration k} for k in keep."""
    cdt = torch.complex128 if mag.dtype == torch.float64 else torch.complex64
    window = torch.hann_window(n_fft, dtype=mag.dtype)
    angles = angles.to(cdt)
    tprev = torch.zeros_like(angles) if tprev is None else tprev.to(cdt)
    mom = momentum / (1 + momentum)
    states = {}
    for k in range(n_iter):
        if k in keep:
            states[k] = (angles, tprev)
        inverse = torch.istft(mag * angles, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window)
        rebuilt = torch.stft(inverse, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                             normalized=False, onesided=True, return_complex=True)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * mom
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    wave = torch.istft(mag * angles, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window)
    return wave, tprev, angles, states


def random_start(shape, seed):
    """The start audio.griffinlim draws for a tensor of this shape from a CPU generator of this seed."""
    g = torch.Generator().manual_seed(seed)
    re = torch.rand(shape, generator=g)
    im = torch.rand(shape, generator=g)
    return torch.complex(re, im)


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_audio_griffinlim():
    mag = magnitude_of(voiced(256 * 20, 3), 1024, 256)
    for dt in (torch.float64, torch.float32):
        m = mag.to(dt)
        want = A.griffinlim(m.pow(2), 1024, 256, 1024, n_iter=5, generator=torch.Generator().manual_seed(11))
        got, _, _, st = gl_loop(m, random_start(m.shape, 11), None, 1024, 256, 5, keep=(0, 3))
        assert torch.allclose(got, want, rtol=0, atol=1e-12 if dt == torch.float64 else 1e-5)  # (pow(2).pow(1 / 2) apart)
        assert set(st) == {0, 3} and float(st[0][1].abs().max()) == 0.0
    # from the all-ones start too
    want = A.griffinlim(mag.pow(2), 1024, 256, 1024, n_iter=3, rand_init=False)
    got = gl_loop(mag, torch.ones(mag.shape, dtype=torch.complex128), None, 1024, 256, 3)[0]
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_new_ttsdec_symbols_are_declared_bound_and_exported():
    new = ("ttsdec_griffinlim_workspace_bytes", "ttsdec_mel_to_magnitude", "ttsdec_griffinlim")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in new:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsdec"] and hasattr(lib, sym), sym
    assert lib.ttsdec_version() == 2 and len(_lib.FAMILIES) == 6
    eng = T.Engine(T.EngineDims(), None)
    h = eng._h
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    ws = lib.ttsdec_griffinlim_workspace_bytes
    assert ws(h, 3, 40, 1024) == up(1024 * 8) + up(3 * 40 * 513 * 4) + 2 * up(3 * 40 * 513 * 8) + up(3 * 40 * 1024 * 4)
    assert ws(h, 1, 40, 768) == 0 and ws(h, 1, 40, 4096) == 0 and ws(h, 1, 1, 1024) == 0 and ws(h, 0, 40, 1024) == 0
    one, big = 256, 1 << 30  # (non-null placeholders: every call below is refused on the host)
    gl = lambda B, T_, n_fft, hop, n_iter=1, mom=0.99, wsb=big, mag=one: lib.ttsdec_griffinlim(  # noqa: E731
        h, mag, None, B, T_, one, n_fft, hop, None, None, n_iter, mom, 0, one, None, None, None, one, wsb, None)
    assert gl(1, 40, 768, 192) == _lib.ERR_DIMS and gl(1, 40, 1024, 513) == _lib.ERR_DIMS and gl(1, 1, 1024, 256) == _lib.ERR_DIMS
    assert gl(0, 40, 1024, 256) == _lib.ERR_INVALID_ARG and gl(1, 40, 1024, 0) == _lib.ERR_INVALID_ARG and gl(1, 0, 1024, 256) == _lib.ERR_INVALID_ARG
    assert gl(1, 40, 1024, 256, n_iter=-1) == _lib.ERR_INVALID_ARG and gl(1, 40, 1024, 256, mom=1.0) == _lib.ERR_INVALID_ARG
    assert gl(1, 40, 1024, 256, mag=None) == _lib.ERR_INVALID_ARG
    assert gl(1, 40, 1024, 256, wsb=4096) == _lib.ERR_WORKSPACE
    # the state outputs exist from the first iteration on
    assert lib.ttsdec_griffinlim(h, one, None, 1, 40, one, 1024, 256, None, None, 0, 0.99, 0, one, one, one, None, one, big, None) == _lib.ERR_INVALID_ARG
    m2m = lambda B, T_, n_mels, n_fft, y=one: lib.ttsdec_mel_to_magnitude(h, y, one, None, B, T_, n_mels, n_fft, one, None, None)  # noqa: E731
    assert m2m(1, 40, 80, 768) == _lib.ERR_DIMS and m2m(1, 40, 257, 1024) == _lib.ERR_DIMS and m2m(1, 1, 80, 1024) == _lib.ERR_DIMS
    assert m2m(0, 40, 80, 1024) == _lib.ERR_INVALID_ARG and m2m(1, 40, 0, 1024) == _lib.ERR_INVALID_ARG
    assert m2m(1, 40, 80, 1024, y=None) == _lib.ERR_INVALID_ARG
    eng.close()


def test_inverse_basis_is_the_gels_solution_on_the_ljspeech_basis():
    fe = frontend()
    fb64 = fe.fb.double()
    assert fb64.shape == (513, 80) and int(torch.linalg.matrix_rank(fb64)) == 80  # full row rank of fb^T: the solution is the minimum-norm one
    P = fe.inverse_basis()
    assert P.dtype == torch.float32 and P.shape == (513, 80) and P is fe.inverse_basis()
    M = model_mel(voiced(256 * 60, 5), frontend(dtype=torch.float64)).double().T  # any right-hand side would do; a mel of the test signal
    M = A.db_to_amplitude(A.m_rev(M), 1, 1)
    sol = torch.linalg.lstsq(fb64.T.contiguous(), M, driver="gels").solution
    err64 = float((P.double() @ M - sol).abs().max() / sol.abs().max())
    err32 = float(((P @ M.float()).double() - sol).abs().max() / sol.abs().max())
    gels32 = torch.linalg.lstsq(fe.fb.T.contiguous(), M.float(), driver="gels").solution
    ref32 = float((gels32.double() - sol).abs().max() / sol.abs().max())
    print(f"P (rounded to fp32) @ M in fp64 vs fp64 gels: {err64:.3g}; fp32 P @ M: {err32:.3g}; fp32 gels: {ref32:.3g}")
    assert err64 < 2.0 ** -23  # the one rounding of P
    assert err32 < 1e-6
    # and P is a right inverse of fb^T: the inverted mel maps back to the mel
    assert float((fb64.T @ P.double() - torch.eye(80, dtype=torch.float64)).abs().max()) < 1e-5


def test_sample_and_frame_arithmetic():
    for n_fft, hop in ((1024, 256), (512, 128), (2048, 512), (256, 128), (512, 100)):
        w = torch.hann_window(n_fft, dtype=torch.float64)
        for frames in (2, 3, 17):
            spec = torch.ones(n_fft // 2 + 1, frames, dtype=torch.complex128)
            n = torch.istft(spec, n_fft, hop, n_fft, w).numel()
            assert A.wave_samples(frames, hop) == n == hop * (frames - 1)
            if n > n_fft // 2:  # (torch refuses to reflect an utterance no longer than the padding)
                assert torch.stft(torch.zeros(n, dtype=torch.float64), n_fft, hop, n_fft, w, return_complex=True).shape[1] == frames


def test_entry_points_refuse_before_any_device_work():
    cpu = torch.zeros(1, 513, 8)
    with pytest.raises(_lib.DimsNotBuilt, match="768"):  # the dataclass default: needs a radix-3 pass
        A.griffinlim_native(torch.zeros(1, 385, 8), 768, 192, 768)
    with pytest.raises(_lib.DimsNotBuilt, match="768"):
        A.AudioFrontend(A.AudioFrontendConfig()).mel_to_magnitude(torch.zeros(1, 8, 80))
    with pytest.raises(_lib.DimsNotBuilt, match="hop_length"):  # hop > n_fft / 2
        A.griffinlim_native(cpu, 1024, 513, 1024)
    with pytest.raises(_lib.DimsNotBuilt, match="win_length"):
        A.griffinlim_native(cpu, 1024, 256, 800)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        A.griffinlim_native(cpu, 1024, 256, 1024)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        frontend().mel_to_magnitude(torch.zeros(1, 8, 80))
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        A.synth_audio_native(torch.zeros(1, 8, 80), frontend())
    assert issubclass(_lib.DimsNotBuilt, NotImplementedError)
    with pytest.raises(NotImplementedError, match="exact fp32"):  # fp64
        A.griffinlim_native(cpu.double(), 1024, 256, 1024)
    with pytest.raises(NotImplementedError, match="exact fp32"):
        frontend().mel_to_magnitude(torch.zeros(1, 8, 80, dtype=torch.float64))
