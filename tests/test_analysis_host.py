"""Host-side checks of the waveform -> dB spectrogram / mel path (torch-tts_amd/audio.py ``AudioFrontend.encode`` /
``encode_native``, csrc/analysis.hip): the C-ABI declarations, exports and host-only refusals, ``encode`` against an independent
restatement with ``torch.stft`` in fp64, and the Python refusals (all before any device work).  No GPU."""
import os
import re

import pytest
import torch

import torch_tts_amd as T
from test_griffinlim_host import SR, frontend, voiced
from torch_tts_amd import _lib

A = T.audio
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_ttsdec_symbols_are_declared_bound_and_exported():
    new = ("ttsdec_mel_analysis_workspace_bytes", "ttsdec_mel_analysis")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in new:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsdec"] and hasattr(lib, sym), sym
    assert lib.ttsdec_version() == 2 and len(_lib.FAMILIES) == 6


def test_host_refusals_of_the_c_abi():
    lib = _lib.load()
    eng = T.Engine(T.EngineDims(), None)
    h = eng._h
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    ws = lib.ttsdec_mel_analysis_workspace_bytes
    assert ws(h, 3, 1024, 80) == up(1024 * 8) + up(80 * 8) + up(4) + up(3 * 4)  # twiddles, bands, 1 / sum w^2, peaks
    assert ws(h, 1, 768, 80) == 0 and ws(h, 1, 300, 80) == 0 and ws(h, 1, 4096, 80) == 0
    assert ws(h, 0, 1024, 80) == 0 and ws(h, 65536, 1024, 80) == 0 and ws(h, 1, 1024, 257) == 0 and ws(h, 1, 1024, 0) == 0
    assert ws(None, 1, 1024, 80) == 0
    one, big = 256, 1 << 30  # (non-null placeholders: every call below is refused on the host)

    def call(B=1, N=4096, n_mels=80, n_fft=1024, hop=256, T_=17, handle=h, wave=one, mel=one, wsb=big):
        return lib.ttsdec_mel_analysis(handle, wave, None, B, N, one, one, n_mels, n_fft, hop, T_, None, mel, None, None, one, wsb, None)

    assert call(n_fft=768, hop=192) == _lib.ERR_DIMS and call(n_fft=300, hop=75) == _lib.ERR_DIMS
    assert call(hop=1024 // 2 + 1) == _lib.ERR_DIMS and call(hop=0) == _lib.ERR_DIMS
    assert call(n_mels=257) == _lib.ERR_DIMS and call(B=65536) == _lib.ERR_DIMS
    assert call(T_=0) == _lib.ERR_DIMS and call(T_=(1 << 22) + 1) == _lib.ERR_DIMS
    assert call(handle=None) == _lib.ERR_INVALID_ARG
    assert call(B=0) == _lib.ERR_INVALID_ARG and call(N=0) == _lib.ERR_INVALID_ARG and call(n_mels=0) == _lib.ERR_INVALID_ARG
    assert call(wave=None) == _lib.ERR_INVALID_ARG and call(mel=None) == _lib.ERR_INVALID_ARG
    assert call(wsb=4096) == _lib.ERR_WORKSPACE
    eng.close()


@pytest.mark.parametrize("n_fft,hop,n", ((1024, 256, 256 * 30 + 37), (512, 128, 128 * 40), (256, 100, 5000)))
def test_encode_is_the_chain_restated_with_torch_stft(n_fft, hop, n):
    """x / max |x| -> stft(center, reflect) -> |X|^2 / sum w^2 -> fb^T D -> 10 log10(max(., 1e-12)), written out here in fp64."""
    fe = frontend(n_fft, hop)
    x = 0.37 * voiced(n, 3)
    x[10 * hop: 10 * hop + 3 * n_fft] = 0  # frames of digital silence: the clamp at 1e-12
    D_db, M_db = fe.encode(x, SR)
    frames = 1 + n // hop
    assert D_db.shape == (frames, n_fft // 2 + 1) and M_db.shape == (frames, 80) and D_db.dtype == torch.float64
    w = torch.hann_window(n_fft, dtype=torch.float64)
    X = torch.stft(x / x.abs().max(), n_fft, hop, n_fft, w, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    D = (X.real ** 2 + X.imag ** 2) / (w * w).sum()
    M = fe.fb.double().T @ D
    want_D, want_M = 10 * torch.log10(D.clamp(min=1e-12)), 10 * torch.log10(M.clamp(min=1e-12))
    assert float((D_db - want_D.T).abs().max()) <= 1e-9 and float((M_db - want_M.T).abs().max()) <= 1e-9
    assert abs(float(D_db.min()) + 120.0) < 1e-9 and abs(float(M_db.min()) + 120.0) < 1e-9
    # the fp32 form keeps its dtype, and the peak normalisation makes the result independent of the scale
    D32, M32 = fe.encode(x.float(), SR)
    assert D32.dtype == torch.float32 and M32.dtype == torch.float32
    assert torch.equal(fe.encode(4 * x, SR)[1], M_db)


def test_encode_refuses_another_sample_rate():
    fe = frontend()
    with pytest.raises(NotImplementedError, match="resampl"):
        fe.encode(voiced(4096, 1), SR + 1)


def test_encode_native_refuses_before_any_device_work():
    fe = frontend()
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        fe.encode_native(torch.zeros(2, 4096))
    with pytest.raises(NotImplementedError, match="exact fp32"):
        fe.encode_native(torch.zeros(2, 4096, dtype=torch.float64))
    with pytest.raises(_lib.DimsNotBuilt, match="768"):  # the dataclass default: needs a radix-3 pass
        A.AudioFrontend(A.AudioFrontendConfig()).encode_native(torch.zeros(2, 4096))
    with pytest.raises(_lib.DimsNotBuilt, match="hop_length"):
        frontend(1024, 513).encode_native(torch.zeros(2, 4096))
