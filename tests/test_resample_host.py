"""Host-side checks of sample-rate conversion (torch-tts_amd/audio.py ``resample`` / ``resample_native``, csrc/resample.hip):
``resample`` in fp64 against a plain double loop over the definition, the sample counts, a tone through the eight rate pairs, the
C-ABI declarations, exports and host-only refusals, and the Python refusals (all before any device work).  No GPU."""
import math
import os
import re

import pytest
import torch

import torch_tts_amd as T
from torch_tts_amd import _lib

A = T.audio
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ((22050, 16000), (48000, 16000), (16000, 22050), (44100, 22050), (8000, 16000), (44100, 16000), (32000, 22050), (24000, 16000))


def by_definition(x, orig, new, lpw=6, rolloff=0.99):
    """y[blk * n + p] = sum_k K[p, k] * xp[blk * o + k], every factor a Python float, over the same tap range."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    taps = 2 * width + o
    xs = [float(v) for v in x]
    xp = [0.0] * width + xs + [0.0] * (width + o)
    count = -(-n * len(xs) // o)
    y = []
    for j in range(count):
        blk, p = divmod(j, n)
        acc = 0.0
        for k in range(taps):
            t = max(-lpw, min(lpw, base * ((k - width) / o - p / n)))
            sinc = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            acc += (base / o) * math.cos(t * math.pi / lpw / 2) ** 2 * sinc * xp[blk * o + k]
        y.append(acc)
    return torch.tensor(y, dtype=torch.float64)


@pytest.mark.parametrize("orig,new", ((3, 2), (2, 3), (3, 1)))
def test_resample_fp64_is_the_definition_written_as_a_double_loop(orig, new):
    x = torch.randn(50, generator=torch.Generator().manual_seed(orig * 10 + new), dtype=torch.float64)
    got = A.resample(x, orig, new)
    want = by_definition(x, orig, new)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12
    # a common factor changes nothing, and leading dimensions are kept
    assert torch.equal(A.resample(x, orig * 8000, new * 8000), got)
    both = A.resample(torch.stack([x, -x]).reshape(2, 1, 50), orig, new)
    assert both.shape == (2, 1, got.numel()) and torch.equal(both[0, 0], got) and torch.equal(both[1, 0], -got)


@pytest.mark.parametrize("orig,new", PAIRS)
def test_sample_counts(orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    for L in (3 * o, 3 * o + 1, 2 * o + o // 2 + 1, 7):  # a multiple of o, and lengths that are not
        y = A.resample(torch.zeros(L, dtype=torch.float64), orig, new)
        assert y.numel() == -(-n * L // o) == math.ceil(n * L / o), (L, y.numel())


def test_equal_rates_return_the_input():
    x = torch.randn(2, 40)
    assert A.resample(x, 16000, 16000) is x
    assert A.resample(x, 16000, 16000, lowpass_filter_width=3, rolloff=0.5) is x
    with pytest.raises(ValueError, match="rolloff"):
        A.resample(x, 3, 2, rolloff=0.0)
    with pytest.raises(ValueError, match="lowpass_filter_width"):
        A.resample(x, 3, 2, lowpass_filter_width=0)
    with pytest.raises(ValueError, match="rates"):
        A.resample(x, 0, 2)


@pytest.mark.parametrize("orig,new", PAIRS)
def test_a_300_hz_tone_comes_back(orig, new):
    """A unit tone far below both Nyquist rates, sampled at one rate, is the same tone sampled at the other, within the filter's own
    ripple (at most 6.6e-4 over these pairs), over the middle half of the signal; the fp32 form stays beside the fp64 one."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    N = max(20 * o, 4000)
    x = torch.sin(2 * math.pi * 300 * torch.arange(N, dtype=torch.float64) / orig)
    y = A.resample(x, orig, new)
    M = y.numel()
    want = torch.sin(2 * math.pi * 300 * torch.arange(M, dtype=torch.float64) / new)
    mid = slice(M // 4, M - M // 4)
    err = float((y - want)[mid].abs().max())
    y32 = A.resample(x.float(), orig, new)
    e32 = float((y32.double() - y).abs().max() / y.abs().max())
    print(f"{orig} -> {new}: {o} / {n}, tone error {err:.3g}, fp32 beside fp64 {e32:.3g}")
    assert y32.dtype == torch.float32
    assert err <= 1e-3
    assert e32 <= 1e-6


def test_new_ttsdec_symbols_are_declared_bound_and_exported():
    new = ("ttsdec_resample_workspace_bytes", "ttsdec_resample")
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
    ws = lib.ttsdec_resample_workspace_bytes
    assert ws(h, 22050, 16000, 6, 0.99) == up(4 * 320 * 459)  # 441 / 320: width 9
    assert ws(h, 48000, 16000, 6, 0.99) == up(4 * 1 * 41)  # 3 / 1: width 19
    assert ws(h, 32000, 22050, 6, 0.99) == up(4 * 441 * (2 * 9 + 640))
    assert ws(h, 16001, 16000, 6, 0.99) == 0 and ws(h, 16000, 16001, 6, 0.99) == 0
    assert ws(h, 16000, 16000, 6, 0.99) == 0 and ws(h, 0, 16000, 6, 0.99) == 0 and ws(h, 16000, -1, 6, 0.99) == 0
    assert ws(h, 3, 2, 0, 0.99) == 0 and ws(h, 3, 2, 6, 0.0) == 0 and ws(h, 3, 2, 6, 1.5) == 0 and ws(h, 3, 2, 6, 1.0) == up(4 * 2 * 21)
    assert ws(h, 1000, 1, 8, 0.99) == 0  # 2 * 8081 + 1000 taps
    assert ws(None, 3, 2, 6, 0.99) == 0
    one, big = 256, 1 << 30  # (non-null placeholders: every call below is refused on the host)

    def call(B=1, N=4096, orig=22050, new=16000, lpw=6, rolloff=0.99, n_out=2973, handle=h, wave=one, out=one, wsp=one, wsb=big):
        return lib.ttsdec_resample(handle, wave, None, B, N, orig, new, lpw, rolloff, out, n_out, None, None, wsp, wsb, None)

    for kw in (dict(B=0), dict(N=0), dict(n_out=0), dict(orig=0), dict(new=-1), dict(orig=16000), dict(lpw=0), dict(rolloff=0.0),
               dict(rolloff=1.01), dict(rolloff=float("nan")), dict(handle=None)):
        assert call(**kw) == _lib.ERR_INVALID_ARG, kw
    for kw in (dict(orig=16001), dict(orig=16000, new=16001), dict(orig=1000, new=1, lpw=8), dict(B=65536), dict(N=(1 << 30) + 1),
               dict(n_out=(1 << 30) + 1)):
        assert call(**kw) == _lib.ERR_DIMS, kw
    # sizes before pointers, pointers before the workspace
    assert call(orig=16001, wave=None) == _lib.ERR_DIMS and call(B=0, out=None) == _lib.ERR_INVALID_ARG
    assert call(wave=None) == _lib.ERR_INVALID_ARG and call(out=None) == _lib.ERR_INVALID_ARG
    assert call(wave=None, wsb=16) == _lib.ERR_INVALID_ARG
    assert call(wsb=up(4 * 320 * 459) - 1) == _lib.ERR_WORKSPACE and call(wsp=None) == _lib.ERR_WORKSPACE and call(wsp=128) == _lib.ERR_WORKSPACE
    eng.close()


def test_resample_native_refuses_before_any_device_work():
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        A.resample_native(torch.zeros(2, 4096), 22050, 16000)
    with pytest.raises(NotImplementedError, match="exact fp32"):
        A.resample_native(torch.zeros(2, 4096, dtype=torch.float64), 22050, 16000)
    with pytest.raises(_lib.DimsNotBuilt, match="16001"):
        A.resample_native(torch.zeros(2, 4096), 16001, 16000)
    with pytest.raises(_lib.DimsNotBuilt, match="taps"):
        A.resample_native(torch.zeros(2, 4096), 1000, 1, lowpass_filter_width=8)
    with pytest.raises(ValueError, match="rolloff"):
        A.resample_native(torch.zeros(2, 4096), 3, 2, rolloff=2.0)
    # the chained form refuses in the same way, and encode itself still refuses another rate
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=16000, hop_length=256, win_length=1024, num_mels=80, fmin=0, fmax=8000))
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        fe.encode_native(torch.zeros(2, 4096), sr=22050)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        A.xref_native(fe, torch.zeros(2, 4096), sr=22050)
    with pytest.raises(NotImplementedError, match="resampl"):
        fe.encode(torch.zeros(4096), 22050)
