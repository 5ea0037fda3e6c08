"""Sample-rate conversion on the GPU (csrc/resample.hip through audio.resample_native, AudioFrontend.encode_native(sr=...) and
audio.xref_native) against audio.py's torch-op ``resample`` run in fp64 on the CPU from the same fp32 samples.  The margin of every
bar is the same torch-op code run in fp32 on the CPU, computed here on the same inputs and printed before it is asserted: 4 x, the
error being a count of roundings.  The HIP path is never compared with itself (except for bit-equality) nor with the
torch-op path on the GPU.  Parity with torchaudio itself stays unpinned (it is absent)."""
import functools
import math

import pytest
import torch

import torch_tts_amd as T
from test_analysis_hip import errors
from test_griffinlim_host import voiced

pytestmark = pytest.mark.gpu
A = T.audio
DEV = torch.device("cuda:0")
# 441 / 320: odd o, the big table; 320 / 441: even o = 320, upsampling; 3 / 1: one phase; 2 / 1: one phase, even o; 1 / 2;
# 4 / 1: the skewed LDS image
PAIRS = ((22050, 16000), (16000, 22050), (48000, 16000), (44100, 22050), (8000, 16000), (32000, 8000))
SR16 = 16000


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def count(n, length, o):
    return -(-n * length // o)


@functools.lru_cache(maxsize=None)
def case(orig, new):
    """The padded batch (fp32), its lengths - a full row, an exact multiple of o, one shorter than the filter's width - and per
    utterance the fp64 oracle and the fp32 yardstick, both torch ops on the CPU."""
    o, n = reduced(orig, new)
    N = 5 * o + 37 if o >= 147 else 4001
    lens = [N, 2 * o, 5]
    g = torch.Generator().manual_seed(orig + new)
    wave = torch.stack([0.37 * voiced(N, 7 + b) + 0.02 * torch.randn(N, generator=g, dtype=torch.float64) for b in range(3)]).to(torch.float32)
    ref64 = [A.resample(wave[b, :l].double(), orig, new) for b, l in enumerate(lens)]
    ref32 = [A.resample(wave[b, :l], orig, new) for b, l in enumerate(lens)]
    return wave, lens, ref64, ref32


def poisoned(wave, lens):
    """NaN at every sample past an utterance's length: nothing of it may reach the output."""
    w = wave.clone()
    for b, l in enumerate(lens):
        w[b, l:] = float("nan")
    return w


@pytest.mark.parametrize("orig,new", PAIRS)
def test_resample_native_against_the_fp64_restatement(orig, new):
    wave, lens, ref64, ref32 = case(orig, new)
    o, n = reduced(orig, new)
    out, lens_out = A.resample_native(wave.to(DEV), orig, new, lens)
    assert out.shape == (3, count(n, wave.shape[1], o)) and out.dtype == torch.float32 and out.is_cuda and lens_out.dtype == torch.int32
    assert lens_out.tolist() == [count(n, l, o) for l in lens]
    for b, l in enumerate(lens):
        m = count(n, l, o)
        y, y64, y32 = out[b, :m].double().cpu(), ref64[b], ref32[b].double()
        assert y64.numel() == m
        e = float((y - y64).abs().max() / y64.abs().max())
        e32 = float((y32 - y64).abs().max() / y64.abs().max())
        print(f"{orig} -> {new} ({o} / {n}), utterance {b}: {l} -> {m} samples, HIP {e:.3g} torch fp32 {e32:.3g} (ratio {e / e32:.2f})")
        assert e <= 4 * e32


@pytest.mark.parametrize("orig,new", PAIRS)
def test_lengths_guards_batch_invariance_and_determinism(orig, new):
    wave, lens, _, _ = case(orig, new)
    o, n = reduced(orig, new)
    clean = wave.to(DEV)
    out, lens_out = A.resample_native(clean, orig, new, lens)
    want = [count(n, l, o) for l in lens]
    assert lens_out.tolist() == want
    for b, m in enumerate(want):  # exact zeros at and past every count
        assert m == out.shape[1] or float(out[b, m:].abs().max()) == 0.0
        assert float(out[b, :m].abs().max()) > 0.0
    # samples past a length are never read
    dirty, _ = A.resample_native(poisoned(wave, lens).to(DEV), orig, new, lens)
    assert not bool(torch.isnan(dirty).any()) and torch.equal(dirty, out)
    # every utterance alone, its row cut to its length
    for b, l in enumerate(lens):
        alone, m = A.resample_native(clean[b, :l].contiguous(), orig, new)
        assert alone.shape == (want[b],) and int(m) == want[b]
        assert torch.equal(out[b, : want[b]], alone), (b, l)
    again, lens_again = A.resample_native(clean, orig, new, lens)
    assert torch.equal(again, out) and torch.equal(lens_again, lens_out)
    on_dev, lens_dev = A.resample_native(clean, orig, new, torch.tensor(lens, device=DEV))
    assert torch.equal(on_dev, out) and torch.equal(lens_dev, lens_out)
    none, lens_full = A.resample_native(clean, orig, new)
    assert lens_full.tolist() == [out.shape[1]] * 3 and torch.equal(none[0], out[0])


def test_equal_rates_lengths_refusals_and_the_status_word():
    wave, lens, _, _ = case(22050, 16000)
    x = wave.to(DEV)
    same, counts = A.resample_native(x, 16000, 16000, lens)
    assert same is x and counts.tolist() == lens and counts.dtype == torch.int32
    one, c1 = A.resample_native(x[0], 22050, 22050)
    assert one.shape == x[0].shape and int(c1) == x.shape[1]
    with pytest.raises(ValueError, match="lengths"):
        A.resample_native(x, 22050, 16000, [1, 2])
    with pytest.raises(ValueError, match="lengths"):
        A.resample_native(x, 22050, 16000, [x.shape[1] + 1, 2, 3])
    with pytest.raises(ValueError, match="exceeds"):  # what the host has not seen is refused through the status word
        A.resample_native(x, 22050, 16000, torch.tensor([x.shape[1] + 1, 2, 3], device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------
# the chain: 22 050 Hz audio into a 16 kHz front-end
# ---------------------------------------------------------------------------------------------------------------------------
def frontend16(device=None, dtype=torch.float32):
    fe = A.AudioFrontend(A.AudioFrontendConfig(sample_rate=SR16, hop_length=256, win_length=1024, num_mels=80, fmin=0, fmax=8000), device)
    fe.fb = fe.fb.to(dtype)
    return fe


@functools.lru_cache(maxsize=None)
def chain_case():
    """2 x about 0.4 s at 22 050 Hz, ragged; per utterance the chain's mel in fp64 and in fp32, torch ops on the CPU."""
    N = 8820 + 37
    lens = [N, 6001]
    wave = torch.stack([0.37 * voiced(N, 21 + b) for b in range(2)]).to(torch.float32)
    fe64, fe32 = frontend16(dtype=torch.float64), frontend16()
    ref64 = [fe64.encode(A.resample(wave[b, :l].double(), 22050, SR16), SR16)[1] for b, l in enumerate(lens)]
    ref32 = [fe32.encode(A.resample(wave[b, :l], 22050, SR16), SR16)[1] for b, l in enumerate(lens)]
    return wave, lens, ref64, ref32


def test_encode_native_with_sr_is_the_two_calls_chained():
    wave, lens, _, _ = chain_case()
    fe = frontend16(DEV)
    x = wave.to(DEV)
    D_db, M_db, frames = fe.encode_native(x, lens, sr=22050)
    y, ylens = A.resample_native(x, 22050, SR16, lens)
    D2, M2, f2 = fe.encode_native(y, ylens)
    assert torch.equal(D_db, D2) and torch.equal(M_db, M2) and torch.equal(frames, f2)
    assert frames.tolist() == [1 + count(320, l, 441) // 256 for l in lens]
    # the configured rate, or none, is the call without resampling
    D3, M3, f3 = fe.encode_native(y, ylens, sr=SR16)
    assert torch.equal(D3, D2) and torch.equal(M3, M2) and torch.equal(f3, f2)
    # one utterance, 1-D
    D1, M1, n1 = fe.encode_native(x[1, : lens[1]].contiguous(), sr=22050)
    assert int(n1) == int(frames[1]) and torch.equal(M1, M_db[1, : int(n1)]) and torch.equal(D1, D_db[1, : int(n1)])


def test_chain_parity_against_the_fp64_chain():
    wave, lens, ref64, ref32 = chain_case()
    fe = frontend16(DEV)
    _, M_db, frames = fe.encode_native(wave.to(DEV), lens, spectrogram=False, sr=22050)
    for b in range(2):
        tb = int(frames[b])
        assert ref64[b].shape == (tb, 80)
        p, d, share, silent = errors(M_db[b, :tb], ref64[b])
        p32, d32, share32, _ = errors(ref32[b], ref64[b])
        print(f"22050 -> 16000 -> mel, utterance {b}: {tb} frames: power HIP {p:.3g} torch fp32 {p32:.3g} (ratio {p / p32:.2f}); dB HIP {d:.3g} "
              f"torch fp32 {d32:.3g} (ratio {d / d32:.2f}); mask keeps {share:.3f}")
        assert int(silent.sum()) == 0 and share >= 0.9 and share32 >= 0.9  # (conditions on the input, not measurements)
        assert p <= 4 * p32
        assert d <= 4 * d32


def test_xref_native_is_m_fwd_of_the_mel_with_zeros_past_each_end():
    wave, lens, _, _ = chain_case()
    fe = frontend16(DEV)
    x = wave.to(DEV)
    xref, frames = A.xref_native(fe, x, lens, sr=22050)
    _, M_db, f2 = fe.encode_native(x, lens, spectrogram=False, sr=22050)
    assert xref.shape == M_db.shape and xref.dtype == torch.float32 and torch.equal(frames, f2)
    for b in range(2):
        tb = int(frames[b])
        assert torch.equal(xref[b, :tb], A.m_fwd(M_db[b, :tb]))
        assert float(xref[b, :tb].min()) >= 0.0 and float(xref[b, :tb].max()) > 0.5
        if tb < xref.shape[1]:
            assert float(xref[b, tb:].abs().max()) == 0.0
    assert int(frames[1]) < xref.shape[1]  # (the batch is ragged: the mask has work to do)
    # at the configured rate it is the analysis alone, and 1-D input keeps the reference's 2-D shape
    y, ylens = A.resample_native(x, 22050, SR16, lens)
    x2, f3 = A.xref_native(fe, y, ylens)
    assert torch.equal(x2, xref) and torch.equal(f3, frames)
    x1, n1 = A.xref_native(fe, x[1, : lens[1]].contiguous(), sr=22050)
    assert x1.shape == (int(frames[1]), 80) and int(n1) == int(frames[1]) and torch.equal(x1, xref[1, : int(n1)])
