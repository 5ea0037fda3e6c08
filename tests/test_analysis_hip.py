"""The native waveform -> dB spectrogram / mel path on the GPU (csrc/analysis.hip through AudioFrontend.encode_native) against
audio.py's torch-op ``encode`` run in fp64 on the CPU from the same fp32 samples.  The margin of every bar is the same torch-op code
run in fp32 on the CPU, computed here on the same inputs and printed before it is asserted: 4 x, the error being a count of
roundings.  The HIP path is never compared with itself (except for bit-equality) nor with the torch-op path on the GPU.  Parity with
torchaudio itself stays unpinned (it is absent)."""
import functools

import pytest
import torch

import torch_tts_amd as T  # noqa: F401
from test_griffinlim_host import SR, frontend, voiced

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CONFIGS = ((1024, 256, 120), (512, 128, 90), (2048, 512, 70), (256, 64, 50), (1024, 200, 60))  # n_fft, hop, frames (200: no divisor of n_fft)


def signal(n_fft, hop, frames, seed=1):
    """A length that is no multiple of hop, a peak that is not 1, and nine frames of digital silence (ten at hop 200) (fp32)."""
    x = 0.37 * voiced(hop * (frames - 1) + 37, seed)
    x[20 * hop: 20 * hop + 3 * n_fft] = 0
    return x.to(torch.float32)


@functools.lru_cache(maxsize=None)
def case(n_fft, hop, frames):
    """The input, the fp64 oracle and the fp32 yardstick, both torch ops on the CPU: x, (D_db64, M_db64), (D_db32, M_db32)."""
    x = signal(n_fft, hop, frames)
    ref64 = frontend(n_fft, hop, dtype=torch.float64).encode(x.double(), SR)
    ref32 = frontend(n_fft, hop).encode(x, SR)
    return x, ref64, ref32


def errors(db, db64):
    """[T, n] dB each -> (power-domain error: max over non-silent frames of max_k |P - P64| / max_k P64; dB-domain error: max |dB -
    dB64| over the bins of those frames with P64 >= 1e-6 max_k P64; the share of their bins that mask keeps; the silent frames)."""
    db, db64 = db.detach().double().cpu(), db64.double()
    P, P64 = 10.0 ** (db / 10), 10.0 ** (db64 / 10)
    silent = db64.amax(1) <= -120.0 + 1e-9
    top = P64.amax(1, keepdim=True)
    e_pow = float(((P - P64).abs().amax(1) / top[:, 0])[~silent].max())
    mask = (P64 >= 1e-6 * top) & ~silent[:, None]
    e_db = float((db - db64).abs()[mask].max())
    return e_pow, e_db, float(mask.sum()) / float((~silent).sum() * db.shape[1]), silent


@pytest.mark.parametrize("n_fft,hop,frames", CONFIGS)
def test_encode_native_against_the_fp64_chain(n_fft, hop, frames):
    x, ref64, ref32 = case(n_fft, hop, frames)
    fe = frontend(n_fft, hop, device=DEV)
    D_db, M_db, n = fe.encode_native(x.to(DEV))
    assert D_db.shape == (frames, n_fft // 2 + 1) and M_db.shape == (frames, 80) and int(n) == frames == 1 + x.numel() // hop
    assert D_db.dtype == torch.float32 and M_db.dtype == torch.float32 and D_db.is_cuda
    for name, got, r64, r32 in (("D", D_db, ref64[0], ref32[0]), ("M", M_db, ref64[1], ref32[1])):
        p, d, share, silent = errors(got, r64)
        p32, d32, _, _ = errors(r32, r64)
        quiet = float((got.cpu()[silent] + 120.0).abs().max())
        print(f"{n_fft} / {hop}, {frames} frames, {name}: power HIP {p:.3g} torch fp32 {p32:.3g} (ratio {p / p32:.2f}); dB HIP {d:.3g} "
              f"torch fp32 {d32:.3g} (ratio {d / d32:.2f}); mask keeps {share:.3f}; {int(silent.sum())} silent frames, off -120 by {quiet:.3g}")
        assert int(silent.sum()) == (10 if hop == 200 else 9)
        assert share >= 0.9  # (a condition on the input, not a measurement)
        assert p <= 4 * p32
        assert d <= 4 * d32
        assert quiet <= 1e-4


@pytest.mark.parametrize("n_fft,hop,frames", CONFIGS)
def test_scale_invariance_mel_only_and_determinism(n_fft, hop, frames):
    x = case(n_fft, hop, frames)[0].to(DEV)
    fe = frontend(n_fft, hop, device=DEV)
    D_db, M_db, n = fe.encode_native(x)
    assert bool(torch.isfinite(D_db).all()) and bool(torch.isfinite(M_db).all()) and float(M_db.max()) > -60
    for s in (0.25, 4.0):  # the peak pass: x / max |x| is exact under a power of two
        D2, M2, n2 = fe.encode_native(s * x)
        assert torch.equal(D2, D_db) and torch.equal(M2, M_db) and int(n2) == int(n)
    none, M3, n3 = fe.encode_native(x, spectrogram=False)
    assert none is None and torch.equal(M3, M_db) and int(n3) == int(n)
    again = fe.encode_native(x)
    assert torch.equal(again[0], D_db) and torch.equal(again[1], M_db)


@pytest.mark.parametrize("B", (1, 5, 64))
def test_ragged_batch_is_each_utterance_alone_bit_for_bit(B):
    n_fft, hop, N = 1024, 256, 256 * 36 + 100
    T_ = 1 + N // hop
    g = torch.Generator().manual_seed(B)
    # the full row, the shortest legal, a multiple of hop, others; every row is signal to its end, so a length has to be honoured
    lens = [N, n_fft // 2 + 1, hop * 7, 5000, hop * 36][:B] + [int(v) for v in torch.randint(n_fft // 2 + 1, N + 1, (max(B - 5, 0),), generator=g)]
    wave = torch.stack([(0.2 + 0.01 * b) * voiced(N, 40 + b) for b in range(B)]).to(torch.float32).to(DEV)
    fe = frontend(n_fft, hop, device=DEV)
    D_db, M_db, frames = fe.encode_native(wave, lens)
    assert D_db.shape == (B, T_, 513) and M_db.shape == (B, T_, 80) and frames.dtype == torch.int32
    assert frames.tolist() == [1 + n // hop for n in lens]
    for b, n in enumerate(lens):
        D1, M1, f1 = fe.encode_native(wave[b, :n].contiguous())
        tb = 1 + n // hop
        assert int(f1) == tb and D1.shape == (tb, 513) and M1.shape == (tb, 80)
        assert torch.equal(D_db[b, :tb], D1) and torch.equal(M_db[b, :tb], M1), (b, n)
        if tb < T_:  # exact zeros past each end
            assert float(D_db[b, tb:].abs().max()) == 0.0 and float(M_db[b, tb:].abs().max()) == 0.0
    on_dev = fe.encode_native(wave, torch.tensor(lens, device=DEV))
    assert torch.equal(on_dev[0], D_db) and torch.equal(on_dev[1], M_db) and torch.equal(on_dev[2], frames)
    none, M2, f2 = fe.encode_native(wave, lens, spectrogram=False)
    assert none is None and torch.equal(M2, M_db) and torch.equal(f2, frames)
    if B == 5:  # what the host has not seen is refused through the status word
        dev_lens = lambda v: torch.tensor(v, device=DEV)  # noqa: E731
        with pytest.raises(ValueError, match="reflect"):
            fe.encode_native(wave, dev_lens([N, n_fft // 2, hop * 7, 5000, hop * 36]))
        with pytest.raises(ValueError, match="exceeds"):
            fe.encode_native(wave, dev_lens([N + 1, n_fft // 2 + 1, hop * 7, 5000, hop * 36]))
        silent = wave.clone()
        silent[3, :5000] = 0  # all zeros over the utterance's own samples (what follows them is not part of it)
        with pytest.raises(ValueError, match="all zeros"):
            fe.encode_native(silent, dev_lens(lens))
        with pytest.raises(ValueError, match="lengths"):
            fe.encode_native(wave, [N, n_fft // 2, hop * 7, 5000, hop * 36])
