"""Every work layout a rate pair can select in csrc/resample.hip (tests/resample_plan_cases.py: the three instantiations of
resample_kernel, the halving of G, the skewed LDS image at R = 2 and 1, 1 < G < 86, ragged and many item passes, L = taps, other
filter widths and rolloffs) against audio.py's torch-op ``resample`` run in fp64 on the CPU from the same fp32 samples.  The bar is
test_resample_hip.py's: 4 x the error of the same torch-op code run in fp32 on the CPU, computed here on the same inputs and printed
before it is asserted.  Beside parity: counts, guards and bit-equality as there, and that a sum does not depend on the tile or the
(g, r) position its output falls in - the same utterance behind k o zeros gives the same bits k n outputs later."""
import functools

import pytest
import torch

import resample_plan_cases as K
import torch_tts_amd as T
from hip_helpers import assert_workspace_fits
from test_analysis_hip import errors
from test_griffinlim_host import voiced
from test_resample_hip import SR16, count, frontend16, poisoned
from torch_tts_amd.engine import Handle

pytestmark = pytest.mark.gpu
A = T.audio
DEV = torch.device("cuda:0")
cases = pytest.mark.parametrize("c", K.CASES, ids=K.IDS)


def native(c, wave, lengths=None):
    return A.resample_native(wave, c.orig, c.new, lengths, **c.filter)


@cases
def test_parity_against_the_fp64_restatement(c):
    wave, lens, ref64, ref32 = K.inputs(c.id)
    pl = K.case_plan(c)
    out, lens_out = native(c, wave.to(DEV), lens)
    assert out.shape == (len(lens), count(pl.n, wave.shape[1], pl.o)) and out.dtype == torch.float32 and lens_out.dtype == torch.int32
    assert lens_out.tolist() == [count(pl.n, l, pl.o) for l in lens]
    for b, l in enumerate(lens):
        if not l:
            continue
        m = count(pl.n, l, pl.o)
        y, y64, y32 = out[b, :m].double().cpu(), ref64[b], ref32[b].double()
        assert y64.numel() == m
        e = float((y - y64).abs().max() / y64.abs().max())
        e32 = float((y32 - y64).abs().max() / y64.abs().max())
        print(f"{c.id} (G {pl.G} R {pl.R} halvings {pl.halvings} skew {pl.skew} L {pl.L}), utterance {b}: {l} -> {m} samples, HIP {e:.3g} "
              f"torch fp32 {e32:.3g} (ratio {e / e32 if e32 else float('inf'):.2f})")
        assert e <= 4 * e32


@cases
def test_counts_guards_batch_invariance_and_determinism(c):
    wave, lens, _, _ = K.inputs(c.id)
    pl = K.case_plan(c)
    clean = wave.to(DEV)
    out, lens_out = native(c, clean, lens)
    want = [count(pl.n, l, pl.o) for l in lens]
    assert lens_out.tolist() == want and want[-1] == 0 and want[0] == out.shape[1]
    for b, m in enumerate(want):  # exact zeros at and past every count; the whole row for the empty utterance
        assert m == out.shape[1] or float(out[b, m:].abs().max()) == 0.0
        assert m == 0 or float(out[b, :m].abs().max()) > 0.0
    # samples past a length are never read
    dirty, _ = native(c, poisoned(wave, lens).to(DEV), lens)
    assert not bool(torch.isnan(dirty).any()) and torch.equal(dirty, out)
    # every utterance alone, its row cut to its length: another n_out, another grid
    for b, l in enumerate(lens):
        if not l:
            continue
        alone, m = native(c, clean[b, :l].contiguous())
        assert alone.shape == (want[b],) and int(m) == want[b]
        assert torch.equal(out[b, : want[b]], alone), (b, l)
    again, lens_again = native(c, clean, lens)
    assert torch.equal(again, out) and torch.equal(lens_again, lens_out)
    on_dev, lens_dev = native(c, clean, torch.tensor(lens, device=DEV))
    assert torch.equal(on_dev, out) and torch.equal(lens_dev, lens_out)


@cases
def test_a_sum_does_not_depend_on_its_tile_position(c):
    """k o zero samples in front move every output by k n places and change nothing else: a leading fmaf(kv, 0, acc) leaves acc as it
    is.  k = 1 moves every block to the next g (or r) of its tile, k = G R - 1 moves all but one block of a tile into the next."""
    wave, lens, _, _ = K.inputs(c.id)
    pl = K.case_plan(c)
    x = wave[0].to(DEV)
    base, m = native(c, x)
    assert int(m) == base.numel()
    for k in sorted({1, pl.G * pl.R - 1}):
        shifted, ms = native(c, torch.cat([torch.zeros(k * pl.o, device=DEV), x]))
        assert int(ms) == k * pl.n + base.numel() == shifted.numel()
        same = shifted[k * pl.n:] == base
        assert bool(same.all()), (k, int((~same).sum()), int((~same).nonzero()[0]))


@pytest.mark.parametrize("case_id", ["48-1", "128-1"])
def test_the_status_word_of_the_smaller_instantiations(case_id):
    c = K.by_id(case_id)
    wave, lens, _, _ = K.inputs(case_id)
    N = wave.shape[1]
    with pytest.raises(ValueError, match="exceeds"):
        native(c, wave.to(DEV), torch.tensor([N + 1] + lens[1:], device=DEV))


@pytest.mark.parametrize("case_id", ["441-160", "128-1"])
def test_a_short_n_out_keeps_the_prefix(case_id):
    """Engine.resample with less room than the longest utterance needs: the stores are guarded by j < n_out, every row is the prefix
    of the full result, the counts are clamped, and the status word says so."""
    c = K.by_id(case_id)
    wave, lens, _, _ = K.inputs(case_id)
    pl = K.case_plan(c)
    clean = wave.to(DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    full, counts = native(c, clean, lens)
    n_out = full.shape[1] - (pl.n + 1)
    assert 0 < n_out < int(counts[0])
    eng = A._engine(DEV)
    args = (clean, lens_dev, c.orig, c.new, c.lpw, c.rolloff, n_out)
    short, short_counts = eng.resample(*args)
    assert short.shape == (len(lens), n_out)
    assert torch.equal(short, full[:, :n_out])
    assert short_counts.tolist() == [min(int(m), n_out) for m in counts.tolist()]
    with pytest.raises(ValueError, match="exceeds"):
        eng.resample(*args, check=True)
    fits, _ = eng.resample(clean, lens_dev, c.orig, c.new, c.lpw, c.rolloff, full.shape[1], check=True)
    assert torch.equal(fits, full)


@pytest.mark.parametrize("case_id", ["1024-1", "1024-1023"])
def test_the_table_fits_its_workspace(monkeypatch, case_id):
    c = K.by_id(case_id)
    wave, lens, _, _ = K.inputs(case_id)
    clean = wave.to(DEV)
    want, _ = native(c, clean, lens)
    got = []

    def run():
        got.append(native(c, clean, lens)[0])
        return got[-1]

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)
    assert torch.equal(got[0], want)


# ---------------------------------------------------------------------------------------------------------------------------
# the chain at the common pair: 44 100 Hz audio into a 16 kHz front-end (G = 2)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case():
    """2 x about 0.4 s at 44 100 Hz, ragged; per utterance the chain's mel in fp64 and in fp32, torch ops on the CPU."""
    N = 17640 + 37
    lens = [N, 12001]
    wave = torch.stack([0.37 * voiced(N, 31 + b) for b in range(2)]).to(torch.float32)
    fe64, fe32 = frontend16(dtype=torch.float64), frontend16()
    ref64 = [fe64.encode(A.resample(wave[b, :l].double(), 44100, SR16), SR16)[1] for b, l in enumerate(lens)]
    ref32 = [fe32.encode(A.resample(wave[b, :l], 44100, SR16), SR16)[1] for b, l in enumerate(lens)]
    return wave, lens, ref64, ref32


def test_chain_parity_at_44100_against_the_fp64_chain():
    wave, lens, ref64, ref32 = chain_case()
    fe = frontend16(DEV)
    x = wave.to(DEV)
    D_db, M_db, frames = fe.encode_native(x, lens, sr=44100)
    assert frames.tolist() == [1 + count(160, l, 441) // 256 for l in lens]
    for b in range(2):
        tb = int(frames[b])
        assert ref64[b].shape == (tb, 80)
        p, d, share, silent = errors(M_db[b, :tb], ref64[b])
        p32, d32, share32, _ = errors(ref32[b], ref64[b])
        print(f"44100 -> 16000 -> mel, utterance {b}: {tb} frames: power HIP {p:.3g} torch fp32 {p32:.3g} (ratio {p / p32:.2f}); dB HIP {d:.3g} "
              f"torch fp32 {d32:.3g} (ratio {d / d32:.2f}); mask keeps {share:.3f}")
        assert int(silent.sum()) == 0 and share >= 0.9 and share32 >= 0.9  # (conditions on the input, not measurements)
        assert p <= 4 * p32
        assert d <= 4 * d32
    # the chained call is the two calls, bit for bit
    y, ylens = A.resample_native(x, 44100, SR16, lens)
    D2, M2, f2 = fe.encode_native(y, ylens)
    assert torch.equal(D_db, D2) and torch.equal(M_db, M2) and torch.equal(frames, f2)
