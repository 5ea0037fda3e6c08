"""Host-side checks of the resampling plan cases (tests/resample_plan_cases.py; csrc/resample.hip): the replica of the planning gives
the table's rows, the rows cover every work layout the kernel has, the replica's table size is the library's, the premise of the
run-relative table (every rounded tap outside a phase's run is an exact zero) holds on the oracle's own kernel, and the inputs
keep the output's peak near 0.5.  No GPU."""
import math

import pytest
import torch

import resample_plan_cases as K
import torch_tts_amd as T

A = T.audio


@pytest.mark.parametrize("c", K.CASES, ids=K.IDS)
def test_the_replica_of_the_plan_gives_the_table(c):
    pl = K.case_plan(c)
    assert (pl.o, pl.n) == (c.orig, c.new), "the table holds reduced pairs"
    got = dict(G=pl.G, R=pl.R, halvings=pl.halvings, skew=pl.skew, items=pl.items, taps=pl.taps, L=pl.L)
    want = dict(G=c.G, R=c.R, halvings=c.halvings, skew=c.skew, items=c.items, taps=c.taps, L=c.L)
    assert got == want, c.why
    assert pl.items == pl.n * pl.G and pl.tile_in == pl.G * pl.R * pl.o and pl.window == (pl.G * pl.R - 1) * pl.o + pl.taps
    assert pl.window <= K.WINDOW_CAP and pl.L <= pl.taps
    # the oracle's own sizes (from the rolloff as a double) are the replica's (from the float's 7-digit decimal)
    o, n, _, width, taps = A._resample_plan(c.orig, c.new, c.lpw, c.rolloff, "test")
    assert (o, n, width, taps) == (pl.o, pl.n, pl.width, pl.taps)


def test_the_rows_cover_every_layout():
    plans = [K.case_plan(c) for c in K.CASES]
    assert {p.R for p in plans} == {1, 2, 4}
    assert {min(p.halvings, 2) for p in plans} == {0, 1, 2}
    assert all(p.R == 1 for p in plans if p.halvings)
    assert any(p.skew and p.R == 2 for p in plans) and any(p.skew and p.R == 1 for p in plans)  # (R = 4: 4 / 1 in test_resample_hip.py)
    assert any(p.G == 1 for p in plans) and any(1 < p.G <= 4 for p in plans)
    assert any(p.G > 4 and p.items % K.THREADS for p in plans)  # lanes along blocks, a ragged last item pass
    assert any(p.items > 2 * K.THREADS for p in plans)  # more than two item passes
    assert any(p.items < K.THREADS for p in plans)  # idle threads
    assert any(p.L == p.taps for p in plans)
    assert any(c.lpw != 6 for c in K.CASES) and any(K.c_rolloff(c.rolloff) != c.rolloff for c in K.CASES)
    # the dynamic LDS: within the 160 KiB of a workgroup everywhere, and past the 64 KiB default limit somewhere
    assert all(p.lds_bytes <= 160 * 1024 for p in plans)
    assert max(p.lds_bytes for p in plans) > 64 * 1024
    print("LDS bytes:", {c.id: p.lds_bytes for c, p in zip(K.CASES, plans)})


def test_the_replica_of_the_plan_sizes_the_table_as_the_library_does():
    eng = T.Engine(T.EngineDims(), None)
    try:
        for c in K.CASES:
            pl = K.case_plan(c)
            got = eng._lib.ttsdec_resample_workspace_bytes(eng._h, c.orig, c.new, c.lpw, c.rolloff)
            assert got == (4 * pl.n * pl.taps + 255) // 256 * 256, c.id
    finally:
        eng.close()


def oracle_kernel(c):
    """audio.resample's polyphase kernel [n, taps]: its lines, in fp64, rounded once to fp32."""
    o, n, base, width, taps = A._resample_plan(c.orig, c.new, c.lpw, c.rolloff, "test")
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = (t * base).clamp(-c.lpw, c.lpw)
    window = torch.cos(t * math.pi / c.lpw / 2) ** 2
    t = t * math.pi
    kernel = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * (window * (base / o))
    return kernel.to(torch.float32)


@pytest.mark.parametrize("c", K.CASES, ids=K.IDS)
def test_every_rounded_tap_outside_a_phases_run_is_an_exact_zero(c):
    """What lets the kernel sum over [band_lo(p), band_lo(p) + L) alone.  The run comes from the C side's h, the kernel from the
    oracle's rolloff.  The slack is the count of exact zeros inside the run, below and above its non-zero taps."""
    pl = K.case_plan(c)
    k32 = oracle_kernel(c)
    assert k32.shape == (pl.n, pl.taps)
    # the restated kernel is audio.resample's: an impulse at sample j gives column j of it (conv1d is exact on a single product)
    x = torch.zeros(2 * pl.o, dtype=torch.float32)
    x[pl.o - 1] = 1.0
    y = A.resample(x, c.orig, c.new, **c.filter)
    for blk in range(2):
        k = pl.o - 1 + pl.width - blk * pl.o
        if 0 <= k < pl.taps:
            assert torch.equal(y[blk * pl.n:(blk + 1) * pl.n], k32[:, k])
    nz = k32 != 0
    taps = torch.arange(pl.taps)
    first = torch.where(nz, taps, pl.taps).min(dim=1).values
    last = torch.where(nz, taps, -1).max(dim=1).values
    lo = torch.tensor([K.band_lo(p, pl.o, pl.n, pl.width, pl.h) for p in range(pl.n)])
    below, above = first - lo, lo + pl.L - 1 - last
    clipped = int((lo + pl.L > pl.taps).sum())
    print(f"{c.id}: {pl.n} phases, L = {pl.L} of {pl.taps} taps: slack below {int(below.min())} - {int(below.max())}, above "
          f"{int(above.min())} - {int(above.max())} taps; {clipped} runs end at the last tap")
    assert bool(nz.any(dim=1).all())
    assert int(below.min()) >= 0 and int(above.min()) >= 0


@pytest.mark.parametrize("c", K.CASES, ids=K.IDS)
def test_the_inputs_keep_the_output_near_half_scale(c):
    """A condition on the inputs, not a measurement: the relative metric of the parity test divides by this peak."""
    pl = K.case_plan(c)
    wave, lens, ref64, ref32 = K.inputs(c.id)
    N = K.n_samples(pl)
    assert wave.shape == (6, N) and wave.dtype == torch.float32 and lens == [N, 2 * pl.tile_in, pl.tile_in + 1, pl.tile_in - 1, 1, 0]
    peaks = []
    for b, l in enumerate(lens):
        if not l:
            assert ref64[b] is None
            continue
        assert ref64[b].dtype == torch.float64 and ref32[b].dtype == torch.float32 and ref64[b].numel() == K.count(pl.n, l, pl.o)
        peaks.append(float(ref64[b].abs().max()))
        if l >= pl.tile_in - 1:
            assert peaks[-1] >= 0.3, (b, l)
    e32 = [float((ref32[b].double() - ref64[b]).abs().max() / ref64[b].abs().max()) for b, l in enumerate(lens) if l]
    print(f"{c.id}: N = {N}, max|y64| " + " ".join(f"{v:.3g}" for v in peaks) + "; torch fp32 beside fp64 " + " ".join(f"{v:.2g}" for v in e32))
