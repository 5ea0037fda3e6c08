"""Inputs of the resampling plan tests (test_resample_plans_host.py checks them on the CPU, test_resample_plans_hip.py runs them on
the GPU): one rate pair per work layout that csrc/resample.hip can select.

The layout of a call - G blocks per workgroup along the lanes, R accumulators per work item (the template argument of
resample_kernel: 4, 2 or 1), how often G is halved once R is 1, the skewed LDS image, the run length L - is a function of the rate
pair, the filter width and the rolloff alone.  ``plan`` restates it, ``CASES`` names one pair per regime together with the plan it
is there for, and the host test asserts that the two agree: a change to the planning that moves a row out of its regime fails
there instead of silently un-testing the regime.

Every oracle result is computed once per process (functools.lru_cache) and never written to."""
import functools
import math
import struct
from typing import NamedTuple

import torch

import torch_tts_amd as T

A = T.audio
THREADS = 256        # kThreads
MAX_R = 4            # kMaxR
WINDOW_CAP = 32768   # kWindowCap: staged samples per workgroup
ODD_ROLLOFF = 0.9475937167399596  # no 7-digit decimal: the C side rebuilds 0.9475937 from the float, the oracle takes the double


class Plan(NamedTuple):
    o: int
    n: int
    width: int
    taps: int
    L: int
    G: int
    R: int
    halvings: int
    window: int
    skew: int
    items: int      # n * G work items per tile
    tile_in: int    # G * R * o input samples per tile
    lds_bytes: int
    h: float        # lpw * o / base, as the C side has it


def c_rolloff(rolloff):
    """What the C side makes of a rolloff: the double rounded to a float at the ABI, printed with %.7g and read back."""
    as_float = struct.unpack("f", struct.pack("f", rolloff))[0]
    return float("%.7g" % as_float)


def plan(orig, new, lpw=6, rolloff=0.99):
    """csrc/resample.hip make_plan, line for line (keep the two together)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    assert o != n and o <= 1024 and n <= 1024
    base = float(min(o, n)) * c_rolloff(rolloff)
    h = float(lpw) * o / base
    width = math.ceil(h)
    taps = 2 * width + o
    assert taps <= 16384
    L = min(math.ceil(2.0 * h) + 3, taps)
    G = 1 if n >= THREADS else (THREADS + n - 1) // n
    R, halvings = MAX_R, 0
    while (G * R - 1) * o + taps > WINDOW_CAP:
        if R > 1:
            R >>= 1
        else:
            G = (G + 1) // 2
            halvings += 1
    window = (G * R - 1) * o + taps
    skew = int(n == 1 and o % 4 == 0)
    return Plan(o, n, width, taps, L, G, R, halvings, window, skew, n * G, G * R * o, 4 * (window + (window // 32 + 1 if skew else 0)), h)


def band_lo(p, o, n, width, h):
    """csrc/resample.hip band_lo: the first tap of phase p's run."""
    return max(0, math.floor(float(width) + float(o) * float(p) / float(n) - h) - 1)


class Case(NamedTuple):
    orig: int   # the reduced pair
    new: int
    lpw: int
    rolloff: float
    G: int
    R: int
    halvings: int
    skew: int
    items: int
    taps: int
    L: int
    why: str

    @property
    def id(self):
        return f"{self.orig}-{self.new}" + ("" if (self.lpw, self.rolloff) == (6, 0.99) else f"-lpw{self.lpw}")

    @property
    def filter(self):
        return dict(lowpass_filter_width=self.lpw, rolloff=self.rolloff)


def _c(orig, new, G, R, halvings, skew, items, taps, L, why, lpw=6, rolloff=0.99):
    return Case(orig, new, lpw, rolloff, G, R, halvings, skew, items, taps, L, why)


CASES = [
    _c(48, 1, 256, 2, 0, 1, 256, 630, 585, "<2> with the skewed image"),
    _c(33, 1, 256, 2, 0, 0, 256, 433, 403, "<2>, odd o, no skew"),
    _c(100, 3, 86, 2, 0, 0, 258, 506, 408, "<2>, second item pass of 2 lanes"),
    _c(300, 7, 37, 2, 0, 0, 259, 820, 523, "<2>, n = 7"),
    _c(66, 1, 256, 1, 0, 0, 256, 866, 803, "<1>, no halving"),
    _c(128, 1, 128, 1, 1, 1, 128, 1680, 1555, "<1>, one halving, skew"),
    _c(1000, 3, 22, 1, 2, 0, 66, 5042, 4044, "<1>, two halvings, 66 of 256 threads live"),
    _c(1024, 1, 16, 1, 4, 1, 16, 13438, 12416, "the longest chain, the largest LDS (116 KiB)"),
    _c(441, 160, 2, 4, 0, 0, 320, 475, 37, "G = 2: the 44.1 -> 16 kHz pair"),
    _c(160, 147, 2, 4, 0, 0, 294, 174, 17, "48 -> 44.1 kHz"),
    _c(147, 160, 2, 4, 0, 0, 320, 161, 16, "44.1 -> 48 kHz"),
    _c(255, 64, 4, 4, 0, 0, 256, 305, 52, "G = 4"),
    _c(7, 5, 52, 4, 0, 0, 260, 25, 20, "lanes along blocks, ragged last pass"),
    _c(2, 3, 86, 4, 0, 0, 258, 16, 16, "lanes along blocks, ragged last pass, L = taps"),
    _c(1024, 1023, 1, 4, 0, 0, 1023, 1038, 16, "four item passes, the largest table"),
    _c(1023, 1024, 1, 4, 0, 0, 1024, 1037, 16, "four full item passes"),
    _c(1, 1024, 1, 4, 0, 0, 1024, 15, 15, "window of 18 samples, tile_in = 4, no slack at the run's end"),
    _c(441, 160, 2, 4, 0, 0, 320, 535, 97, "other width; a rolloff that is no 7-digit decimal", lpw=16, rolloff=ODD_ROLLOFF),
    _c(441, 320, 1, 4, 0, 0, 320, 629, 190, "long runs at G = 1", lpw=64, rolloff=ODD_ROLLOFF),
    _c(3, 2, 128, 4, 0, 0, 256, 7, 6, "the smallest filter, rolloff at its upper bound", lpw=1, rolloff=1.0),
]
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def by_id(case_id):
    return CASES[IDS.index(case_id)]


def case_plan(c: Case):
    return plan(c.orig, c.new, c.lpw, c.rolloff)


def count(n, length, o):
    return -(-n * length // o)


def signal(o, N, seed):
    """Two slow tones below every pair's cutoff (the output keeps an amplitude of about 0.5 even at 1024 / 1) plus seeded noise,
    built in fp64 and rounded to fp32."""
    t = torch.arange(N, dtype=torch.float64) / o
    noise = torch.randn(N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x = 0.3 * torch.sin(2 * math.pi * 0.11 * t) + 0.2 * torch.cos(2 * math.pi * 0.031 * t + 1) + 0.05 * noise
    return x.to(torch.float32)


def n_samples(pl: Plan):
    """Three tiles, the last partly filled."""
    return 2 * pl.tile_in + 777


def lengths(pl: Plan, N):
    """The whole row; an end exactly on a tile boundary (the whole third tile takes the zero-fill branch); the last output just past
    and just before a tile boundary; shorter than any filter; nothing."""
    return [N, 2 * pl.tile_in, pl.tile_in + 1, pl.tile_in - 1, 1, 0]


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(wave [6, N] fp32, lengths, and per utterance the fp64 oracle and the fp32 yardstick - audio.resample on the CPU from the
    same fp32 samples; None for the empty utterance)."""
    c = by_id(case_id)
    pl = case_plan(c)
    N = n_samples(pl)
    lens = lengths(pl, N)
    wave = torch.stack([signal(pl.o, N, 1000 * CASES.index(c) + b) for b in range(len(lens))])
    ref64 = [A.resample(wave[b, :l].double(), c.orig, c.new, **c.filter) if l else None for b, l in enumerate(lens)]
    ref32 = [A.resample(wave[b, :l], c.orig, c.new, **c.filter) if l else None for b, l in enumerate(lens)]
    return wave, lens, ref64, ref32
