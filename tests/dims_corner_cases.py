"""The corners of the dims that ttsgen_create, ttsdur_create / ttsvits_durnll_create and ttsvits_disc_create accept and that no
other test runs: one table per family, shared by tests/golden/make_golden_dims_corners.py (which runs the REFERENCE's modules on
them), tests/test_dims_corners_host.py and tests/test_dims_corners_hip.py, so that all three see the same cases.

Nothing here stores a weight: every module - the reference's in the golden script, the drop-in in the tests; `ns` below is
whichever namespace holds the classes - is filled from a seed, the generator and the discriminators by recipes.fill_by_key(module,
seed, gain), the duration nets by test_duration_host.randomize(module, seed).  The inputs are seeded too; the golden file keeps
them beside the reference's outputs."""
import torch

import recipes
from test_duration_host import randomize

# ---------------------------------------------------------------------------------------------------------------------------
# Generator (generator.hip dims_ok): gin_channels = 4, B = 2
# ---------------------------------------------------------------------------------------------------------------------------
GEN_GIN, GEN_B = 4, 2


def _gen(initial_channel, upsample_initial_channel, rates, res_kernels, dilations):
    return dict(initial_channel=initial_channel, resblock="1", resblock_kernel_sizes=res_kernels, resblock_dilation_sizes=dilations,
                upsample_rates=rates, upsample_initial_channel=upsample_initial_channel, upsample_kernel_sizes=[2 * u for u in rates])


GEN_CASES = {
    # odd u / 2 in the polyphase pack (u = 6, 10); C = 32, 16: one whole tap per 32-k tile, and two; 1 tap; 31 taps at dilation 3
    # and 5 taps at dilation 16, which reach past both ends of every utterance; even dilations
    "G1": dict(dims=_gen(8, 64, [6, 10], [1, 5, 31], [[1, 2, 4], [1, 16, 8], [3, 1, 1]]), T=[1, 5, 23], gain=1.2, seed=51),
    # n_res = 4 and u = 64; C = 8, 4 (one 16-byte column is one whole tap); the last stage is not the largest per frame.  In
    # split-fp16 a mixed handle in both orders: conv_pre (4 input channels) and the last stage (C = 4) stay exact, ups[0], stage 0
    # and ups[1] split
    "G2": dict(dims=_gen(4, 16, [2, 64], [3, 1, 9, 31], [[1, 3, 5], [2, 2, 2], [16, 1, 7], [1, 1, 4]]), T=[1, 9], gain=1.2, seed=52),
    # n_up = 8: C = 512 ... 4, every tap-walk regime inside one call; an initial_channel that is no multiple of 8.  gain 0.8: at 1.2
    # the waveform saturates (sat_frac 0.999) and the reference's own fp32 is 8.9 x the bar away from fp64
    "G3": dict(dims=_gen(12, 1024, [2] * 8, [5], [[2, 7, 16]]), T=[3], gain=0.8, seed=53),
}


def make_generator(ns, name):
    c = GEN_CASES[name]
    gen = ns.Generator(**c["dims"], gin_channels=GEN_GIN).eval()
    recipes.fill_by_key(gen, c["seed"], gain=c["gain"])
    return gen


def gen_inputs(name, T):
    """-> x [B, initial_channel, T], g [B, gin, 1]"""
    c = GEN_CASES[name]
    return recipes.seeded_randn(1000 * c["seed"] + T, GEN_B, c["dims"]["initial_channel"], T), recipes.seeded_randn(c["seed"], GEN_B, GEN_GIN, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# Duration predictors (duration.hip dims_ok): B = 3, T = 33, lengths 33 / 17 / 1 - M = 99 rows, seven 16-row tiles, the last one
# ragged, utterances starting at tile offsets 1 and 2
# ---------------------------------------------------------------------------------------------------------------------------
DUR_B, DUR_T, DUR_LENGTHS = 3, 33, [33, 17, 1]
DUR_NOISE_SCALE = 2.0  # as in the golden case of make_golden_duration.py: the inverse spline sees inputs outside its tails
DUR_EQ_SCALE = 3.0     # the likelihood's draw, as test_durnll_hip.py's tails-and-clamp case scales it
SDP_CASES = {
    "D1": dict(C=4, n_flows=2, gin=0, seed=61),    # one column of a 16-byte row; fewer channels than a flow tail's 29 columns
    "D2": dict(C=256, n_flows=8, gin=4, seed=62),  # kMaxC, the most flows
    "D3": dict(C=68, n_flows=3, gin=0, seed=63),   # no multiple of 64: a ragged second pass over the lanes; an odd flow count
    "D4": dict(C=192, n_flows=5, gin=0, seed=64),  # the model's width at the other Flip parity
}
DP_CASES = {  # (C, F, gin)
    "DP1": dict(C=4, F=4, gin=0, seed=71),
    "DP2": dict(C=256, F=256, gin=4, seed=72),  # both convs exactly at pw_conv_kernel's 64 KiB of LDS
    "DP3": dict(C=68, F=36, gin=0, seed=73),
    "DP4": dict(C=8, F=256, gin=0, seed=74),
}


def make_sdp(ns, name):
    c = SDP_CASES[name]
    return randomize(ns.StochasticDurationPredictor(c["C"], 192, 3, 0.5, c["n_flows"], gin_channels=c["gin"]).eval(), c["seed"])


def make_dp(ns, name):
    c = DP_CASES[name]
    return randomize(ns.DurationPredictor(c["C"], c["F"], 3, 0.5, gin_channels=c["gin"]).eval(), c["seed"])


def dur_mask():
    return (torch.arange(DUR_T)[None, :] < torch.tensor(DUR_LENGTHS)[:, None]).unsqueeze(1).float()


def dur_inputs(c):
    """One case's operands (c: a row of SDP_CASES or DP_CASES): x [B, C, T] (padded frames zero), x_mask, g [B, gin, 1] or None, the
    reverse pass's noise [B, 2, T], and the likelihood's integer durations w [B, 1, T] and draw e_q [B, 2, T]."""
    gen = torch.Generator().manual_seed(100 * c["seed"])
    x_mask = dur_mask()
    x = torch.randn(DUR_B, c["C"], DUR_T, generator=gen) * x_mask
    g = torch.randn(DUR_B, c["gin"], 1, generator=gen) if c["gin"] else None
    noise = torch.randn(DUR_B, 2, DUR_T, generator=gen)
    # x noise_scale 2.0: inputs of the first inverse spline (channel 0 after the Flip) beyond the +-5 tails, and one on the top edge
    noise[0, 0, 1], noise[0, 0, 20], noise[1, 0, 3] = 3.1, -3.4, 2.8
    noise[2, 0, 0] = 2.5
    w = torch.randint(1, 13, (DUR_B, 1, DUR_T), generator=gen).float() * x_mask
    w[1, 0, 7] = 0.0  # an in-length token without a frame: Log's clamp
    e_q = torch.randn(DUR_B, 2, DUR_T, generator=gen) * DUR_EQ_SCALE
    return dict(x=x, x_mask=x_mask, g=g, noise=noise, w=w, e_q=e_q)


# ---------------------------------------------------------------------------------------------------------------------------
# DiscriminatorP (disc.hip ttsvits_disc_create): B = 2
# ---------------------------------------------------------------------------------------------------------------------------
DISC_B = 2
DISC_STRIDE = 13  # the feature-map samples of disc_meta.json
DISC_CASES = {
    "P1": dict(period=2, kernel_size=1, stride=1, T=64, gain=1.0, seed=81),     # no padding: no k window at all
    "P2": dict(period=3, kernel_size=15, stride=16, T=2311, gain=1.2, seed=82),  # H 49, 4, 1, 1, 1, 1: windows clipped on both sides, pad 7 > H
    "P3": dict(period=2, kernel_size=15, stride=1, T=96, gain=1.2, seed=83),    # 15 taps, the deep GEMMs at K = 15 360 over 192 rows
    "P4": dict(period=13, kernel_size=3, stride=2, T=521, gain=1.2, seed=84),   # reflect pad 12
    "P5": dict(period=1, kernel_size=5, stride=3, T=300, gain=1.2, seed=85),    # period 1
    "P6": dict(period=97, kernel_size=7, stride=5, T=823, gain=1.2, seed=86),   # a period larger than every H after layer 0
}


def make_disc(ns, name):
    c = DISC_CASES[name]
    disc = ns.DiscriminatorP(c["period"], c["kernel_size"], c["stride"]).eval()
    recipes.fill_by_key(disc, c["seed"], gain=c["gain"])
    return disc


def disc_input(name):
    c = DISC_CASES[name]
    return recipes.seeded_randn(1000 + c["seed"], DISC_B, 1, c["T"])
