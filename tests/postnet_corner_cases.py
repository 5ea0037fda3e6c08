"""The corners of the dims that ttsdec_create accepts for the Tacotron Postnets (MelPostnet: any odd kernel >= 1, hidden and d_mel
multiples of 4, 1 to 8 layers; MelPostnet2: the same with kernel 5) and ttsenc_create for Encoder2 (d_emb % 4 == 0, d_out % 8 == 0)
that no other test runs: one table per family, shared by tests/golden/make_golden_postnet_corners.py (which runs the REFERENCE's
modules on them), tests/test_postnet_corners_host.py and tests/test_postnet_corners_hip.py, so that all three see the same cases.

Nothing here stores a weight: every module is filled from the case's seed by the oracle's own recipes
(O.random_postnet_weights / random_postnet2_weights / random_encoder2_weights) and load_state_dict; `ns` below is whichever
namespace holds the classes (the reference's modules in the golden script, torch_tts_amd in the tests).  The inputs are seeded too.

No shape of the issue's table had to be adjusted for the margin condition of test_postnet_corners_host.py (the fp32 oracle within
half of the bar from the fp64 oracle): it holds for every case and shape as listed."""
import torch

import recipes
from oracle import tacotron_oracle as O

GOLDEN_MAX_ELEMENTS = 100_000  # the golden file holds the reference's output of every shape up to this size

# ---------------------------------------------------------------------------------------------------------------------------
# MelPostnet (api.hip postnet_impl, decode_kernels.hip LoaderConv, conv256.hip): dims = (d_mel, hidden, kernel, layers)
# ---------------------------------------------------------------------------------------------------------------------------
MEL_CASES = {
    # 1 tap: no window, no padding; the hidden layers are conv256's (Cin = N = 512) with nk = Cin / kBK steps
    "M1": dict(dims=(80, 512, 1, 3), shapes=[(3, 57)], seed=101),
    # layer 0 on conv256 with Cin = 128 != N = 256 (128 * 4 % 128 == 0; in bf16 too); one column tile; (128, 600): 76 800 rows =
    # whole 256-row tiles plus a short round at 256 CUs
    "M2": dict(dims=(128, 256, 3, 2), shapes=[(3, 131), (2, 1), (128, 600)], seed=102),
    # three column tiles in the XCD order (ct = j % 3); (40, 600) = 24 000 rows > 85 * 256: whole tiles run
    "M3": dict(dims=(80, 768, 7, 2), shapes=[(2, 150), (40, 600)], seed=103),
    # conv256's largest taps; T = 5 and T = 1 are below taps / 2 = 7: every row's window is clipped on both sides
    "M4": dict(dims=(80, 256, 15, 2), shapes=[(3, 5), (2, 1), (2, 40)], seed=104),
    # taps > 15: conv256 refuses even when forced; the shared tile's descriptor base lies 8 frames in front of x
    "M5": dict(dims=(80, 256, 17, 2), shapes=[(2, 40), (3, 7)], seed=105),
    # one layer; hidden % 8 == 4: 16-bit requests stay on exact fp32
    "M6": dict(dims=(20, 36, 3, 1), shapes=[(3, 37)], seed=106),
    # kMaxPostnetLayers; d_mel % 8 == 4 (fp32 in every mode); Cin = 12 and 40: a 32-k tile straddles taps
    "M7": dict(dims=(12, 40, 9, 8), shapes=[(3, 37), (2, 3)], seed=107),
    # the smallest handle create accepts
    "M8": dict(dims=(4, 4, 1, 1), shapes=[(2, 9)], seed=108),
    # the smallest dims that still take the 16-bit planes (one 16-byte column per tap)
    "M9": dict(dims=(8, 8, 5, 3), shapes=[(3, 37)], seed=109),
    # a ragged last column tile (136 = 128 + 8 = 2 * 64 + 8); 2107 rows: the 16-bit 128 x 128 tile (N >= 128, M >= 2048), fp32 on
    # the 32 x 32 split-K tile (33 x 3 = 99 64-tiles < 512); 10 963 rows: 172 x 3 = 516 >= 512, the fp32 64 x 64 tile
    "M10": dict(dims=(80, 136, 3, 2), shapes=[(7, 301), (19, 577)], seed=110),
}

# ---------------------------------------------------------------------------------------------------------------------------
# MelPostnet2: dims = (d_in, hidden, layers); the kernel is the module's fixed 5
# ---------------------------------------------------------------------------------------------------------------------------
MEL2_CASES = {
    "Q1": dict(dims=(4, 4, 1), shapes=[(2, 9), (2, 1)], seed=201),
    "Q2": dict(dims=(12, 36, 2), shapes=[(3, 37), (2, 2)], seed=202),  # (d_in | hidden) & 7: fp32 in every mode
    "Q3": dict(dims=(8, 136, 8), shapes=[(3, 37)], seed=203),          # kMaxPostnetLayers, a ragged column tile, the planes
    "Q4": dict(dims=(128, 256, 1), shapes=[(3, 131)], seed=204),
    "Q5": dict(dims=(80, 136, 2), shapes=[(7, 301)], seed=205),        # 2107 rows: the 16-bit 128 x 128 tile
}

# ---------------------------------------------------------------------------------------------------------------------------
# Encoder2: dims = (alphabet, d_emb, d_out); every case runs ENC_SHAPES = (B, L, lengths)
# ---------------------------------------------------------------------------------------------------------------------------
ENC_CASES = {
    "E1": dict(dims=(5, 4, 8), seed=301),      # the smallest
    "E2": dict(dims=(40, 36, 72), seed=302),   # d_emb % 8 == 4: a split-fp16 request stays on exact fp32
    "E3": dict(dims=(40, 68, 24), seed=303),   # d_out < d_emb; no multiple of 64
    "E4": dict(dims=(300, 8, 136), seed=304),
}
ENC_SHAPES = [(3, 23, [23, 1, 2]), (2, 1, [1, 1]), (2, 5, [2, 2])]  # L = 1 and lengths 1, 2: below the conv's reach of 2; L_out < L

FAMILIES = {"mel": MEL_CASES, "mel2": MEL2_CASES}


def case(name):
    return MEL_CASES.get(name) or MEL2_CASES.get(name) or ENC_CASES[name]


def kind_of(name):
    return "mel" if name in MEL_CASES else "mel2" if name in MEL2_CASES else "enc"


def weights(name):
    """The case's oracle-style weight dict (fp32)."""
    c = case(name)
    if name in MEL_CASES:
        d_mel, hidden, k, layers = c["dims"]
        return O.random_postnet_weights(d_mel, hidden, layers, k=k, seed=c["seed"])
    if name in MEL2_CASES:
        d_in, hidden, layers = c["dims"]
        return O.random_postnet2_weights(d_in, hidden, layers, seed=c["seed"])
    return O.random_encoder2_weights(*c["dims"], seed=c["seed"])


def make_module(ns, name):
    """ns.MelPostnet / ns.MelPostnet2 / ns.Encoder2 at the case's dims with the case's weights, in eval mode."""
    c = case(name)
    if name in MEL_CASES:
        d_mel, hidden, k, layers = c["dims"]
        m = ns.MelPostnet(d_mel, dim_hidden=hidden, kernel_size=k, num_layers=layers)
    elif name in MEL2_CASES:
        d_in, hidden, layers = c["dims"]
        m = ns.MelPostnet2(d_in, dim_hidden=hidden, num_layers=layers)
    else:
        alphabet, d_emb, d_out = c["dims"]
        m = ns.Encoder2(alphabet, dim_out=d_out, dim_emb=d_emb)
    missing, unexpected = m.load_state_dict(weights(name), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (name, missing, unexpected)
    return m.eval()


def layers_of(name):
    return case(name)["dims"][-1]


def taps_of(name):
    return case(name)["dims"][2] if name in MEL_CASES else 5


def stays_fp32(name):
    """api.hip postnet_impl: `(d_mel | hidden) & 7` keeps a 16-bit request on exact fp32; encoder.hip: `E & 7` for split-fp16."""
    d = case(name)["dims"]
    return bool(d[1] & 7) if name in ENC_CASES else bool((d[0] | d[1]) & 7)


def postnet_input(name, B, T):
    """y [B, T, d_mel], seeded by the case and the shape."""
    c = case(name)
    return recipes.seeded_randn(1000 * c["seed"] + 7 * B + T, B, T, c["dims"][0])


def postnet_oracle(name, y, wts=None, dtype=torch.float32):
    """O.mel_postnet / O.mel_postnet2 on the case's weights in `dtype` (torch.float64: the tests' reference)."""
    wts = weights(name) if wts is None else wts
    f = O.mel_postnet if name in MEL_CASES else O.mel_postnet2
    return f(y.to(dtype), {k: v.to(dtype) for k, v in wts.items()}, layers_of(name))


def conv_layers(name):
    """[(Cin, N, taps)] of a MelPostnet case's conv layers (the fc layer is a plain GEMM)."""
    d_mel, hidden, k, layers = MEL_CASES[name]["dims"]
    return [(hidden if i else d_mel, hidden, k) for i in range(layers)]


def shared_tile(mode, M, N):
    """The tile decode_kernels.hip launch_gemm_cfg gives a Postnet layer [M, K] -> [M, N] that stays on the shared GEMM kernel - a
    restatement (tests/test_postnet_corners_host.py pins it to the dispatcher's source text):
        16-bit (split_f16, bf16):  N >= 128 && M >= 2048 -> "128x128", else "64x64"
        exact fp32:                M >= 64 && ceil(M / 64) * ceil(N / 64) >= 512 -> "64x64", else "32x32" (K split over four waves)"""
    if mode != "f32":
        return "128x128" if N >= 128 and M >= 2048 else "64x64"
    return "64x64" if M >= 64 and ((M + 63) // 64) * ((N + 63) // 64) >= 512 else "32x32"


LARGE_ROWS = 5000 # beyond this many frames the oracle runs on a sample of the utterances (they never interact)


def oracle_utterances(name, B, T, cus=256):
    """The utterances the oracle computes: all of them, or at the large shapes hip_helpers.sample_utterances' choice - the first,
    the last, the one holding row full * 256 of conv256's schedule on a device of `cus` CUs (where the short tiles begin), and two
    seeded others."""
    import hip_helpers as H

    if B * T <= LARGE_ROWS:
        return list(range(B))
    bounds = []
    if name in MEL_CASES:
        for cin, n, taps in conv_layers(name):
            sch = H.conv256_schedule(B * T, cus, Cin=cin, N=n, taps=taps, elem_bytes=4)
            if sch is not None and 0 < sch["full"] * 256 < B * T:
                bounds.append(sch["full"] * 256)
    return H.sample_utterances(B, T, bounds, k_random=2, seed=B)


# the ragged batches (forward(x, lengths=)): (B, T) per case
RAGGED_SHAPES = {"M4": (5, 40), "M5": (5, 40), "M7": (5, 37), "M10": (7, 301), "Q2": (5, 37), "Q3": (5, 37)}


def ragged_lengths(name):
    """T, 0, 1, one below taps / 2 and a value in between (M10's seven utterances: also T - 1 and 2)."""
    B, T = RAGGED_SHAPES[name]
    lengths = [T, 0, 1, max(taps_of(name) // 2 - 1, 0), T // 2 + 1, T - 1, 2][:B]
    assert len(lengths) == B
    return lengths


def ragged_input(name):
    """-> x [B, T, d] with 1e3 from each utterance's length on (what the padding holds must not matter), the lengths"""
    B, T = RAGGED_SHAPES[name]
    x = recipes.seeded_randn(1000 * case(name)["seed"] + 500, B, T, case(name)["dims"][0])
    lengths = ragged_lengths(name)
    for b, n in enumerate(lengths):
        x[b, n:] = 1e3
    return x, lengths


def in_golden(name, B, T):
    return B * T * case(name)["dims"][0] <= GOLDEN_MAX_ELEMENTS


def postnet_shapes(golden_only=False):
    """[(name, B, T)] over both Postnet tables."""
    return [(n, B, T) for table in (MEL_CASES, MEL2_CASES) for n, c in table.items() for B, T in c["shapes"]
            if not golden_only or in_golden(n, B, T)]


def encoder_input(name, i):
    """ids [B, L] (1 ... alphabet - 1, zero from each length on) and lengths [B] of ENC_SHAPES[i]."""
    c = ENC_CASES[name]
    B, L, lengths = ENC_SHAPES[i]
    ids = recipes.seeded_ids(1000 * c["seed"] + i, c["dims"][0], B, L, low=1)
    for b, n in enumerate(lengths):
        ids[b, n:] = 0
    return ids, torch.tensor(lengths)


def encoder_oracle(name, ids, lengths, wts=None, dtype=torch.float32):
    wts = weights(name) if wts is None else wts
    return O.encoder2(ids, lengths, {k: v.to(dtype) for k, v in wts.items()})
