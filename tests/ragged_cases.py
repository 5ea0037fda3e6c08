"""Inputs of the per-utterance stop rule's tests (test_ragged_host.py checks them on the CPU, test_ragged_hip.py runs them on
the GPU): decode cases whose oracle result - one run over the batch; rows never interact, so it is every row's result alone -
has stop steps spread the way the tests need, at a threshold that no stop logit comes near."""
import functools
from typing import NamedTuple

import torch

from oracle import tacotron_oracle as O

B, L, T = 37, 23, 44  # B: no tile multiple; T: more than one captured graph of steps
MEM_LENGTHS = [23] * 30 + [1, 2, 5, 9, 14, 20, 23]
PHILOX_SEED = 5
MARGIN = 1e-3  # no stop logit within this of the threshold: fp32 reordering on the GPU (1e-4 relative) cannot move a stop step


def stop_steps(s, thr):
    """s [B, T, r] stop logits -> (t_b [B], the first step with a logit below thr, or T where there is none; fire [B, T])."""
    fire = (s < thr).any(dim=2)
    first = torch.where(fire.any(dim=1), fire.to(torch.int64).argmax(dim=1), torch.full((s.shape[0],), s.shape[1]))
    return first, fire


def recrossing_rows(fire, t_last):
    """Rows that fire, stop firing and fire again, all at steps <= t_last (the steps a batched decode computes)."""
    rows = []
    for b in range(fire.shape[0]):
        f = fire[b, : t_last + 1].tolist()
        runs = [f[0]] + [f[i] for i in range(1, len(f)) if f[i] != f[i - 1]]  # run-length collapsed
        if sum(runs) >= 2:  # two separate runs of firing steps
            rows.append(b)
    return rows


def conditions(s, thr, r):
    """What keeps the GPU tests meaningful at threshold thr; every entry must be true (test_ragged_host.py asserts each)."""
    tb, fire = stop_steps(s, thr)
    t_all = int(tb.max())
    c = {
        "every row fires before step T - 2": t_all < T - 2,
        "no stop logit within MARGIN of the threshold": float((s - thr).abs().min()) >= MARGIN,
        "at least 4 distinct stop steps": tb.unique().numel() >= 4,
        "rows stop in at least 3 different chunks of 4 steps": (tb // 4).unique().numel() >= 3,
        "a row stops at step 0 or 1": int(tb.min()) <= 1,
        "a row's logit crosses, recrosses and crosses again": t_all < T and len(recrossing_rows(fire, t_all)) >= 1,
    }
    if r == 2 and t_all < T:
        both = (s[torch.arange(s.shape[0]), tb.clamp(max=T - 1)] < thr).all(dim=1)
        c["r = 2: a row with both logits of its firing step below the threshold"] = bool(both.any())
    return c


def cap_conditions(s, thr):
    tb, _ = stop_steps(s, thr)
    return {
        "cap case: a row never fires": bool((tb == T).any()),
        "cap case: a row fires": bool((tb < T).any()),
        "cap case: no stop logit within MARGIN of the threshold": float((s - thr).abs().min()) >= MARGIN,
    }


class Case(NamedTuple):
    dims: object
    wts: dict
    mem: torch.Tensor
    masks: object       # per step [2, B, d_pre]: the keep-masks of dropout_source = "philox", dropout_seed = PHILOX_SEED
    thr: float          # every row fires by step T - 3
    thr_cap: float      # at least one row never fires in T steps
    y: torch.Tensor     # the oracle's T steps, no stop rule: [B, T * r, d_mel], [B, T, r], [B, T, L]
    s: torch.Tensor
    w: torch.Tensor


def _thresholds(s):
    """Candidate thresholds: the middles of the gaps wider than 2 * MARGIN between neighbouring stop logits."""
    v = s.flatten().sort().values
    gap = v[1:] - v[:-1]
    mid = ((v[1:] + v[:-1]) / 2)[gap > 2.5 * MARGIN]
    return [float(x) for x in mid]


def _build(dims, wts, decode, masks):
    """The first (scale of fc_stop, threshold pair) under which the oracle alone satisfies conditions() and cap_conditions().  The
    stop logits of a random model stay within +-1 and lie close together: scaling fc_stop by a power of two spreads them (exactly,
    and nothing feeds back from them), a negative one turns their drift round."""
    mem = O.synthetic_memory(B, L, dims.d_ctx, lengths=MEM_LENGTHS, seed=4)
    for scale in (8.0, -8.0, 16.0, -16.0, 32.0, -32.0):
        w2 = {k: (v * scale if "fc_stop" in k else v) for k, v in wts.items()}
        y, s, w = decode(w2, dims, mem, max_steps=T - 1, masks=masks, stop_threshold=-1e30)
        s = s.reshape(B, T, dims.r)
        cands = _thresholds(s)
        good = [t for t in cands if all(conditions(s, t, dims.r).values())]
        thr = max(good, key=lambda t: stop_steps(s, t)[0].unique().numel()) if good else None  # (the most distinct stop steps)
        thr_cap = next((t for t in reversed(cands) if all(cap_conditions(s, t).values())), None)  # (the highest that leaves a row out)
        if thr is not None and thr_cap is not None:
            return Case(dims, w2, mem, masks, thr, thr_cap, y, s, w)
    raise AssertionError("no fc_stop scale and threshold give the spread of stop steps the tests need; change the seeds")


def _philox_masks(d_pre):
    return torch.stack([O.philox_keep_masks(PHILOX_SEED, t, B, d_pre) for t in range(T)])


DECODE_CASES = [(1, 128), (2, 256)]  # (r, d_pre)


@functools.lru_cache(maxsize=None)
def prod_case(r, d_pre):
    dims = O.DecoderDims(d_mel=80, r=r, d_pre=d_pre, d_ctx=64, h_att=256, h_dec=192)
    wts = O.random_decoder_weights(dims, seed=21, nonzero_init_state=True)
    return _build(dims, wts, O.decode, _philox_masks(d_pre))


@functools.lru_cache(maxsize=None)
def taco2_case():
    dims = O.DecoderDims(d_mel=80, r=1, d_pre=128, d_ctx=64, h_att=256, h_dec=192)
    wts = O.random_taco2_weights(dims, d_pre_hidden=128, seed=3)
    return _build(dims, wts, O.taco2_decode, _philox_masks(128))


@functools.lru_cache(maxsize=None)
def gemm_proj_case():
    """PreNet width 64: outside the fused frame kernel's shapes, so the projection is the row GEMM whose epilogue holds the other
    site of the stop rule."""
    dims = O.DecoderDims(d_mel=80, r=2, d_pre=64, d_ctx=64, h_att=256, h_dec=192)
    wts = O.random_decoder_weights(dims, seed=22, nonzero_init_state=True)
    return _build(dims, wts, O.decode, _philox_masks(64))
