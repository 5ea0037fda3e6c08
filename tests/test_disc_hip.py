"""GPU parity of the VITS2 waveform discriminators (ttsvits_disc_* through torch_tts_amd.DiscriminatorS / DiscriminatorP /
MultiPeriodDiscriminator, exact fp32) against the fp64 restatement of tests/test_disc_host.py: the scores and EVERY element of
every feature map at rtol 1e-4 / atol 1e-5.

With the recipe weights (gain 1.2) every layer's activations stay O(1-8) at T = 2310, and the reference's own fp32 differs from
fp64 by at most 0.18 of that bar, so the bar judges the kernels.  T = 2310 = 2 * 3 * 5 * 7 * 11 needs no padding for any period and
gives GEMM row counts that end inside a tile (2 * 2 * 129 = 516); T = 2311 is the maximal reflect pad p - 1 for every period; at
T = 97 and T = 12 H collapses to 1-2 rows and every tap window is clipped on both sides (the deep layers fade to ~0.03 there:
those cases test indexing, the 2310 / 2311 ones the deep GEMMs)."""
import pytest
import torch

import recipes
import torch_tts_amd as T
from hip_helpers import assert_workspace_fits
from test_disc_host import ATOL, RTOL, make_mpd, reference_disc
from torch_tts_amd.engine import Handle

pytestmark = pytest.mark.gpu
SEED = 31


@pytest.fixture(scope="module")
def mpd():
    """(the module on the GPU with its weights packed once, its state dict on the CPU for the restatement)"""
    m = make_mpd(SEED)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda().eval(), sd


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("B,Tn", [(2, 2310), (2, 2311), (2, 97), (2, 12)])
def test_scores_and_fmaps_vs_restatement(mpd, B, Tn):
    m, sd = mpd
    x = recipes.seeded_randn(100 + Tn, B, 1, Tn)
    for d, disc in enumerate(m.discriminators):
        with torch.no_grad():
            scores, fmap = disc(x.cuda())
            only = disc.scores(x.cuda())
        ref_s, ref_f = reference_disc(sd, d, x)
        _close(scores, ref_s, f"T={Tn} d={d} scores")
        assert torch.equal(only, scores), f"T={Tn} d={d}: the scores-only call differs"
        assert len(fmap) == len(ref_f)
        for l, (f, r) in enumerate(zip(fmap, ref_f)):
            _close(f, r, f"T={Tn} d={d} fmap {l}")


def test_rows_are_batch_independent_and_pairs_are_two_calls(mpd):
    m, _ = mpd
    y, y_hat = recipes.seeded_randn(7, 3, 1, 2310).cuda(), recipes.seeded_randn(8, 3, 1, 2310).cuda()
    with torch.no_grad():
        s_r, s_g, f_r, f_g = m(y, y_hat)
        for d, disc in enumerate(m.discriminators):
            for src, scores, fmaps in ((y, s_r[d], f_r[d]), (y_hat, s_g[d], f_g[d])):
                s_all, f_all = disc(src)  # a single call on this side alone
                assert torch.equal(s_all, scores), f"d={d}: forward(y, y_hat) is not two single calls"
                assert all(torch.equal(a, b) for a, b in zip(f_all, fmaps))
            for b in range(3):  # each row alone
                s1, f1 = disc(y[b:b + 1])
                assert torch.equal(s1, s_r[d][b:b + 1]), f"d={d} row {b}: scores depend on the batch"
                for l, (a, full) in enumerate(zip(f1, f_r[d])):
                    assert a.shape == full[b:b + 1].shape and torch.equal(a, full[b:b + 1]), f"d={d} row {b} fmap {l}"
    assert len(s_r) == len(s_g) == len(f_r) == len(f_g) == 6
    assert f_r[0][0].shape == (3, 16, 2310) and f_r[1][0].shape == (3, 32, 385, 2) and f_r[5][-1].shape == (3, 1, 3, 11)


def test_two_identical_calls_give_equal_bits(mpd):
    m, _ = mpd
    y, y_hat = recipes.seeded_randn(9, 2, 1, 2311).cuda(), recipes.seeded_randn(10, 2, 1, 2311).cuda()
    with torch.no_grad():
        a, b = m(y, y_hat), m(y, y_hat)
    for la, lb in zip(a[:2], b[:2]):
        assert all(torch.equal(u, v) for u, v in zip(la, lb))
    for la, lb in zip(a[2:], b[2:]):
        assert all(torch.equal(u, v) for fa, fb in zip(la, lb) for u, v in zip(fa, fb))


@pytest.mark.parametrize("d", [0, 3])
def test_workspace_fits(mpd, monkeypatch, d):
    m, _ = mpd
    x = recipes.seeded_randn(11, 2, 1, 2311).cuda()

    def run():
        with torch.no_grad():
            return m.discriminators[d].scores(x)

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


def test_strict_load_repacks(mpd):
    m, _ = mpd
    x = recipes.seeded_randn(12, 2, 1, 97).cuda()
    disc = T.DiscriminatorP(3).cuda().eval()
    disc.load_state_dict(m.discriminators[2].state_dict(), strict=True)
    with torch.no_grad():
        before, _ = disc(x)
        assert torch.equal(before, m.discriminators[2](x)[0])
        other = T.DiscriminatorP(3)
        recipes.fill_by_key(other, SEED + 1)
        disc.load_state_dict(other.state_dict(), strict=True)
        after, _ = disc(x)
    assert not torch.equal(before, after)
    sd = {"discriminators.2." + k: v for k, v in other.state_dict().items()}
    _close(after, reference_disc(sd, 2, x.cpu())[0], "after the second load")


def test_gpu_refusals(mpd):
    m, _ = mpd
    x = recipes.seeded_randn(13, 1, 1, 97).cuda()
    disc = m.discriminators[1]
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            disc(x.double())
        with pytest.raises(NotImplementedError):
            disc(x.half())
    with pytest.raises(NotImplementedError):  # grad enabled, parameters require grad
        disc(x)
    with torch.no_grad(), pytest.raises(ValueError):
        m.discriminators[5](x[:, :, :3])  # period 11, T = 3: the pad (8) is not smaller than T
