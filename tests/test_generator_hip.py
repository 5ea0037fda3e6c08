"""GPU parity of the VITS2 HiFi-GAN generator (ttsgen_* through torch_tts_amd.Generator, exact fp32) against (a) the reference's
own outputs at small dims (tests/golden/make_golden_generator.py) and (b) the fp64 restatement of tests/test_generator_host.py at the
ModelConfig dims, at the timing tool's batch (64 x 600) and above the 2-GiB group bound (128 x 600)."""
import os

import pytest
import torch

from hip_helpers import sample_utterances
from test_generator_host import load_golden, make_generator, reference_forward, scaled_weights, weights

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
FULL = dict(initial_channel=192, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
            upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _stages_close(gen, sd, dims, x, g, what):
    """Every stage's activated output (ttsgen_forward_stages) against the restatement: a wrong late layer cannot hide behind tanh."""
    _, acts = reference_forward(sd, dims, x.cpu(), None if g is None else g.cpu(), stages=True)
    with torch.no_grad():
        for s, ref in enumerate(acts):
            _close(gen.stage_outputs(x, g, n_stages=s), ref, f"{what} stage {s}")


@pytest.fixture(scope="module")
def full_gen():
    gen = make_generator(FULL)
    scaled_weights(gen, 5)
    gen = gen.cuda().eval()
    sd = {k: v.detach().cpu() for k, v in gen.state_dict().items()}
    return gen, sd


def test_golden_small_dims():
    gsd, meta = load_golden()
    for gin in (0, 4):
        gen = make_generator(meta["dims"], gin)
        gen.load_state_dict(weights(gsd, gin), strict=True)
        gen = gen.cuda().eval()
        for T in meta["T"]:
            x = gsd[f"x{gin}/T{T}"].cuda()
            g = gsd[f"g{gin}/T{T}"].cuda() if gin else None
            with torch.no_grad():
                y = gen(x, g)
            _close(y, gsd[f"y{gin}/T{T}"], f"gin={gin} T={T}")
            _stages_close(gen, weights(gsd, gin), meta["dims"], x, g, f"gin={gin} T={T}")
        # remove_weight_norm: same module, plain weights, repacked
        gen.remove_weight_norm()
        with torch.no_grad():
            y = gen(gsd[f"x{gin}/T9"].cuda(), gsd[f"g{gin}/T9"].cuda() if gin else None)
        _close(y, gsd[f"y{gin}/T9"], f"gin={gin} after remove_weight_norm")


def test_carved_workspace_fits_the_reported_bytes(monkeypatch):
    """ttsgen_forward at the golden small dims, B = 3 x T = 37 in groups of two (a full group, then a short last one whose buffers
    lie closer together than the reported size's): nothing is written outside ttsgen_workspace_bytes, and the waveform is that of a
    roomy workspace bit for bit."""
    from hip_helpers import assert_workspace_fits
    from torch_tts_amd.engine import Handle

    gsd, meta = load_golden()
    gen = make_generator(meta["dims"], 4)
    gen.load_state_dict(weights(gsd, 4), strict=True)
    gen = gen.cuda().eval()
    rng = torch.Generator().manual_seed(4)
    x, g = torch.randn(3, meta["dims"]["initial_channel"], 37, generator=rng).cuda(), torch.randn(3, 4, 1, generator=rng).cuda()
    monkeypatch.setenv("TTSGEN_GROUP_FORCE", "2")

    def run():
        with torch.no_grad():
            return gen(x, g)

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


def test_fulldims_b64_x_600(full_gen):
    gen, sd = full_gen
    B, T = 64, 600
    torch.manual_seed(1)
    z = torch.randn(B, 192, T)
    with torch.no_grad():
        y = gen(z.cuda())
        y2 = gen(z.cuda())
    assert torch.equal(y, y2), "two identical calls differ"
    y = y.cpu()
    assert y.shape == (B, 1, T * 256)
    assert float((y.abs() > 0.99).float().mean()) < 0.05
    # (group boundaries: groups of 27 utterances at T = 600; tile boundaries lie inside every utterance)
    for b in sample_utterances(B, T * 256, boundaries=[27 * T * 256 - 1, 27 * T * 256, 54 * T * 256], k_random=2, seed=3):
        _close(y[b : b + 1], reference_forward(sd, FULL, z[b : b + 1]), f"b={b}")
    _stages_close(gen, sd, FULL, z[:2].cuda(), None, "B=2 T=600")


def test_fulldims_odd_lengths_and_noncontiguous(full_gen):
    gen, sd = full_gen
    torch.manual_seed(2)
    for T in (1, 3, 37, 601):
        z = torch.randn(2, 192, T)
        with torch.no_grad():
            y = gen(z.cuda()).cpu()
        _close(y, reference_forward(sd, FULL, z), f"T={T}")
    # SynthesizerTrn.infer passes (z * y_mask)[:, :, :max_len]: a non-contiguous slice
    zz = torch.randn(3, 192, 50)
    with torch.no_grad():
        y = gen(zz.cuda()[:, :, :41]).cpu()
    _close(y, reference_forward(sd, FULL, zz[:, :, :41]), "sliced input")


def test_neighbour_independence(full_gen):
    gen, _ = full_gen
    torch.manual_seed(4)
    z = torch.randn(5, 192, 37, device="cuda")
    with torch.no_grad():
        y0 = gen(z)
        z2 = z.clone()
        z2[1] = torch.randn_like(z2[1])
        z2[3] = torch.randn_like(z2[3])
        y1 = gen(z2)
    assert torch.equal(y0[2], y1[2])
    assert not torch.equal(y0[1], y1[1])


def test_above_2gib_bound_and_group_size(full_gen, monkeypatch):
    gen, sd = full_gen
    B, T = 128, 600  # one stage-4 activation of 128 utterances is 2.5 GB; groups of 27 (include/ttsdec.h)
    torch.manual_seed(6)
    z = torch.randn(B, 192, T)
    with torch.no_grad():
        y = gen(z.cuda()).cpu()
    for b in (0, 26, 27, 108, 109, B - 1):
        _close(y[b : b + 1], reference_forward(sd, FULL, z[b : b + 1]), f"b={b}")
    eng = gen._engines.get(gen._cfg, torch.device("cuda", 0))
    eng.release_workspaces()  # (free the large workspace before the forced-group run)
    monkeypatch.setenv("TTSGEN_GROUP_FORCE", "7")
    with torch.no_grad():
        yf = gen(z[100:120].cuda()).cpu()
    assert torch.equal(yf, y[100:120]), "result depends on the group size"
