"""GPU parity at the corners of the dims that ttsgen_create, ttsdur_create / ttsvits_durnll_create and ttsvits_disc_create accept
(tests/dims_corner_cases.py): every case through torch_tts_amd.Generator (exact fp32 and split-fp16), StochasticDurationPredictor
(reverse and nll), DurationPredictor and DiscriminatorP against the fp64 restatements of the host tests, under each family's own bar -
rtol 1e-4 / atol 1e-5 for the generator (waveform and every stage) and the discriminators (scores and every element of every feature
map), |a - b| / (0.1 + |b|) <= 1e-4 for logw, nll and its terms.  tests/test_dims_corners_host.py shows that the restatements are
the reference at these dims and that the reference's own fp32 is within half of each bar."""
import pytest
import torch

import dims_corner_cases as K
import recipes
import torch_tts_amd as T
from hip_helpers import assert_workspace_fits
from test_dims_corners_host import ATOL, LOGW_REL, RTOL, load_golden, sdp_refs, state
from test_disc_host import reference_disc
from test_duration_host import _rel, dp_forward
from test_durnll_hip import check, run_parts
from test_generator_host import reference_forward
from torch_tts_amd.engine import Handle

pytestmark = pytest.mark.gpu
_built = {}  # (family, case) -> what the tests of this module share: the module on the GPU, its CPU state dict, references


@pytest.fixture(scope="module", autouse=True)
def _drop_modules():
    yield
    _built.clear()


def once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    print(f"{what}: worst |err| / (atol + rtol |ref|) = {float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()):.3f}")
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


# ---------------------------------------------------------------------------------------------------------------------------
# Generator
# ---------------------------------------------------------------------------------------------------------------------------
def generator(name):
    def make():
        gen = K.make_generator(T, name)
        return gen.cuda().eval(), state(gen)

    return once(("gen", name), make)


def gen_case(name, Tn):
    """-> x, g on the GPU and the restatement's (waveform, stage outputs), computed once"""
    def make():
        x, g = K.gen_inputs(name, Tn)
        return x.cuda(), g.cuda(), reference_forward(generator(name)[1], K.GEN_CASES[name]["dims"], x, g, stages=True)

    return once(("gen", name, Tn), make)


def gen_run(name, Tn, precision, stages=False):
    """-> the waveform (, the activated output of conv_pre and of every stage)"""
    gen, _ = generator(name)
    x, g, _ = gen_case(name, Tn)
    gen.precision = precision
    try:
        with torch.no_grad():
            y = gen(x, g)
            return (y, [gen.stage_outputs(x, g, n_stages=s) for s in range(gen.num_upsamples + 1)]) if stages else y
    finally:
        gen.precision = "f32"


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("name", list(K.GEN_CASES))
def test_generator_waveform_and_every_stage(name, precision):
    g, _ = load_golden()
    for Tn in K.GEN_CASES[name]["T"]:
        y_ref, acts = gen_case(name, Tn)[2]
        y, stages = gen_run(name, Tn, precision, stages=True)
        _close(y, y_ref, f"{name} T={Tn} {precision}")
        _close(y, g[f"gen/{name}/T{Tn}/y"], f"{name} T={Tn} {precision} against the reference's output")
        assert len(stages) == len(acts)
        for s, (a, r) in enumerate(zip(stages, acts)):
            _close(a, r, f"{name} T={Tn} {precision} stage {s}")


def test_g2_split_is_a_mixed_handle_and_not_the_exact_path():
    """G2 in split-fp16: conv_pre (4 input channels) and the last stage (C = 4) keep the exact tiles, ups[0], stage 0 and ups[1]
    split; had the mode fallen back as a whole, the two results would agree in every sample."""
    for Tn in K.GEN_CASES["G2"]["T"]:
        assert not torch.equal(gen_run("G2", Tn, "split_f16"), gen_run("G2", Tn, "f32")), Tn


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_g2_workspace_fits_in_groups_of_one(monkeypatch, precision):
    """TTSGEN_GROUP_FORCE=1: two groups of one utterance (u = 64: one frame of z becomes 128 of the last stage), in both
    precisions - split-fp16 adds the planes of z and, the handle being mixed, the fp32 hand-off buffer to the carve."""
    want = gen_run("G2", 9, precision)
    monkeypatch.setenv("TTSGEN_GROUP_FORCE", "1")
    got = []

    def run():
        got.append(gen_run("G2", 9, precision))
        return got[-1]

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)
    assert torch.equal(got[0], want), "the result depends on the group size"


def test_g1_neighbour_independence():
    gen, _ = generator("G1")
    x, g, _ = gen_case("G1", 23)
    x2 = x.clone()
    x2[0] = recipes.seeded_randn(9, *x2[0].shape).cuda()
    with torch.no_grad():
        y0, y1 = gen(x, g), gen(x2, g)
    assert torch.equal(y0[1], y1[1]) and not torch.equal(y0[0], y1[0])


# ---------------------------------------------------------------------------------------------------------------------------
# Duration predictors
# ---------------------------------------------------------------------------------------------------------------------------
def sdp(name):
    def make():
        m = K.make_sdp(T, name)
        g, _ = load_golden()
        ops = {k: g.get(f"sdp/{name}/{k}") for k in ("x", "x_mask", "g", "noise", "w", "e_q")}
        return m.cuda().eval(), ops, sdp_refs(name)

    return once(("sdp", name), make)


def sdp_reverse_run(m, ops, rows=slice(None), n=K.DUR_T):
    g = None if ops["g"] is None else ops["g"][rows].cuda()
    with torch.no_grad():
        return m(ops["x"][rows, :, :n].cuda(), ops["x_mask"][rows, :, :n].cuda(), g=g, reverse=True, noise_scale=K.DUR_NOISE_SCALE,
                 noise=ops["noise"][rows, :, :n]).cpu()


def sdp_nll_run(m, ops, rows=slice(None), n=K.DUR_T):
    g = None if ops["g"] is None else ops["g"][rows]
    return run_parts(m, ops["x"][rows, :, :n], ops["x_mask"][rows, :, :n], ops["w"][rows, :, :n], ops["e_q"][rows, :, :n], g)


@pytest.mark.parametrize("name", list(K.SDP_CASES))
def test_sdp_reverse(name):
    m, ops, (logw_ref, _, _) = sdp(name)
    lw = sdp_reverse_run(m, ops)
    print(name, "reverse", _rel(lw, logw_ref))
    assert lw.shape == logw_ref.shape and _rel(lw, logw_ref) <= LOGW_REL, (name, _rel(lw, logw_ref))
    for b, n in enumerate(K.DUR_LENGTHS):  # padded frames: exactly 0
        assert float(lw[b, 0, n:].abs().sum()) == 0.0 and bool((lw[b, 0, :n] != 0).all()), (name, b)


@pytest.mark.parametrize("name", list(K.SDP_CASES))
def test_sdp_likelihood(name):
    m, ops, (_, ref, _) = sdp(name)
    got = sdp_nll_run(m, ops)
    check(got, ref, f"{name} nll")
    for b, n in enumerate(K.DUR_LENGTHS):
        assert float(got[2][b, :, n:].abs().sum()) == 0.0, (name, b)


@pytest.mark.parametrize("name", ["D2", "D3"])
def test_sdp_rows_alone_and_twice(name):
    """Each utterance alone, at its own length, gives the bits it has in the padded batch; a second call gives the first's bits."""
    m, ops, _ = sdp(name)
    lw, parts = sdp_reverse_run(m, ops), sdp_nll_run(m, ops)
    assert torch.equal(lw, sdp_reverse_run(m, ops)), "two identical reverse calls differ"
    for a, b in zip(parts, sdp_nll_run(m, ops)):
        assert torch.equal(a, b), "two identical likelihood calls differ"
    for b, n in enumerate(K.DUR_LENGTHS):
        rows = slice(b, b + 1)
        assert torch.equal(sdp_reverse_run(m, ops, rows, n)[0], lw[b, :, :n]), (name, b)
        alone = sdp_nll_run(m, ops, rows, n)
        assert torch.equal(alone[0][0], parts[0][b]) and torch.equal(alone[1][0], parts[1][b]), (name, b)
        assert torch.equal(alone[2][0], parts[2][b, :, :n]), (name, b)


@pytest.mark.parametrize("direction", ["reverse", "nll"])
def test_d2_workspace_fits(monkeypatch, direction):
    m, ops, _ = sdp("D2")

    def run():
        if direction == "reverse":
            return sdp_reverse_run(m, ops)
        return torch.cat([t.reshape(-1) for t in sdp_nll_run(m, ops)])

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


@pytest.mark.parametrize("name", list(K.DP_CASES))
def test_dp(name):
    g, _ = load_golden()
    dp = K.make_dp(T, name)
    sd = state(dp)
    dp = dp.cuda().eval()
    x, x_mask, gg = g[f"dp/{name}/x"], g[f"dp/{name}/x_mask"], g.get(f"dp/{name}/g")
    with torch.no_grad():
        ld = dp(x.cuda(), x_mask.cuda(), g=None if gg is None else gg.cuda()).cpu()
        again = dp(x.cuda(), x_mask.cuda(), g=None if gg is None else gg.cuda()).cpu()
    ref = dp_forward(sd, x, x_mask, gg)
    print(name, _rel(ld, ref))
    assert ld.shape == ref.shape and _rel(ld, ref) <= LOGW_REL, (name, _rel(ld, ref))
    assert torch.equal(ld, again)
    for b, n in enumerate(K.DUR_LENGTHS):
        assert float(ld[b, 0, n:].abs().sum()) == 0.0, (name, b)


# ---------------------------------------------------------------------------------------------------------------------------
# DiscriminatorP
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.DISC_CASES))
def test_disc_scores_and_every_feature_map(name):
    """P3 is what gave disc.hip its long-K tile: with one fp32 accumulator per output its feature map 3 (K = 15 x 512) was 1.017 of
    the bar from fp64 on an MI355X; with four chains per output it is at 0.602 and feature map 4 (K = 15 x 1024) at 0.945 - the
    reference's own fp32 on the CPU is at 0.27 and 0.34 there (dims_corners_meta.json).  Every other case stays below 0.41."""
    c = K.DISC_CASES[name]
    disc = K.make_disc(T, name)
    sd = state(disc)
    disc = disc.cuda().eval()
    x = K.disc_input(name)
    with torch.no_grad():
        scores, fmap = disc(x.cuda())
        only = disc.scores(x.cuda())
        alone = disc(x[1:2].cuda()) if name in ("P3", "P6") else None
    ref_s, ref_f = reference_disc(sd, 1, x, period=c["period"], stride=c["stride"], prefix="")
    assert len(fmap) == len(ref_f) == 6
    pairs = [(scores, ref_s, f"{name} scores")] + [(f, r, f"{name} fmap {l}") for l, (f, r) in enumerate(zip(fmap, ref_f))]
    for a, b, what in pairs:  # every figure before the first assertion
        print(f"{what} (all figures first): {float(((a.cpu().double() - b).abs() / (ATOL + RTOL * b.abs())).max()):.3f} of the bar")
    for a, b, what in pairs:
        _close(a, b, what)
    assert torch.equal(only, scores), f"{name}: the scores-only call differs"
    if alone is not None:  # row 1 alone: the bits it has in the batch
        assert torch.equal(alone[0], scores[1:2]), f"{name}: row 1's scores depend on the batch"
        for l, (a, full) in enumerate(zip(alone[1], fmap)):
            assert a.shape == full[1:2].shape and torch.equal(a, full[1:2]), f"{name} row 1 fmap {l}"
