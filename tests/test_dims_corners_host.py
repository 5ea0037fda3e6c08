"""Host-side checks of the dims corners of tests/dims_corner_cases.py (the generator, the duration predictors, DiscriminatorP):
the fp64 restatements of test_generator_host / test_duration_host / test_durnll_host / test_disc_host - the oracles of
tests/test_dims_corners_hip.py - against the reference's own outputs at these dims (tests/golden/make_golden_dims_corners.py),
each under its family's existing bar; that the reference's own fp32 lies within half of that bar at every case, so the bar judges
the kernels and not the case; that each SDP case reaches both branches of the spline; and that the four *_create calls accept
every case's dims.  No GPU needed."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dims_corner_cases as K
import recipes
import torch_tts_amd as T
from test_disc_host import reference_disc
from test_duration_host import _rel, dp_forward, sdp_reverse
from test_durnll_host import NLL_REL, rel, sdp_nll
from test_generator_host import reference_forward
from torch_tts_amd import _lib, vits2

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-4, 1e-5  # generator and discriminators
LOGW_REL = 1e-4          # durations: test_duration_host._rel
RATIO_MAX = 0.5


@functools.lru_cache(maxsize=None)
def load_golden():
    z = np.load(os.path.join(HERE, "golden", "dims_corners.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "dims_corners_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def state(mod):
    return {k: v.detach().clone().cpu() for k, v in mod.state_dict().items()}


def ratio_close(a, b):
    """a against the fp64 b as a fraction of the rtol / atol bar (make_golden_dims_corners.ratio_close)."""
    return float(((a.double() - b.double()).abs() / (ATOL + RTOL * b.double().abs())).max())


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _same_ratio(got, recorded, what):
    """The ratio the golden script measured is the one this machine measures (both are fp32-vs-fp64 differences: rounding noise
    of the fp64 side moves them by far less than a percent), and it is within half of the bar."""
    assert recorded <= RATIO_MAX, (what, recorded)
    assert got == pytest.approx(recorded, rel=1e-3, abs=1e-6), (what, got, recorded)


def sdp_refs(name):
    """The fp64 restatement of both directions of one SDP case on the recorded operands, and the first inverse spline's inputs."""
    g, _ = load_golden()
    c = K.SDP_CASES[name]
    sd = state(K.make_sdp(T, name))
    k = lambda n: g.get(f"sdp/{name}/{n}")  # noqa: E731
    probe = []
    logw = sdp_reverse(sd, k("x"), k("x_mask"), k("noise"), K.DUR_NOISE_SCALE, k("g"), n_flows=c["n_flows"], probe=probe)
    nll = sdp_nll(sd, k("x"), k("x_mask"), k("w"), k("e_q"), k("g"), n_flows=c["n_flows"])
    return logw, nll, probe


def test_tables_are_the_recorded_ones():
    g, meta = load_golden()
    assert meta["ratio_max"] == RATIO_MAX and meta["stride"] == K.DISC_STRIDE == 13
    assert {n: (c["dims"], c["gain"], c["seed"], [int(t) for t in c["T"]]) for n, c in meta["gen"].items()} == {
        n: (c["dims"], c["gain"], c["seed"], c["T"]) for n, c in K.GEN_CASES.items()}
    for fam, table in (("sdp", K.SDP_CASES), ("dp", K.DP_CASES), ("disc", K.DISC_CASES)):
        assert {n: {k: c[k] for k in table[n]} for n, c in meta[fam].items()} == table, fam
    for name, c in K.SDP_CASES.items():  # the recorded operands are the table's recipe
        for k, v in K.dur_inputs(c).items():
            assert (v is None and f"sdp/{name}/{k}" not in g) or torch.equal(v, g[f"sdp/{name}/{k}"]), (name, k)
    assert K.dur_mask()[:, 0].sum(1).long().tolist() == K.DUR_LENGTHS and K.DUR_B * K.DUR_T == 99
    for name, c in K.GEN_CASES.items():
        for Tn in c["T"]:
            x, gg = K.gen_inputs(name, Tn)
            assert torch.equal(x, g[f"gen/{name}/T{Tn}/x"]) and torch.equal(gg, g[f"gen/{name}/T{Tn}/g"])
    for name in K.DISC_CASES:
        assert torch.equal(K.disc_input(name), g[f"disc/{name}/x"])


@pytest.mark.parametrize("name", list(K.GEN_CASES))
def test_generator_restatement_matches_the_reference(name):
    g, meta = load_golden()
    c = K.GEN_CASES[name]
    gen = K.make_generator(T, name)
    sd = state(gen)
    assert len(sd) == meta["gen"][name]["n_tensors"]
    for Tn in c["T"]:
        rec = meta["gen"][name]["T"][str(Tn)]
        y = reference_forward(sd, c["dims"], g[f"gen/{name}/T{Tn}/x"], g[f"gen/{name}/T{Tn}/g"])
        ref = g[f"gen/{name}/T{Tn}/y"]
        assert list(y.shape) == rec["shape"] == [K.GEN_B, 1, Tn * int(np.prod(c["dims"]["upsample_rates"]))]
        _close(y, ref, f"{name} T={Tn}")
        _same_ratio(ratio_close(ref, y), rec["ratio"], f"{name} T={Tn}")
        assert rec["stage_ratio"] <= RATIO_MAX and rec["sat_frac"] < 0.05 and rec["y_rms"] > 0.05  # (neither saturated nor faded)


@pytest.mark.parametrize("name", list(K.SDP_CASES))
def test_sdp_restatement_matches_the_reference_in_both_directions(name):
    g, meta = load_golden()
    rec = meta["sdp"][name]
    logw, ref, _ = sdp_refs(name)
    assert len(K.make_sdp(T, name).state_dict()) == rec["n_tensors"]
    got = g[f"sdp/{name}/logw"]
    assert got.shape == logw.shape == (K.DUR_B, 1, K.DUR_T)
    assert _rel(got, logw) <= LOGW_REL, (name, _rel(got, logw))
    _same_ratio(_rel(got, logw) / LOGW_REL, rec["ratio_reverse"], f"{name} reverse")
    assert float(got.abs().max()) > 0.5 and float(got[2, 0, 1:].abs().max()) == 0.0  # (not an identity chain; padded frames)
    assert rel(g[f"sdp/{name}/nll"], ref["nll"]) <= NLL_REL, (name, rel(g[f"sdp/{name}/nll"], ref["nll"]))
    _same_ratio(rel(g[f"sdp/{name}/nll"], ref["nll"]) / NLL_REL, rec["ratio_nll"], f"{name} nll")
    _close(g[f"sdp/{name}/z"], ref["z"], f"{name} z")
    _same_ratio(ratio_close(g[f"sdp/{name}/z"], ref["z"]), rec["ratio_z"], f"{name} z")
    t = ref["terms"]
    assert rel((t[:, 2] - t[:, 3]) + (t[:, 0] - t[:, 1]), ref["nll"]) <= 1e-9 and ref["clamped"]


@pytest.mark.parametrize("name", list(K.SDP_CASES))
def test_sdp_cases_reach_both_branches_of_the_spline(name):
    """The first inverse spline of the reverse pass sees in-length inputs outside +-5 (linear tails) and inside (the bins), one of
    them on the top edge; the likelihood's splines too."""
    _, ref, probe = sdp_refs(name)
    assert len(probe) == K.SDP_CASES[name]["n_flows"] - 1  # (flows.1 is dropped)
    first = probe[0].abs()
    assert first.numel() == sum(K.DUR_LENGTHS) and int((first > 5).sum()) >= 3 and int((first < 5).sum()) >= 3 and bool((probe[0] == 5.0).any())
    si = ref["spline_inputs"].abs()
    assert int((si > 5).sum()) >= 3 and int((si < 5).sum()) >= 3 * int((si > 5).sum())


@pytest.mark.parametrize("name", list(K.DP_CASES))
def test_dp_restatement_matches_the_reference(name):
    g, meta = load_golden()
    c = K.DP_CASES[name]
    want = K.dur_inputs(c)
    assert torch.equal(want["x"], g[f"dp/{name}/x"]) and torch.equal(want["x_mask"], g[f"dp/{name}/x_mask"])
    logw = dp_forward(state(K.make_dp(T, name)), g[f"dp/{name}/x"], g[f"dp/{name}/x_mask"], g.get(f"dp/{name}/g"))
    got = g[f"dp/{name}/logw"]
    assert _rel(got, logw) <= LOGW_REL, (name, _rel(got, logw))
    _same_ratio(_rel(got, logw) / LOGW_REL, meta["dp"][name]["ratio"], name)
    assert float(got.abs().max()) > 0.5 and float(got[2, 0, 1:].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(K.DISC_CASES))
def test_disc_restatement_matches_the_reference(name):
    g, meta = load_golden()
    c, rec = K.DISC_CASES[name], meta["disc"][name]
    disc = K.make_disc(T, name)
    assert sum(p.numel() for p in disc.parameters()) == rec["n_params"]
    scores, fmap = reference_disc(state(disc), 1, g[f"disc/{name}/x"], period=c["period"], stride=c["stride"], prefix="")
    _close(scores, g[f"disc/{name}/score"], f"{name} scores")
    _same_ratio(ratio_close(g[f"disc/{name}/score"], scores), rec["ratio_score"], f"{name} scores")
    assert len(fmap) == len(rec["fmaps"]) == 6 and rec["ratio"] <= RATIO_MAX
    for l, (f, r) in enumerate(zip(fmap, rec["fmaps"])):
        assert list(f.shape) == r["shape"]
        got = g[f"disc/{name}/fmap/{l}"]
        _close(f.reshape(-1)[::K.DISC_STRIDE], got, f"{name} fmap {l}")
        assert float(f.abs().mean()) == pytest.approx(r["mean_abs"], rel=1e-5) and r["mean_abs"] > 0.02  # (no layer faded away)
        # the recorded ratio is over every element, the samples are a thirteenth of them
        assert r["ratio"] <= rec["ratio"] and ratio_close(got, f.reshape(-1)[::K.DISC_STRIDE]) <= r["ratio"] * (1 + 1e-3) + 1e-6


def test_existing_disc_calls_keep_their_defaults():
    """reference_disc without the new arguments is the MultiPeriodDiscriminator member it was: stride 3, the period of its index."""
    disc = T.DiscriminatorP(5).eval()
    recipes.fill_by_key(disc, 7)
    x = recipes.seeded_randn(8, 1, 1, 97)
    sd = {"discriminators.3." + k: v for k, v in state(disc).items()}
    a = reference_disc(sd, 3, x)
    b = reference_disc(state(disc), 1, x, period=5, stride=3, prefix="")
    assert torch.equal(a[0], b[0]) and all(torch.equal(u, v) for u, v in zip(a[1], b[1]))
    assert not torch.equal(a[0], reference_disc(state(disc), 1, x, period=5, stride=2, prefix="")[0])


def test_create_accepts_every_case():
    """ttsgen_create, ttsdur_create, ttsvits_durnll_create and ttsvits_disc_create return OK (a Handle raises otherwise); the
    tensor counts are the modules'; the workspaces are positive."""
    for name, c in K.GEN_CASES.items():
        gen = K.make_generator(T, name)
        eng = vits2.GenEngine(gen._cfg, None)
        try:
            assert eng.num_weight_tensors() == len(gen.weight_tensors())
            for Tn in c["T"]:
                assert int(eng._lib.ttsgen_workspace_bytes(eng._h, K.GEN_B, Tn)) > 0
                for prec in (_lib.PREC_F32, _lib.PREC_SPLIT_F16):
                    assert int(eng._lib.ttsvits_generator_workspace_bytes(eng._h, prec, K.GEN_B, Tn)) > 0
        finally:
            eng.close()
    for name in K.SDP_CASES:
        sdp = K.make_sdp(T, name)
        for eng, tensors in ((vits2.DurEngine(sdp._cfg, None), sdp.weight_tensors()), (vits2.DurNllEngine(sdp._nll_cfg, None), sdp.nll_weight_tensors())):
            try:
                assert eng.num_weight_tensors() == len(tensors), name
                assert int(eng._fn("workspace_bytes")(eng._h, K.DUR_B, K.DUR_T)) > 0
            finally:
                eng.close()
        assert len(sdp.nll_weight_tensors()) == len(list(sdp.parameters()))
    for name in K.DP_CASES:
        dp = K.make_dp(T, name)
        eng = vits2.DurEngine(dp._cfg, None)
        try:
            assert eng.num_weight_tensors() == len(dp.weight_tensors()) == len(list(dp.parameters()))
            assert int(eng._fn("workspace_bytes")(eng._h, K.DUR_B, K.DUR_T)) > 0
        finally:
            eng.close()
    for name, c in K.DISC_CASES.items():
        eng = vits2.DiscEngine(dict(period=c["period"], kernel_size=c["kernel_size"], stride=c["stride"]), None)
        try:
            assert eng.num_weight_tensors() == len(K.make_disc(T, name).weight_tensors()) == 12 and eng.workspace_bytes(K.DISC_B, c["T"]) > 0
            _, meta = load_golden()
            assert eng.heights(c["T"]) == [f["shape"][2] for f in meta["disc"][name]["fmaps"]]
        finally:
            eng.close()
