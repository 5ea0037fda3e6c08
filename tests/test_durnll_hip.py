"""GPU parity of the VITS2 duration likelihood (ttsvits_durnll_* through torch_tts_amd.vits2, exact fp32) against (a) the
reference's own outputs at small dims (tests/golden/make_golden_durnll.py) and (b) the fp64 restatement of
tests/test_durnll_host.py, at the tile edges, beyond the spline's tails, at Log's clamp and at the model dims.  The bar is the
project's |a - b| / (0.1 + |b|) <= 1e-4 on nll and on each of its four terms - at least 4 x the reference's own fp32-vs-fp64 error
recorded in durnll_meta.json - and RTOL / ATOL on z; no token and no utterance is left out of a comparison."""
import functools

import pytest
import torch

from test_align_host import AlignNet
from test_duration_host import randomize
from test_durnll_host import NLL_REL, big_case, golden_sdp, load_golden, mask_of, rel, same_checksum, sdp_nll, state

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
LOGW_REL = 1e-4


def _T():
    import torch_tts_amd as T

    return T


def run_parts(sdp, x, x_mask, w, e_q, g=None):
    """nll_cl(parts=True) on the reference's operands -> (nll, terms, z) on the CPU."""
    lengths = x_mask[:, 0].sum(1).to(torch.int32)
    with torch.no_grad():
        out = sdp.nll_cl(x.transpose(1, 2).contiguous().cuda(), lengths.cuda(), w[:, 0].contiguous().cuda(), None if g is None else g.cuda(),
                         noise=e_q, parts=True)
    return tuple(t.cpu() for t in out)


def check(got, ref, what):
    """nll, each term and z of a call against the restatement's dict; prints every figure before it asserts."""
    nll, terms, z = got
    errs = {"nll": rel(nll, ref["nll"]), **{f"term{i}": rel(terms[:, i], ref["terms"][:, i]) for i in range(4)}}
    print(what, errs, "z", float((z.double() - ref["z"]).abs().max()))
    for k, e in errs.items():
        assert e <= NLL_REL, (what, k, e)
    torch.testing.assert_close(z.double(), ref["z"], rtol=RTOL, atol=ATOL, msg=lambda m: f"{what} z: {m}")
    assert rel((terms[:, 2] - terms[:, 3]) + (terms[:, 0] - terms[:, 1]), nll) <= 1e-6


@functools.lru_cache(maxsize=None)
def small_sdp(gin):
    _, meta = load_golden()
    sdp = golden_sdp(meta, gin)
    return sdp.cuda().eval(), state(sdp)


def small_case(T, lengths, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    x_mask = mask_of(lengths, T)
    x = torch.randn(len(lengths), 32, T, generator=gen) * x_mask
    w = torch.randint(1, 13, (len(lengths), 1, T), generator=gen).float() * x_mask
    e_q = torch.randn(len(lengths), 2, T, generator=gen) * scale
    return x, x_mask, w, e_q


@pytest.mark.parametrize("gin", [0, 4])
def test_golden_small_dims(gin):
    sd, meta = load_golden()
    sdp, _ = small_sdp(gin)
    x, x_mask, w, e_q = sd["case/x"], sd["case/x_mask"], sd["case/w"], sd["case/e_q"]
    g = sd["case/g4"] if gin else None
    nll, terms, z = run_parts(sdp, x, x_mask, w, e_q, g)
    for ref in (sd[f"sdp{gin}/nll"], sd[f"sdp{gin}/nll64"]):
        print("golden", gin, rel(nll, ref))
        assert rel(nll, ref) <= NLL_REL, (gin, rel(nll, ref))
    torch.testing.assert_close(z, sd[f"sdp{gin}/z"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(z.double(), sd[f"sdp{gin}/z64"], rtol=RTOL, atol=ATOL)
    assert float(z[2, :, 1:].abs().max()) == 0.0 and float(z[1, :, 5:].abs().max()) == 0.0  # padded tokens
    with torch.no_grad():  # the reference's call shape, g as [B, gin, 1]; and its own draw when none is given
        gc = None if g is None else g.cuda()
        assert torch.equal(sdp.nll(x.cuda(), x_mask.cuda(), w.cuda(), g=gc, noise=e_q).cpu(), nll)
        torch.manual_seed(5)
        drawn = sdp.nll(x.cuda(), x_mask.cuda(), w.cuda(), g=gc)
        torch.manual_seed(5)
        assert torch.equal(drawn, sdp.nll(x.cuda(), x_mask.cuda(), w.cuda(), g=gc, noise=torch.randn(3, 2, 9)))
        assert not torch.equal(drawn.cpu(), nll)


@pytest.mark.parametrize("T", [15, 16, 17, 33])
@pytest.mark.parametrize("short", ["one", "T-1"])
def test_tile_edges(T, short):
    """16 token rows per workgroup, dilations 1, 3, 9 reaching across them; utterance 1 starts at row T of the batch."""
    sdp, sd = small_sdp(0)
    x, x_mask, w, e_q = small_case(T, [T, 1 if short == "one" else T - 1], 100 + T)
    check(run_parts(sdp, x, x_mask, w, e_q), sdp_nll(sd, x, x_mask, w, e_q), f"T={T} {short}")


def test_tails_and_the_clamp():
    sdp, sd = small_sdp(4)
    x, x_mask, w, e_q = small_case(21, [21, 13, 4], 55, scale=3.0)
    g = torch.randn(3, 4, 1, generator=torch.Generator().manual_seed(56))
    w[1, 0, 7] = 0.0  # an in-length token without a frame: z0 = -u < 1e-5
    ref = sdp_nll(sd, x, x_mask, w, e_q, g)
    si = ref["spline_inputs"].abs()
    assert ref["clamped"] and int((si > 5).sum()) >= 3 and int((si < 5).sum()) >= 3 * int((si > 5).sum())
    check(run_parts(sdp, x, x_mask, w, e_q, g), ref, "tails")


@functools.lru_cache(maxsize=None)
def model_dims(gin):
    """C = 192, 4 x 150 with lengths 150 / 149 / 64 / 2: the predictor on the device, its operands, the call's results and the
    restatement's - computed once, shared by the tests below and left unchanged.  gin 0 is the yardstick's case of
    durnll_meta.json.  For gin 4 the weights' seed is the one make_golden_durnll.py settled on by the reference's own error
    (c192_t150_g4): at these dims a token's z is often so ill-conditioned that the reference's own fp32 CPU z misses the bar on z
    against its fp64 self (at 11 of the 21 seeds it tried; at the first, seed 11, by 9.3e-5 at a value of 0.395, where these kernels
    were off by 7.7e-5), which says nothing about a kernel; the seed kept has the reference within a quarter of the bar."""
    _, meta = load_golden()
    c = meta["c192_t150"]
    sdp = randomize(_T().StochasticDurationPredictor(192, 192, 3, 0.5, 4, gin_channels=gin), meta["c192_t150_g4"]["seed"] if gin else c["seed"])
    sd = state(sdp)
    sdp = sdp.cuda().eval()
    x, x_mask, w, e_q = big_case(c["case_seed"])
    g = torch.randn(4, gin, 1, generator=torch.Generator().manual_seed(meta["c192_t150_g4"]["g_seed"])) if gin else None
    return sdp, sd, (x, x_mask, w, e_q, g), run_parts(sdp, x, x_mask, w, e_q, g), sdp_nll(sd, x, x_mask, w, e_q, g)


@pytest.mark.parametrize("gin", [0, 4])
def test_model_dims_b4(gin):
    _, meta = load_golden()
    _, _, _, got, ref = model_dims(gin)
    check(got, ref, f"c192 gin={gin}")
    if gin == 0:  # the yardstick's case: the reference's own fp32 nll is recorded
        assert rel(got[0], torch.tensor(meta["c192_t150"]["nll"])) <= NLL_REL


def test_model_dims_b64_four_rows():
    sdp, _, (x, x_mask, w, e_q, _), _, ref = model_dims(0)
    gen = torch.Generator().manual_seed(64)
    lengths = torch.randint(1, 151, (64,), generator=gen)
    xm = mask_of(lengths, 150)
    xb = torch.randn(64, 192, 150, generator=gen) * xm
    wb = torch.randint(1, 13, (64, 1, 150), generator=gen).float() * xm
    eb = torch.randn(64, 2, 150, generator=gen)
    rows = [0, 21, 42, 63]
    for i, r in enumerate(rows):
        xb[r], xm[r], wb[r], eb[r] = x[i], x_mask[i], w[i], e_q[i]
    nll, terms, z = run_parts(sdp, xb, xm, wb, eb)
    assert bool(torch.isfinite(nll).all()) and bool((nll > 0).all())
    check((nll[rows], terms[rows], z[rows]), ref, "b64 rows")


def test_neighbour_independence_and_repeatability():
    """Every utterance of the padded batch is bit for bit what it gets alone at T = its own length; a second call gives the same bits."""
    sdp, _, (x, x_mask, w, e_q, g), got, _ = model_dims(4)
    again = run_parts(sdp, x, x_mask, w, e_q, g)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two identical calls differ"
    for b, n in enumerate([150, 149, 64, 2]):
        alone = run_parts(sdp, x[b:b + 1, :, :n], x_mask[b:b + 1, :, :n], w[b:b + 1, :, :n], e_q[b:b + 1, :, :n], g[b:b + 1])
        assert torch.equal(alone[0][0], got[0][b]) and torch.equal(alone[1][0], got[1][b]), b
        assert torch.equal(alone[2][0], got[2][b, :, :n]) and float(got[2][b, :, n:].abs().sum()) == 0.0, b


def test_carved_workspace_fits_the_reported_bytes(monkeypatch):
    """ttsvits_durnll_forward at the golden small dims, (B, T) = (2, 37), with g: nothing is written outside
    ttsvits_durnll_workspace_bytes, and the result is that of a roomy workspace bit for bit."""
    from hip_helpers import assert_workspace_fits
    from torch_tts_amd.engine import Handle

    sdp, _ = small_sdp(4)
    x, x_mask, w, e_q = small_case(37, [37, 20], 3)
    g = torch.randn(2, 4, 1, generator=torch.Generator().manual_seed(4)).cuda()

    def run():
        with torch.no_grad():
            out = sdp.nll_cl(x.transpose(1, 2).contiguous().cuda(), torch.tensor([37, 20], dtype=torch.int32).cuda(), w[:, 0].contiguous().cuda(), g,
                             noise=e_q, parts=True)
        return torch.cat([t.reshape(-1) for t in out])

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


class LossNet(AlignNet):
    """AlignNet and the duration predictor: what vits2.duration_loss reads of a SynthesizerTrn."""

    def __init__(self, d, use_sdp, n_speakers, gin_channels):
        super().__init__(d, n_speakers, gin_channels)
        V = _T().vits2
        self.dp = (V.StochasticDurationPredictor(d["hidden_channels"], 192, 3, 0.5, 4, gin_channels=gin_channels) if use_sdp else
                   V.DurationPredictor(d["hidden_channels"], 256, 3, 0.5, gin_channels=gin_channels))


def loss_net(meta, name):
    c = meta["models"][name]
    net = LossNet(meta["net"], c["use_sdp"], c["n_speakers"], c["gin_channels"])
    assert sorted(c["seeds"]) == sorted(p for p in ("enc_p", "enc_q", "flow", "dp", "emb_g") if hasattr(net, p))
    for part, seed in c["seeds"].items():
        randomize(getattr(net, part), seed)
        assert same_checksum(getattr(net, part), c["checksums"][part]), (name, part)
    return net.cuda().eval()


@pytest.mark.parametrize("name", ["model_sdp", "model_dp", "model_sdp_g"])
def test_duration_loss_golden(name):
    sd, meta = load_golden()
    c = meta["models"][name]
    net = loss_net(meta, name)
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    sid = k("sid").cuda() if c["n_speakers"] else None
    noise = (k("e_post").cuda(), k("e_q"), k("e_w")) if c["use_sdp"] else (k("e_post").cuda(), None, None)
    with torch.no_grad():
        l_length, attn, x_mask, (hidden_x, logw, logw_) = _T().vits2.duration_loss(net, k("x").cuda(), k("x_lengths").cuda(), k("y").cuda(),
                                                                                   k("y_lengths").cuda(), sid, noise=noise)
    print(name, "l_length", rel(l_length.cpu(), k("l_length")), "logw", rel(logw.cpu(), k("logw")), "loss_dur", float(l_length.sum()), c["loss_dur"])
    assert l_length.shape == (4,) and attn.shape == k("attn").shape and logw.shape == logw_.shape == (4, 1, 9)
    assert torch.equal(attn.cpu(), k("attn").float())
    assert torch.equal(x_mask.cpu(), mask_of(k("x_lengths"), 9))
    torch.testing.assert_close(logw_.cpu(), k("logw_"), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(hidden_x.cpu(), k("hidden_x"), rtol=RTOL, atol=10 * ATOL)
    assert rel(logw.cpu(), k("logw")) <= LOGW_REL
    assert rel(l_length.cpu(), k("l_length")) <= NLL_REL
    assert abs(float(l_length.sum()) - c["loss_dur"]) <= NLL_REL * (0.1 + abs(c["loss_dur"]))


def test_duration_loss_refuses_a_predictor_that_is_not_a_drop_in():
    sd, meta = load_golden()
    net = loss_net(meta, "model_dp")
    net.dp = torch.nn.Conv1d(32, 1, 1).cuda()
    k = lambda n: sd[f"model_dp/{n}"]  # noqa: E731
    with torch.no_grad(), pytest.raises(TypeError):
        _T().vits2.duration_loss(net, k("x").cuda(), k("x_lengths").cuda(), k("y").cuda(), k("y_lengths").cuda())
    with torch.no_grad(), pytest.raises(ValueError):
        _T().vits2.duration_loss(loss_net(meta, "model_dp"), k("x").cuda(), k("x_lengths").cuda(), k("y").cuda(), k("y_lengths").cuda(),
                                 noise=(k("e_post"), None))
