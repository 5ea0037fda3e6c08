"""GPU parity of the VITS2 duration discriminators (ttsvits_durdisc_* through torch_tts_amd.DurationDiscriminatorV1 / V2 and
vits2.duration_discriminator_scores) against the fp64 restatement of tests/test_durdisc_host.py and the reference's recorded
outputs.  The bar is the project's rtol 1e-4 / atol 1e-5 (tests/test_disc_host.py), on logits, probabilities and trunk output."""
import copy
import functools

import pytest
import torch

import recipes
from test_durdisc_host import ATOL, RTOL, SHAPES, _close, length_mask, load_golden, make_net, shape_case

pytestmark = pytest.mark.gpu

CASES = [(v, s) for v in (1, 2) for s in SHAPES]  # (the table: tests/test_durdisc_host.py, which also holds its margin condition)


def _V():
    import torch_tts_amd as T

    return T.vits2


@functools.lru_cache(maxsize=None)
def case(version, shape):
    """The module on the device, its inputs, and the oracle's results - computed once and shared, never modified."""
    c = shape_case(version, shape)
    net = copy.deepcopy(c["net"])
    return dict(net=net.cuda(), x=c["x"].cuda(), mask=c["mask"].cuda(), dur_r=c["dur_r"].cuda(), dur_hat=c["dur_hat"].cuda(), lengths=c["lengths"],
                h=c["h"], logits=c["logits"], probs=c["probs"], bias=net.state_dict()["output_layer.0.bias"].double().cpu())


def _pair(version, out):
    """forward's nesting: [p_r, p_hat] for V1, [[p_r], [p_hat]] for V2."""
    assert isinstance(out, list) and len(out) == 2
    if version == 2:
        assert all(isinstance(o, list) and len(o) == 1 for o in out)
        return out[0][0], out[1][0]
    return out[0], out[1]


@pytest.mark.parametrize("version,shape", CASES)
def test_parity_with_the_fp64_restatement(version, shape):
    c = case(version, shape)
    net, B, T_ = c["net"], len(c["lengths"]), SHAPES[shape][2]
    with torch.no_grad():
        p_r, p_hat = _pair(version, net(c["x"], c["mask"], c["dur_r"], c["dur_hat"]))
        h = net.trunk(c["x"], c["mask"])
        prob, logit = net.probabilities(h, c["mask"], [c["dur_r"], c["dur_hat"]], with_logits=True)
        # forward_probability on the ORACLE's trunk output, unmasked as the reference hands it over
        q_hat = net.forward_probability(c["h"].float().cuda(), c["mask"], c["dur_hat"])
    assert p_r.shape == p_hat.shape == q_hat.shape == (B, T_, 1) and h.shape == c["h"].shape and prob.shape == logit.shape == (2, B, T_)
    _close(h, c["h"] * c["mask"].cpu().double(), f"v{version} {shape} trunk (times the mask)")
    for j, (p, side) in enumerate(((p_r, "r"), (p_hat, "hat"))):
        _close(logit[j].unsqueeze(-1), c["logits"][j], f"v{version} {shape} logit_{side}")
        _close(p, c["probs"][j], f"v{version} {shape} prob_{side}")
        assert torch.equal(prob[j].unsqueeze(-1), p)  # (forward is trunk + probabilities)
    _close(q_hat, c["probs"][1], f"v{version} {shape} forward_probability on the oracle's trunk")


@pytest.mark.parametrize("version", (1, 2))
def test_masked_tokens_give_sigmoid_of_the_bias_and_are_never_read(version):
    c = case(version, "c192")
    net, m = c["net"], c["mask"]
    masked = (m[:, 0] == 0)
    assert int(masked.sum()) == 17 + 36
    with torch.no_grad():
        h = net.trunk(c["x"], m)
        prob, logit = net.probabilities(h, m, [c["dur_r"], c["dur_hat"]], with_logits=True)
        for j in range(2):
            _close(logit[j][masked], c["bias"].expand(int(masked.sum())), f"v{version} masked logit {j}")
            _close(prob[j][masked], torch.sigmoid(c["bias"]).expand(int(masked.sum())), f"v{version} masked probability {j}")
        assert torch.equal(h.transpose(1, 2)[masked], torch.zeros_like(h.transpose(1, 2)[masked]))
        # NaN at the masked tokens of x, of both durations and of the trunk output changes no bit
        nan = torch.full((), float("nan"), device=m.device)
        poison = lambda t: torch.where(m.expand_as(t) == 0, nan, t)  # noqa: E731
        want = net(c["x"], m, c["dur_r"], c["dur_hat"])
        got = net(poison(c["x"]), m, poison(c["dur_r"]), poison(c["dur_hat"]))
        for a, b in zip(_pair(version, want), _pair(version, got)):
            assert torch.equal(a, b) and bool(torch.isfinite(b).all())
        assert torch.equal(net.trunk(poison(c["x"]), m), h)
        assert torch.equal(net.forward_probability(poison(h), m, poison(c["dur_r"]))[..., 0], prob[0])


@pytest.mark.parametrize("version,shape", [(1, "c192"), (2, "c192"), (2, "c24f40")])
def test_same_bits_twice_alone_and_per_duration(version, shape):
    c = case(version, shape)
    net, m = c["net"], c["mask"]
    with torch.no_grad():
        p_r, p_hat = _pair(version, net(c["x"], m, c["dur_r"], c["dur_hat"]))
        again = _pair(version, net(c["x"], m, c["dur_r"], c["dur_hat"]))
        assert torch.equal(again[0], p_r) and torch.equal(again[1], p_hat)
        # n_dur = 2 gives the bits of two n_dur = 1 calls
        h = net.trunk(c["x"], m)
        assert torch.equal(net.forward_probability(h, m, c["dur_r"]), p_r) and torch.equal(net.forward_probability(h, m, c["dur_hat"]), p_hat)
        # every utterance of the padded batch, alone at its own length
        for b, n in enumerate(c["lengths"]):
            one = lambda t: t[b:b + 1, :, :n].contiguous()  # noqa: E731
            a_r, a_hat = _pair(version, net(one(c["x"]), one(m), one(c["dur_r"]), one(c["dur_hat"])))
            assert torch.equal(a_r[0], p_r[b, :n]) and torch.equal(a_hat[0], p_hat[b, :n]), (version, shape, b)
            assert torch.equal(net.trunk(one(c["x"]), one(m))[0], h[b, :, :n])


@pytest.mark.parametrize("version", (1, 2))
def test_same_bits_alone_and_in_a_batch_past_the_gemm_cores_tile_switch(version):
    """The GEMM core picks its exact-fp32 tile by size: 64 x 64 K-sequential from 512 tiles on, 32 x 32 split-K below - another
    summation order.  With F = 40 (one column tile) that is M >= 32 705 rows; a batch of 2 x 33 000 tokens is past it in every
    conv (66 000 rows, 132 000 in pre_out_conv_2), its 5-token utterance alone (5 and 10 rows) far below.  The discriminators pin
    the tile (GemmArgs::fixed_tile), so the utterance still gets the bits it gets alone; K = 120 of the F -> F convs spans all
    four K slices of the split-K tile, so the two orders would differ."""
    C, F, T_, lengths = 8, 40, 33000, [33000, 5]
    net = make_net(version, C, F, 900 + version).cuda()
    x = recipes.seeded_randn(901, 2, C, T_).cuda()
    dur_r = torch.log(recipes.seeded_ids(902, 8, 2, 1, T_, low=1).float()).cuda()
    dur_hat = (0.8 + 0.7 * recipes.seeded_randn(903, 2, 1, T_)).cuda()
    m = length_mask(lengths, T_).cuda()
    with torch.no_grad():
        p_r, p_hat = _pair(version, net(x, m, dur_r, dur_hat))
        h = net.trunk(x, m)
        n = lengths[1]
        one = lambda t: t[1:2, :, :n].contiguous()  # noqa: E731
        a_r, a_hat = _pair(version, net(one(x), one(m), one(dur_r), one(dur_hat)))
        assert torch.equal(a_r[0], p_r[1, :n]) and torch.equal(a_hat[0], p_hat[1, :n])
        assert torch.equal(net.trunk(one(x), one(m))[0], h[1, :, :n])
        # n_dur = 2 (132 000 rows in pre_out_conv_2) against n_dur = 1 (66 000)
        assert torch.equal(net.forward_probability(h, m, dur_hat), p_hat)
    assert bool(torch.isfinite(p_r).all()) and not torch.equal(p_r[1, :n], p_hat[1, :n])


@pytest.mark.parametrize("version", (1, 2))
def test_swapped_durations_give_swapped_outputs(version):
    c = case(version, "c24f40")
    with torch.no_grad():
        p_r, p_hat = _pair(version, c["net"](c["x"], c["mask"], c["dur_r"], c["dur_hat"]))
        s_r, s_hat = _pair(version, c["net"](c["x"], c["mask"], c["dur_hat"], c["dur_r"]))
    assert torch.equal(s_r, p_hat) and torch.equal(s_hat, p_r) and not torch.equal(p_r, p_hat)


def test_golden_outputs_and_losses():
    """The reference's recorded outputs, through the Python classes: probabilities, logits, trunk samples, and the recorded loss
    values through vits2.discriminator_loss / generator_loss on forward's own nesting."""
    V = _V()
    g, meta = load_golden()
    for name, cs in meta["cases"].items():
        x, dur_r, dur_hat = (g[f"{k}/{name}"].cuda() for k in ("x", "dur_r", "dur_hat"))
        mask = length_mask(cs["lengths"], cs["T"]).cuda()
        for v in (1, 2):
            net = make_net(v, cs["in_channels"], cs["filter_channels"], meta["seed"], meta["gain"]).cuda()
            with torch.no_grad():
                out = net(x, mask, dur_r, dur_hat)
                h = net.trunk(x, mask)
                _, logit = net.probabilities(h, mask, [dur_r, dur_hat], with_logits=True)
            p_r, p_hat = _pair(v, out)
            _close(p_r, g[f"prob_r/{name}/v{v}"], f"{name} v{v} prob_r")
            _close(p_hat, g[f"prob_hat/{name}/v{v}"], f"{name} v{v} prob_hat")
            _close(logit[0].unsqueeze(-1), g[f"logit_r/{name}/v{v}"], f"{name} v{v} logit_r")
            _close(logit[1].unsqueeze(-1), g[f"logit_hat/{name}/v{v}"], f"{name} v{v} logit_hat")
            keep = mask.expand_as(h).reshape(-1)[::cs["trunk_stride"]].cpu() == 1  # (the library's trunk is zero at masked tokens)
            _close(h.reshape(-1)[::cs["trunk_stride"]].cpu()[keep], g[f"trunk/{name}/v{v}"][keep], f"{name} v{v} trunk")
            want = cs[f"v{v}"]
            dr, dg = V.discriminator_loss(out[0], out[1])
            f64 = lambda t: torch.tensor(t, dtype=torch.float64)  # noqa: E731
            torch.testing.assert_close(dr.cpu().double(), f64(want["discriminator_loss"][0]), rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(dg.cpu().double(), f64(want["discriminator_loss"][1]), rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(V.generator_loss(out[1]).cpu().double(), f64(want["generator_loss"]), rtol=RTOL, atol=ATOL)


def test_module_refusals_on_the_device():
    c = case(2, "c24f40")
    net, x, m, d = c["net"], c["x"], c["mask"], c["dur_r"]
    for p in net.parameters():
        assert p.requires_grad
    with pytest.raises(NotImplementedError, match="inference-only"):
        net(x, m, d, d)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="fp32"):
            net(x.double(), m, d, d)
        with pytest.raises(NotImplementedError, match="fp32"):
            net(x, m, d.double(), d)
        with pytest.raises(NotImplementedError):
            net(x, m, d.cpu(), d)
        # a mask built on the host: refused before any launch (the kernels would read the lengths through a host pointer)
        for call in (lambda: net(x, m.cpu(), d, d), lambda: net.trunk(x, m.cpu()),
                     lambda: net.forward_probability(net.trunk(x, m), m.cpu(), d)):
            with pytest.raises(NotImplementedError, match="x_mask"):
                call()
        again = net(x, m, d, d)  # (and the device is as it was)
        assert bool(torch.isfinite(again[0][0]).all())


@pytest.mark.parametrize("kind", ("sdp", "dp"))
@pytest.mark.parametrize("with_sid", (True, False))
def test_scores_equal_the_pieces_called_separately(kind, with_sid):
    """duration_discriminator_scores on the small SynthesizerTrn-shaped model of tests/test_align_hip.py (drop-ins, weights of
    its fixture) with a duration predictor added: bit for bit forced_alignment + enc_p + dp + net_dur_disc called one by one."""
    from test_align_host import align_net
    from test_align_host import load_golden as load_align

    V = _V()
    sd, meta = load_align()
    t = lambda k: torch.from_numpy(sd[k]).cuda()  # noqa: E731
    net = align_net(meta)
    H, gin = meta["net"]["hidden_channels"], meta["model"]["gin_channels"]
    net.dp = (V.StochasticDurationPredictor(H, 192, 3, 0.5, 4, gin_channels=gin) if kind == "sdp"
              else V.DurationPredictor(H, 48, 3, 0.5, gin_channels=gin)).eval()
    recipes.fill_by_key(net.dp, 611, gain=0.8)
    net = net.cuda()
    x, xl, y, yl, e_q = (t(f"model/{k}") for k in ("x", "x_lengths", "y", "y_lengths", "noise"))
    sid = t("model/sid") if with_sid else None
    e_w = recipes.seeded_randn(612, x.shape[0], 2, x.shape[1]).cuda()
    for version in (1, 2):
        disc = make_net(version, H, 40, 613 + version).cuda()
        with torch.no_grad():
            y_r, y_g, (hidden_x, x_mask, logw_, logw) = V.duration_discriminator_scores(net, disc, x, xl, y, yl, sid, noise_scale_w=0.8,
                                                                                        noise=(e_q, e_w))
            # the pieces
            _, _, want_logw_, _ = V.forced_alignment(net, x, xl, y, yl, sid=sid, noise=e_q)
            g = None if sid is None else net.emb_g(sid).unsqueeze(-1)
            want_x, _, _, want_mask = net.enc_p(x, xl)
            want_logw = (net.dp(want_x, want_mask, g=g, reverse=True, noise_scale=0.8, noise=e_w) if kind == "sdp"
                         else net.dp(want_x, want_mask, g=g))
            want = disc(want_x, want_mask, want_logw_, want_logw)
        B, T_x = x.shape
        assert hidden_x.shape == (B, H, T_x) and x_mask.shape == logw_.shape == logw.shape == (B, 1, T_x)
        for a, b in ((hidden_x, want_x), (x_mask, want_mask), (logw_, want_logw_), (logw, want_logw)):
            assert torch.equal(a, b)
        for a, b in zip(_pair(version, [y_r, y_g]), _pair(version, want)):
            assert a.shape == (B, T_x, 1) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(TypeError):
        V.duration_discriminator_scores(net, torch.nn.Linear(2, 2), x, xl, y, yl)
    del net.dp
    with pytest.raises(TypeError):
        V.duration_discriminator_scores(net, disc, x, xl, y, yl)
