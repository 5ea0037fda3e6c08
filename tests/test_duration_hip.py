"""GPU parity of the VITS2 duration predictors, the length regulator and the whole text -> waveform inference (ttsdur_* through
torch_tts_amd.vits2, exact fp32) against (a) the reference's own outputs at small dims (tests/golden/make_golden_duration.py) and
(b) the fp64 restatement of tests/test_duration_host.py at the ModelConfig dims."""
import pytest
import torch

from test_duration_host import (Net, _rel, dp_forward, infer_net, length_regulate, load_golden, randomize, sdp_reverse, weights)
from test_generator_host import reference_forward

pytestmark = pytest.mark.gpu
LOGW_REL = 1e-4  # the project's bar: |a - b| / (0.1 + |b|)
RTOL, ATOL = 1e-4, 1e-5  # the generator tests' waveform tolerance
FULL = dict(n_vocab=100, inter_channels=192, hidden_channels=192, filter_channels=768, n_heads=2, n_layers=6, kernel_size=3, p_dropout=0.1,
            resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2],
            upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])
GEN_FULL = {k: FULL[k] for k in ("resblock", "resblock_kernel_sizes", "resblock_dilation_sizes", "upsample_rates", "upsample_initial_channel",
                                 "upsample_kernel_sizes")}


def _T():
    import torch_tts_amd as T

    return T


def _mask(lengths, T):
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).unsqueeze(1).float()


def _sdp(width, gin, seed):
    m = _T().StochasticDurationPredictor(width, 192, 3, 0.5, 4, gin_channels=gin)
    randomize(m, seed)
    with torch.no_grad():  # durations of a few frames
        m.flows[0].m.copy_(torch.tensor([[-0.8], [0.0]]))
        m.flows[0].logs.copy_(torch.tensor([[0.4], [0.0]]))
    return m


def test_golden_small_dims():
    sd, meta = load_golden()
    T = _T()
    x, x_mask, noise = sd["case/x"].cuda(), sd["case/x_mask"].cuda(), sd["case/noise"]
    for gin in (0, 4):
        g = sd["case/g4"].cuda() if gin else None
        sdp = T.StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin_channels=gin)
        sdp.load_state_dict(weights(sd, f"sdp{gin}"), strict=True)
        dp = T.DurationPredictor(32, 48, 3, 0.5, gin_channels=gin)
        dp.load_state_dict(weights(sd, f"dp{gin}"), strict=True)
        sdp, dp = sdp.cuda().eval(), dp.cuda().eval()
        with torch.no_grad():
            lw = sdp(x, x_mask, g=g, reverse=True, noise_scale=meta["sdp_noise_scale"], noise=noise)
            lw2 = sdp(x, x_mask, g=g[:, :, 0] if gin else None, reverse=True, noise_scale=meta["sdp_noise_scale"], noise=noise.cuda())
            ld = dp(x, x_mask, g=g)
        assert lw.shape == sd[f"sdp{gin}/logw"].shape and ld.shape == sd[f"dp{gin}/logw"].shape
        assert _rel(lw.cpu(), sd[f"sdp{gin}/logw"]) <= LOGW_REL, (gin, _rel(lw.cpu(), sd[f"sdp{gin}/logw"]))
        assert torch.equal(lw, lw2)
        assert _rel(ld.cpu(), sd[f"dp{gin}/logw"]) <= LOGW_REL, (gin, _rel(ld.cpu(), sd[f"dp{gin}/logw"]))
        assert float(lw[2, 0, 1:].abs().max()) == 0.0 and float(ld[1, 0, 5:].abs().max()) == 0.0  # padded frames


@pytest.mark.parametrize("kind", ["sdp", "dp"])
def test_carved_workspace_fits_the_reported_bytes(kind, monkeypatch):
    """ttsdur_sdp_reverse / ttsdur_dp_forward at the golden small dims, (B, T) = (2, 37), with g: nothing is written outside
    ttsdur_workspace_bytes, and the result is that of a roomy workspace bit for bit."""
    from hip_helpers import assert_workspace_fits
    from torch_tts_amd.engine import Handle

    sd, meta = load_golden()
    T = _T()
    m = T.StochasticDurationPredictor(32, 192, 3, 0.5, 4, gin_channels=4) if kind == "sdp" else T.DurationPredictor(32, 48, 3, 0.5, gin_channels=4)
    m.load_state_dict(weights(sd, f"{kind}4"), strict=True)
    m = m.cuda().eval()
    gen = torch.Generator().manual_seed(3)
    x, g, noise = torch.randn(2, 32, 37, generator=gen).cuda(), torch.randn(2, 4, 1, generator=gen).cuda(), torch.randn(2, 2, 37, generator=gen).cuda()
    x_mask = _mask([37, 20], 37).cuda()

    def run():
        with torch.no_grad():
            return m(x, x_mask, g=g, reverse=True, noise_scale=1.0, noise=noise) if kind == "sdp" else m(x, x_mask, g=g)

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


def _fulldims_case(B=64, T=200, seed=0):
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, T + 1, (B,), generator=g)
    lengths[0], lengths[1], lengths[-1] = 1, T, 2
    x_mask = _mask(lengths, T)
    x = torch.randn(B, 192, T, generator=g) * x_mask
    noise = torch.randn(B, 2, T, generator=g)
    return x, x_mask, lengths, noise


def test_fulldims_b64_against_restatement():
    x, x_mask, lengths, noise = _fulldims_case()
    sdp = _sdp(192, 0, 7)
    sd = {k: v.detach().clone() for k, v in sdp.state_dict().items()}
    dp = randomize(_T().DurationPredictor(192, 256, 3, 0.5), 8)
    dsd = {k: v.detach().clone() for k, v in dp.state_dict().items()}
    sdp, dp = sdp.cuda().eval(), dp.cuda().eval()
    with torch.no_grad():
        lw = sdp(x.cuda(), x_mask.cuda(), reverse=True, noise_scale=0.8, noise=noise).cpu()
        ld = dp(x.cuda(), x_mask.cuda()).cpu()
        again = sdp(x.cuda(), x_mask.cuda(), reverse=True, noise_scale=0.8, noise=noise).cpu()
    assert torch.equal(lw, again), "two identical calls differ"
    ref = sdp_reverse(sd, x, x_mask, noise, 0.8)
    assert _rel(lw, ref) <= LOGW_REL, _rel(lw, ref)
    assert _rel(ld, dp_forward(dsd, x, x_mask)) <= LOGW_REL
    # durations: equal except where the restatement's w lies within 1e-4 of an integer
    eng = sdp._engines.get(sdp._cfg, torch.device("cuda", 0))
    cum, y_len, T_y = eng.lengths(lw[:, 0].cuda(), lengths.to(torch.int32).cuda(), 1.0)
    w_ref = torch.exp(ref) * x_mask
    near = ((w_ref - w_ref.round()).abs() < 1e-4)[:, 0]
    wc = torch.diff(cum.cpu().long(), dim=1, prepend=torch.zeros(64, 1, dtype=torch.long))
    wc_ref = torch.ceil(w_ref[:, 0]).long()
    assert ((wc == wc_ref) | near).all()
    valid = x_mask[:, 0] > 0
    assert float(near[valid].float().mean()) < 0.01 and torch.equal(wc[~valid], wc_ref[~valid])


def test_neighbour_independence():
    x, x_mask, lengths, noise = _fulldims_case(B=5, T=37, seed=3)
    sdp = _sdp(192, 0, 9).cuda().eval()
    dp = randomize(_T().DurationPredictor(192, 256, 3, 0.5), 10).cuda().eval()
    x2, n2 = x.clone(), noise.clone()
    x2[1] = torch.randn_like(x2[1])  # utterance 1: other tokens, and garbage in its padded frames
    n2[1] = torch.randn_like(n2[1])
    x3 = x.clone()
    x3[3, :, int(lengths[3]):] = 5.0  # utterance 3: only its padded frames
    with torch.no_grad():
        a = sdp(x.cuda(), x_mask.cuda(), reverse=True, noise=noise)
        b = sdp(x2.cuda(), x_mask.cuda(), reverse=True, noise=n2)
        c = sdp(x3.cuda(), x_mask.cuda(), reverse=True, noise=noise)
        da, db, dc = dp(x.cuda(), x_mask.cuda()), dp(x2.cuda(), x_mask.cuda()), dp(x3.cuda(), x_mask.cuda())
    for i in (0, 2, 3, 4):
        assert torch.equal(a[i], b[i]) and torch.equal(da[i], db[i]), i
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a, c) and torch.equal(da, dc)


def test_expansion_from_given_logw():
    T = _T()
    sdp = _sdp(32, 0, 11).cuda().eval()
    eng = sdp._engines.get(sdp._cfg, torch.device("cuda", 0))
    gen = torch.Generator().manual_seed(12)
    B, Tx, Cc = 6, 23, 16
    lengths = torch.tensor([23, 1, 7, 15, 2, 23])
    x_mask = _mask(lengths, Tx)
    logw = (torch.rand(B, 1, Tx, generator=gen) * 3 - 1) * x_mask
    logw[4, 0, :2] = -200.0  # an utterance with no frames at all (exp underflows to 0): y_len clamps to 1
    m = torch.randn(B, Tx, Cc, generator=gen)
    logs = torch.randn(B, Tx, Cc, generator=gen) * 0.3
    ls, ns = 1.3, 0.7
    ref = length_regulate(logw, x_mask, m.transpose(1, 2), logs.transpose(1, 2), torch.zeros(B, Cc, 1000), ns, ls)
    T_y = int(ref["y_len"].max())
    e_z = torch.randn(B, Cc, T_y + 5, generator=gen)
    ref = length_regulate(logw, x_mask, m.transpose(1, 2), logs.transpose(1, 2), e_z, ns, ls)
    with torch.no_grad():
        cum, y_len, T_y2 = eng.lengths(logw[:, 0].cuda(), lengths.to(torch.int32).cuda(), ls)
        z_p, m_p, logs_p, attn = eng.expand(cum, m.cuda(), logs.cuda(), e_z.cuda(), ns, T_y2)
    assert T_y2 == T_y and y_len.cpu().tolist() == ref["y_len"].tolist() and y_len[4] == 1
    wc = torch.diff(cum.cpu().long(), dim=1, prepend=torch.zeros(B, 1, dtype=torch.long))
    assert torch.equal(wc, ref["w_ceil"][:, 0].long())
    assert torch.equal(attn.cpu(), ref["attn"][:, 0].float())
    assert torch.equal(m_p.cpu(), ref["m_p"].transpose(1, 2).float()) and torch.equal(logs_p.cpu(), ref["logs_p"].transpose(1, 2).float())
    torch.testing.assert_close(z_p.cpu().double(), ref["z_p"].transpose(1, 2), rtol=1e-6, atol=1e-6)
    # frames without a token (past y_len, and utterance 4's clamped frame): m_p = logs_p = 0, z_p = eps * noise_scale
    for b in range(B):
        n = int(ref["w_ceil"][b].sum())
        assert float(m_p[b, n:].abs().sum()) == 0.0 and float(attn[b, n:].abs().sum()) == 0.0
        torch.testing.assert_close(z_p[b, n:].cpu(), (e_z[b, :, n:T_y] * ns).t(), rtol=0, atol=0)
    # refusals
    with pytest.raises(ValueError, match="non-finite"):
        eng.lengths(torch.full((2, 4), 100.0, device="cuda"), torch.tensor([4, 4], dtype=torch.int32, device="cuda"), 1.0)
    with pytest.raises(ValueError, match="2\\^24"):
        eng.lengths(torch.full((1, 4), 16.0, device="cuda"), torch.tensor([4], dtype=torch.int32, device="cuda"), 1.0)
    with pytest.raises(ValueError):
        eng.expand(cum, m.cuda(), logs.cuda(), e_z[:, :, : T_y - 1].cuda(), ns, T_y)
    assert T is not None


def _infer_net_cuda(meta, name):
    return infer_net(meta, name).cuda().eval()


def test_infer_golden_small_dims():
    sd, meta = load_golden()
    T = _T()
    for name, c in meta["infer"].items():
        net = _infer_net_cuda(meta, name)
        ids, lengths = sd[f"{name}/ids"].cuda(), sd[f"{name}/lengths"].cuda()
        sid = sd[f"{name}/sid"].cuda() if c["n_speakers"] else None
        e_w = sd[f"{name}/e_w"] if c["use_sdp"] else None
        with torch.no_grad():
            o, attn, y_mask, (z, z_p, m_p, logs_p) = T.vits2.infer(net, ids, lengths, sid=sid, **c["args"], noise=(e_w, sd[f"{name}/e_z"].cuda()))
        assert torch.equal(y_mask.cpu(), sd[f"{name}/y_mask"]) and torch.equal(attn.cpu(), sd[f"{name}/attn"]), name
        for k, v in (("m_p", m_p), ("logs_p", logs_p), ("z_p", z_p), ("z", z), ("o", o)):
            ref = sd[f"{name}/{k}"]
            assert v.shape == ref.shape, (name, k, v.shape, ref.shape)
            torch.testing.assert_close(v.cpu().double(), ref.double(), rtol=RTOL, atol=ATOL * 10 if k == "z" else ATOL,
                                       msg=lambda msg: f"{name} {k}: {msg}")


def test_infer_options_are_honoured():
    sd, meta = load_golden()
    T = _T()
    name = "infer_sdp"
    c = meta["infer"][name]
    net = _infer_net_cuda(meta, name)
    ids, lengths = sd[f"{name}/ids"].cuda(), sd[f"{name}/lengths"].cuda()
    e_w, e_z = sd[f"{name}/e_w"], torch.randn(3, 16, 400).cuda()
    base = dict(c["args"])
    with torch.no_grad():
        logw = net.dp.logw_cl(net.enc_p.forward_cl(ids, lengths)[0], lengths.to(torch.int32), None, base["noise_scale_w"], e_w)
        for ls in (0.5, 2.0):
            _, _, y_mask, _ = T.vits2.infer(net, ids, lengths, **dict(base, length_scale=ls), noise=(e_w, e_z))
            w = torch.exp(logw.cpu()) * _mask(lengths.cpu(), ids.shape[1])[:, 0] * ls
            assert y_mask[:, 0].sum(1).long().cpu().tolist() == torch.clamp_min(torch.ceil(w).sum(1), 1).long().tolist(), ls
        # noise_scale_w = 0: the durations no longer depend on the SDP's draw
        a = T.vits2.infer(net, ids, lengths, **dict(base, noise_scale_w=0.0), noise=(e_w, e_z))
        b = T.vits2.infer(net, ids, lengths, **dict(base, noise_scale_w=0.0), noise=(torch.randn_like(e_w), e_z))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        full = T.vits2.infer(net, ids, lengths, **base, noise=(e_w, e_z))
        cut = T.vits2.infer(net, ids, lengths, **base, max_len=5, noise=(e_w, e_z))
        assert cut[0].shape[2] == 5 * 8 and torch.equal(cut[3][0], full[3][0])
        # the reference's draws when no noise is given: torch.randn(B, 2, T) on the CPU generator, then torch.randn_like(m_p)
        torch.manual_seed(5)
        drawn = T.vits2.infer(net, ids, lengths, **base)
        torch.manual_seed(5)
        ew = torch.randn(3, 2, ids.shape[1])
        ez = torch.randn(3, 16, drawn[2].shape[2], device="cuda")
        given = T.vits2.infer(net, ids, lengths, **base, noise=(ew, ez))
        assert torch.equal(drawn[0], given[0])


def test_infer_refuses_a_module_that_is_not_a_drop_in():
    sd, meta = load_golden()
    T = _T()
    net = _infer_net_cuda(meta, "infer_dp")
    net.dp = torch.nn.Conv1d(32, 1, 1).cuda()
    with torch.no_grad(), pytest.raises(TypeError):
        T.vits2.infer(net, sd["infer_dp/ids"].cuda(), sd["infer_dp/lengths"].cuda())


def test_infer_fulldims_b4_against_restatement_chain():
    T = _T()
    torch.manual_seed(21)
    net = Net(FULL, use_sdp=True)
    for i, part in enumerate(("enc_p", "dp", "flow", "dec")):
        randomize(getattr(net, part), 300 + i)
    with torch.no_grad():
        net.dp.flows[0].m.copy_(torch.tensor([[-0.8], [0.0]]))
        net.dp.flows[0].logs.copy_(torch.tensor([[0.4], [0.0]]))
    gsd = {k: v.detach().clone() for k, v in net.dec.state_dict().items()}
    net = net.cuda().eval()
    B, Tx = 4, 30
    lengths = torch.tensor([30, 17, 1, 9])
    ids = torch.randint(0, FULL["n_vocab"], (B, Tx)).cuda()
    e_w = torch.randn(B, 2, Tx)
    e_z = torch.randn(B, 192, 2000).cuda()
    args = dict(noise_scale=0.667, length_scale=1.0, noise_scale_w=0.8)
    with torch.no_grad():
        o, attn, y_mask, (z, z_p, m_p, logs_p) = T.vits2.infer(net, ids, lengths.cuda(), **args, noise=(e_w, e_z))
        # the chain of modules, fed the HIP durations
        xh, m, logs, x_mask = net.enc_p(ids, lengths.cuda())
        logw = net.dp(xh, x_mask, reverse=True, noise_scale=args["noise_scale_w"], noise=e_w)
        lr = length_regulate(logw.cpu(), x_mask.cpu(), m.cpu(), logs.cpu(), e_z.cpu(), args["noise_scale"], args["length_scale"])
        zr = net.flow(lr["z_p"].float().cuda(), lr["y_mask"].float().cuda(), reverse=True)
    assert torch.equal(y_mask.cpu().double(), lr["y_mask"]) and torch.equal(attn.cpu().double(), lr["attn"])
    torch.testing.assert_close(z_p.cpu().double(), lr["z_p"], rtol=1e-6, atol=1e-6)
    o_ref = reference_forward(gsd, GEN_FULL, (zr.cpu() * lr["y_mask"].float()))
    assert o.shape == o_ref.shape
    torch.testing.assert_close(o.cpu().double(), o_ref, rtol=RTOL, atol=ATOL)
    assert float(o.abs().max()) > 0.05
