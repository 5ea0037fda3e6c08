"""GPU parity of VITS2 voice conversion (vits2/models.py:1328-1336): the posterior encoder (ttspost_*), the flow's forward direction
(ttsvits_flow_forward) and vits2.voice_conversion against (a) the reference's own outputs (tests/golden/make_golden_vc.py) and (b) the
torch-op restatement of tests/test_vc_host.py evaluated in fp64, at the ModelConfig dims and the shapes the timing quotes."""
import ctypes as C

import pytest
import torch

from oracle import vits2_oracle as V
from test_duration_host import randomize
from test_vc_host import _cast, flow_dims, flow_forward, load_golden, posterior_encoder, vc_net, voice_conversion, weights

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
RAGGED = ([600, 411, 87, 2], 600)


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{what}: max abs err {err.max().item():.3e} (ref max {b.abs().max().item():.3e}), {int(bad.sum())} elements out"


def _T():
    import torch_tts_amd as T

    return T


def _padded_zero(x_cl, lengths, what):
    for b, n in enumerate(lengths.tolist()):
        assert float(x_cl[b, n:].abs().max()) == 0.0 if n < x_cl.shape[1] else True, (what, b)


def _post(spec, gin, seed, n_layers=16, inter=192, hidden=192):
    pe = randomize(_T().vits2.PosteriorEncoder(spec, inter, hidden, 5, 1, n_layers, gin_channels=gin), seed)
    return pe.cuda().eval()


def _flow(gin, seed, channels=192, hidden=192, n_layers=4):
    fl = _T().vits2.ResidualCouplingTransformersBlock(channels, hidden, 5, 1, n_layers, gin_channels=gin, use_transformer_flows=True)
    return randomize(fl, seed).cuda().eval()


def _wts(mod, prefix=""):
    return {prefix + k: v.detach().double() for k, v in mod.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. posterior encoder
# ---------------------------------------------------------------------------------------------------------------------------
def test_posterior_encoder_golden():
    sd, meta = load_golden()
    p = meta["post"]
    T = _T()
    for S in p["spec"]:
        for gin in p["gin"]:
            for prec in ("f32", "split_f16"):
                pe = T.vits2.PosteriorEncoder(S, p["inter"], p["hidden"], p["kernel"], 1, p["n_layers"], gin_channels=gin)
                pe.load_state_dict(weights(sd, f"post{S}_{gin}"))
                pe = pe.cuda().eval()
                pe.precision = prec
                g = sd["post/g8"].cuda() if gin else None
                with torch.no_grad():
                    z, m, logs, x_mask = pe(sd[f"post{S}/y"].cuda(), sd[f"post{S}/lengths"].cuda(), g=g, noise=sd["post/noise"].cuda())
                for name, a in dict(z=z, m=m, logs=logs, x_mask=x_mask).items():
                    _close(a, sd[f"post{S}_{gin}/{name}"], f"post S={S} gin={gin} {prec} {name}")


def _post_case(pe, B, T, lengths, gin, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(B, pe.in_channels, T, generator=gen).cuda()
    lens = torch.tensor(lengths).cuda()
    g = torch.randn(B, gin, 1, generator=gen).cuda() if gin else None
    noise = torch.randn(B, pe.out_channels, T + 3, generator=gen).cuda()  # (eps_T > T: the stride is honoured)
    with torch.no_grad():
        z, m, logs = pe.forward_cl(y, lens, g=g, noise=noise)
    ref = posterior_encoder(_wts(pe), y.double(), lens, None if g is None else g.double(), noise.double(), pe.n_layers, pe.kernel_size)
    for name, a, r in zip(("z", "m", "logs"), (z, m, logs), ref[:3]):
        _close(a, r.transpose(1, 2), f"{name} B={B} T={T} S={pe.in_channels} gin={gin} {pe.precision}")
        _padded_zero(a, lens, name)


@pytest.mark.parametrize("spec", [80, 513])
@pytest.mark.parametrize("gin", [0, 256])
@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_posterior_encoder_modelconfig_ragged(spec, gin, prec):
    pe = _post(spec, gin, 400 + spec + gin)
    pe.precision = prec
    _post_case(pe, 4, RAGGED[1], RAGGED[0], gin, 1)


def test_posterior_encoder_long_and_benchmark_shapes():
    pe = _post(513, 256, 7)
    _post_case(pe, 1, 1000, [1000], 256, 2)
    pe80 = _post(80, 256, 8)
    for prec in ("f32", "split_f16"):
        pe80.precision = prec
        _post_case(pe80, 64, 600, [600 - 9 * i for i in range(64)], 256, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the flow's forward direction, 3. round trip
# ---------------------------------------------------------------------------------------------------------------------------
def test_flow_forward_golden():
    sd, meta = load_golden()
    f = meta["flow"]
    T = _T()
    for prec in ("f32", "split_f16"):
        fl = T.vits2.ResidualCouplingTransformersBlock(f["channels"], f["hidden"], f["kernel"], 1, f["n_layers"], f["n_flows"], gin_channels=f["gin"],
                                                       use_transformer_flows=True)
        missing, unexpected = fl.load_state_dict(weights(sd, "flow"), strict=False)
        assert not unexpected and all("post_transformer" in k for k in missing)
        fl = fl.cuda().eval()
        fl.precision = prec
        lens = torch.tensor(f["lengths"]).cuda()
        with torch.no_grad():
            out = fl.forward_cl(sd["flow/x"].transpose(1, 2).cuda(), lens, sd["flow/g"].cuda())
        _close(out, sd["flow/out"].transpose(1, 2), f"flow forward {prec}")


def _flow_case(fl, B, T, lengths, gin, seed):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lengths)
    mask = V.sequence_mask(lens, T).unsqueeze(1).double()
    x = torch.randn(B, fl.channels, T, generator=gen, dtype=torch.float64) * mask
    g = torch.randn(B, gin, 1, generator=gen, dtype=torch.float64) if gin else None
    x_cl = x.transpose(1, 2).float().contiguous().cuda()
    with torch.no_grad():
        out = fl.forward_cl(x_cl, lens.cuda(), None if g is None else g.float().cuda())
        back = fl.reverse_cl(out, lens.cuda(), None if g is None else g.float().cuda())
    d = flow_dims(fl.channels, fl.hidden_channels, fl.kernel_size, fl.n_layers, fl.n_flows, gin)
    ref = flow_forward(x.float().double().cuda(), mask.cuda(), _wts(fl, "flow."), d, g=None if g is None else g.float().double().cuda())
    _close(out, ref.transpose(1, 2), f"flow forward B={B} T={T} {fl.precision}")
    _padded_zero(out, lens, "flow forward")
    # 3. round trip: reverse(forward(x)) = x on the valid frames, padded frames stay zero
    _close(back, x_cl, f"round trip B={B} T={T} {fl.precision}", rtol=1e-5, atol=1e-5)
    _padded_zero(back, lens, "round trip")


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_flow_forward_modelconfig_ragged(prec):
    fl = _flow(256, 21)
    fl.precision = prec
    _flow_case(fl, 4, RAGGED[1], RAGGED[0], 256, 4)


def test_flow_forward_long_and_benchmark_shapes():
    fl = _flow(256, 22)
    _flow_case(fl, 1, 1000, [1000], 256, 5)
    _flow_case(fl, 64, 600, [600 - 9 * i for i in range(64)], 256, 6)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. voice_conversion
# ---------------------------------------------------------------------------------------------------------------------------
def test_voice_conversion_golden():
    sd, meta = load_golden()
    net = vc_net(meta).cuda()
    with torch.no_grad():
        o_hat, y_mask, (z, z_p, z_hat) = _T().vits2.voice_conversion(net, sd["vc/y"].cuda(), sd["vc/lengths"].cuda(), sd["vc/sid_src"].cuda(),
                                                                     sd["vc/sid_tgt"].cuda(), noise=sd["vc/noise"].cuda())
    for name, a in dict(o_hat=o_hat, y_mask=y_mask, z=z, z_p=z_p, z_hat=z_hat).items():
        _close(a, sd[f"vc/{name}"], f"vc {name}")


MODELCONFIG = dict(spec_channels=513, inter_channels=192, hidden_channels=192, resblock="1", resblock_kernel_sizes=[3, 7, 11],
                   resblock_dilation_sizes=[[1, 3, 5]] * 3, upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512,
                   upsample_kernel_sizes=[16, 16, 4, 4])


def _modelconfig_net():
    from test_vc_host import VcNet

    net = VcNet(MODELCONFIG, 3, 256)
    for i, part in enumerate(("enc_q", "flow", "dec", "emb_g")):
        randomize(getattr(net, part), 500 + i)
    with torch.no_grad():  # logs of O(0.1) (16 WN layers' skip sums would otherwise make exp(logs) ~ 50 and z ~ 100)
        net.enc_q.proj.weight.mul_(0.1)
    return net.cuda().eval()


def test_voice_conversion_modelconfig_ragged():
    net = _modelconfig_net()
    gen = torch.Generator().manual_seed(9)
    B, T = 2, 160
    y = torch.randn(B, 513, T, generator=gen).cuda()
    lens = torch.tensor([160, 97]).cuda()
    sid_src, sid_tgt = torch.tensor([0, 2]).cuda(), torch.tensor([1, 0]).cuda()
    noise = torch.randn(B, 192, T, generator=gen).cuda()
    with torch.no_grad():
        o_hat, y_mask, (z, z_p, z_hat) = _T().vits2.voice_conversion(net, y, lens, sid_src, sid_tgt, noise=noise)
        ref = voice_conversion(net, y, lens, sid_src, sid_tgt, noise)
    assert o_hat.shape == (B, 1, T * 256)
    _close(y_mask, ref[1], "y_mask")
    for name, a, r in zip(("z", "z_p", "z_hat"), (z, z_p, z_hat), ref[2]):
        _close(a, r, f"vc {name}")
    _close(o_hat, ref[0], "vc o_hat")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. neighbour independence, 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_other_rows():
    net = _modelconfig_net()
    gen = torch.Generator().manual_seed(11)
    B, T = 3, 120
    y = torch.randn(B, 513, T, generator=gen).cuda()
    noise = torch.randn(B, 192, T, generator=gen).cuda()
    lens = torch.tensor([120, 75, 31]).cuda()
    sid_src, sid_tgt = torch.tensor([0, 1, 2]).cuda(), torch.tensor([2, 2, 0]).cuda()
    y2, noise2 = y.clone(), noise.clone()
    y2[1:] = torch.randn(B - 1, 513, T, generator=gen).cuda()
    noise2[1:] = torch.randn(B - 1, 192, T, generator=gen).cuda()
    lens2, sid2 = torch.tensor([120, 120, 9]).cuda(), torch.tensor([2, 0, 1]).cuda()  # (row 0: the same target speaker)
    with torch.no_grad():
        a = _T().vits2.voice_conversion(net, y, lens, sid_src, sid_tgt, noise=noise)
        b = _T().vits2.voice_conversion(net, y2, lens2, sid_src, sid2, noise=noise2)
    assert torch.equal(a[0][0], b[0][0])
    for x1, x2 in zip(a[2], b[2]):
        assert torch.equal(x1[0], x2[0])


def test_refusals():
    from torch_tts_amd import _lib

    pe = _post(80, 0, 3, n_layers=2)
    y, lens = torch.zeros(1, 80, 8).cuda(), torch.tensor([8]).cuda()
    with torch.no_grad(), pytest.raises(ValueError):
        pe(y, lens, g=torch.zeros(1, 4, 1).cuda())
    with pytest.raises(NotImplementedError):
        pe(y, lens)  # grad mode with parameters that require grad
    with torch.no_grad(), pytest.raises(NotImplementedError):
        pe.cpu()(y.cpu(), lens.cpu())
    pe = pe.cuda()
    with torch.no_grad():
        pe(y, lens)  # packs the blob
    eng = pe._engines.get(pe._cfg, y.device)
    lib = eng._lib
    z = torch.empty(1, 8, 192, device="cuda")
    eps = torch.zeros(1, 192, 8, device="cuda")
    g = torch.zeros(1, 4, device="cuda")
    nbytes = int(lib.ttspost_workspace_bytes(eng._h, 1, 8))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = lambda gp, n: (eng._h, y.data_ptr(), lens.to(torch.int32).data_ptr(), gp, eps.data_ptr(), 8, 1, 8, z.data_ptr(), z.data_ptr(),  # noqa: E731
                          z.data_ptr(), ws.data_ptr(), n, None)
    assert lib.ttspost_forward(*args(g.data_ptr(), nbytes)) == _lib.ERR_INVALID_ARG  # g on a gin-0 handle
    assert lib.ttspost_forward(*args(None, nbytes - 256)) == _lib.ERR_WORKSPACE  # short workspace
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the one-element (W = 1) kernels of the flow: a z / out that is only 4-byte aligned; 8. the reported workspace size is the layout
# ---------------------------------------------------------------------------------------------------------------------------
SMALL_B, SMALL_T, SMALL_LENGTHS = 2, 37, [37, 5]
PATTERN = 0xA5


def _small_flow(prec):
    """The flow of the golden fixture (four couplings, gin 8) with its inputs at B = 2, T = 37: -> module, z [B, T, C], lengths, g."""
    sd, meta = load_golden()
    f = meta["flow"]
    fl = _T().vits2.ResidualCouplingTransformersBlock(f["channels"], f["hidden"], f["kernel"], 1, f["n_layers"], f["n_flows"], gin_channels=f["gin"],
                                                      use_transformer_flows=True)
    fl.load_state_dict(weights(sd, "flow"), strict=False)
    fl = fl.cuda().eval()
    fl.precision = prec
    assert fl.n_flows >= 2
    gen = torch.Generator().manual_seed(31)
    z = torch.randn(SMALL_B, SMALL_T, f["channels"], generator=gen).cuda()
    g = torch.randn(SMALL_B, f["gin"], generator=gen).cuda()
    return fl, z, torch.tensor(SMALL_LENGTHS, dtype=torch.int32).cuda(), g


def _one_float_in(t, tail=4):
    """t's values in a contiguous view one float into a larger buffer (4-byte, not 16-byte aligned); -> view, the floats behind it."""
    buf = torch.empty(t.numel() + 1 + tail, device=t.device).view(torch.uint8).fill_(PATTERN).view(torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v, buf[1 + t.numel():]


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_flow_misaligned_input_equals_aligned(prec):
    fl, z, lens, g = _small_flow(prec)
    zm, _ = _one_float_in(z)
    assert z.data_ptr() % 16 == 0 and torch.equal(zm, z)
    with torch.no_grad():
        for run in (fl.forward_cl, fl.reverse_cl):  # the first coupling takes the W = 1 split, residual and coupling, the later ones W = 4
            want, got = run(z, lens, g), run(zm, lens, g)
            assert torch.equal(got, want), (prec, run.__name__, float((got - want).abs().max()))
            assert float(want.abs().max()) > 0


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_flow_forward_misaligned_output_equals_aligned(prec):
    from torch_tts_amd import _lib

    fl, z, lens, g = _small_flow(prec)
    with torch.no_grad():
        want = fl.forward_cl(z, lens, g)
        eng = fl._engine(z)
    nbytes = int(eng._lib.ttsvits_flow_workspace_bytes(eng._h, SMALL_B, SMALL_T))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out, behind = _one_float_in(torch.zeros_like(z))  # (only a direct call reaches the W = 1 flip copy-out: the wrapper allocates out)
    rc = eng._lib.ttsvits_flow_forward(eng._h, z.data_ptr(), lens.data_ptr(), g.data_ptr(), SMALL_B, SMALL_T, out.data_ptr(), ws.data_ptr(), nbytes,
                                       None)
    torch.cuda.synchronize()
    assert rc == _lib.OK
    assert torch.equal(out, want)
    assert behind.numel() == 4 and bool((behind.view(torch.uint8) == PATTERN).all())


def _size_is_the_layout(nbytes, run):
    """run(workspace pointer, bytes) -> rc, outputs: with exactly the reported bytes the call succeeds, computes what it computes in a
    much larger workspace and leaves the bytes behind them alone; with one byte less it is refused."""
    from torch_tts_amd import _lib

    big = torch.zeros(4 * nbytes + (1 << 20), dtype=torch.uint8, device="cuda")
    rc, want = run(big.data_ptr(), big.numel())
    assert rc == _lib.OK
    buf = torch.full((nbytes + 4096,), PATTERN, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    rc, got = run(buf.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert rc == _lib.OK
    for a, b in zip(got, want):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
    assert bool((buf[nbytes:] == PATTERN).all())
    rc, _ = run(buf.data_ptr(), nbytes - 1)
    assert rc == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_reported_workspace_size_is_the_layout(prec):
    B, T = SMALL_B, SMALL_T
    gen = torch.Generator().manual_seed(32)
    # the flow (g given: cond, the last buffer, is in use)
    fl, z, lens, g = _small_flow(prec)
    with torch.no_grad():
        eng = fl._engine(z)  # packs the blob
    lib = eng._lib

    def run_flow(ws, n):
        out = torch.empty_like(z)
        return lib.ttsvits_flow_forward(eng._h, z.data_ptr(), lens.data_ptr(), g.data_ptr(), B, T, out.data_ptr(), ws, n, None), (out,)

    _size_is_the_layout(int(lib.ttsvits_flow_workspace_bytes(eng._h, B, T)), run_flow)
    # the text encoder (g given: the projected speaker embedding is its last buffer)
    te = randomize(_T().vits2.TextEncoder(23, 16, 32, 48, 2, 3, 3, 0.1, gin_channels=8), 33).cuda().eval()
    te.precision = prec
    ids = torch.randint(0, 23, (B, T), generator=gen).cuda()
    with torch.no_grad():
        te.forward_cl(ids, lens, g)  # packs the blob
    et = te._engines.get(te._dims(), ids.device)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run_text(ws, n):
        x, m, logs = torch.empty(B, T, 32, device="cuda"), torch.empty(B, T, 16, device="cuda"), torch.empty(B, T, 16, device="cuda")
        rc = lib.ttsvits_text_encoder(et._h, ids.data_ptr(), lens.data_ptr(), g.data_ptr(), B, T, x.data_ptr(), m.data_ptr(), logs.data_ptr(), ws, n,
                                      None, status.data_ptr())
        return rc, (x, m, logs)

    _size_is_the_layout(int(lib.ttsvits_text_encoder_workspace_bytes(et._h, B, T)), run_text)
    assert int(status) == 0
    # the posterior encoder (13 spectrogram channels: padded to 16)
    pe = _post(13, 8, 34, n_layers=3, inter=8, hidden=16)
    pe.precision = prec
    y = torch.randn(B, 13, T, generator=gen).cuda()
    eps = torch.randn(B, 8, T, generator=gen).cuda()
    with torch.no_grad():
        pe.forward_cl(y, lens, g, noise=eps)  # packs the blob
    ep = pe._engines.get(pe._cfg, y.device)

    def run_post(ws, n):
        zml = [torch.empty(B, T, 8, device="cuda") for _ in range(3)]
        rc = lib.ttspost_forward(ep._h, y.data_ptr(), lens.data_ptr(), g.data_ptr(), eps.data_ptr(), T, B, T, zml[0].data_ptr(), zml[1].data_ptr(),
                                 zml[2].data_ptr(), ws, n, None)
        return rc, zml

    _size_is_the_layout(int(lib.ttspost_workspace_bytes(ep._h, B, T)), run_post)
