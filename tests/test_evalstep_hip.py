"""GPU parity of the VITS2 validation step's glue (csrc/evalstep.hip through torch_tts_amd.vits2) against (a) the fp64 restatements
of tests/test_evalstep_host.py at the kernels' edges and (b) the reference's own outputs at small dims
(tests/golden/make_golden_evalstep.py).  The bar on every loss is the project's |a - b| / (0.1 + |b|) <= 1e-4 - at least 4 x the
reference's own fp32-vs-fp64 error recorded in evalstep_meta.json; gathers and slices are compared for equality; no frame and no
utterance is left out of a comparison.

The KL kernel takes 4 frames per workgroup (one per wave), a lane's channels are 256 apart, and an utterance's frame sums are added
by 256 threads: T_y covers 1, 3 / 4 / 5, 63 / 64 / 65, 129 and 255 / 256 / 257, C covers 4, 16, 192 and 260."""
import functools

import pytest
import torch

from test_disc_host import make_mpd
from test_durnll_host import mask_of, rel
from test_evalstep_host import (MODELS, REL, eval_net, frame_token_of, gather_prior, kl_restated, load_golden, slice_restated,
                                sliced_l1_restated)

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5


def _V():
    import torch_tts_amd as T

    return T.vits2


def engine():
    return _V()._align_engine(torch.device("cuda:0"))


def cl(t):
    return t.transpose(1, 2).contiguous().cuda()


def kl_case(B, C, T_y, T_x, seed, t_y=None):
    """z_p, logs_q [B, C, T_y], m_p, logs_p [B, C, T_x], frame_token [B, T_y] and t_y: utterance 0 walks its tokens in random runs
    and fills the width, utterance 1 (when there is one) is padded - t_y < T_y where T_y > 1, -1 tokens from there - and utterance
    2 keeps every frame on token 0 (one long run); the others walk."""
    gen = torch.Generator().manual_seed(seed)
    z_p, logs_q = torch.randn(B, C, T_y, generator=gen), 0.3 * torch.randn(B, C, T_y, generator=gen)
    m_p, logs_p = torch.randn(B, C, T_x, generator=gen), 0.3 * torch.randn(B, C, T_x, generator=gen)
    if t_y is None:
        t_y = [T_y if b != 1 else max(1, T_y // 2) for b in range(B)]
    ft = torch.full((B, T_y), -1, dtype=torch.int32)
    for b in range(B):
        n = t_y[b]
        if b == 2 or n == 0:
            ft[b, :n] = 0
            continue
        tx = min(T_x, n)
        cuts = torch.randperm(n - 1, generator=gen)[:tx - 1].sort().values + 1 if tx > 1 else torch.zeros(0, dtype=torch.long)
        ft[b, :n] = torch.bucketize(torch.arange(n), cuts, right=True).to(torch.int32)
    return z_p, logs_q, m_p, logs_p, ft, torch.tensor(t_y, dtype=torch.int32)


def run_kl(z_p, logs_q, m_p, logs_p, ft, t_y, expand=True):
    with torch.no_grad():
        out = engine().kl_loss(cl(z_p), cl(logs_q), cl(m_p), cl(logs_p), None if ft is None else ft.cuda(), t_y.cuda(), expand)
    return tuple(None if t is None else t.cpu() for t in out)


def check_kl(case, what):
    z_p, logs_q, m_p, logs_p, ft, t_y = case
    kl, rows, m_exp, logs_exp = run_kl(*case)
    want_rows, want_sum, want_kl = kl_restated(z_p, logs_q, m_p, logs_p, t_y, ft)
    errs = {"kl": rel(kl[1], want_kl), "sum": rel(kl[0], want_sum), "rows": rel(rows, want_rows)}
    print(what, errs)
    for k, e in errs.items():
        assert e <= REL, (what, k, e)
    # the reference's expansion: attn @ m_p in fp64, rounded - the one-hot product is the gathered value exactly
    attn = (ft[:, :, None] == torch.arange(m_p.shape[2])[None, None, :]).double()
    for got, p in ((m_exp, m_p), (logs_exp, logs_p)):
        want = torch.matmul(attn, p.double().transpose(1, 2)).float()
        assert torch.equal(got, want), what
        assert torch.equal(got, gather_prior(p, ft).transpose(1, 2)), what
    return kl, rows, m_exp, logs_exp


@pytest.mark.parametrize("T_y", [1, 3, 4, 5, 63, 64, 65, 129, 255, 256, 257])
@pytest.mark.parametrize("C", [4, 16, 192])
def test_kl_edges(C, T_y):
    check_kl(kl_case(3, C, T_y, min(T_y, 7), 1000 * C + T_y), f"C={C} T_y={T_y}")


def test_kl_more_than_one_pass_over_the_channels():
    check_kl(kl_case(3, 260, 9, 4, 5), "C=260")


def test_kl_single_utterance_and_empty_utterance():
    check_kl(kl_case(1, 16, 37, 5, 6), "B=1")
    case = kl_case(3, 16, 12, 5, 7, t_y=[12, 0, 5])
    _, rows, _, _ = check_kl(case, "t_y=0")
    assert float(rows[1]) == 0.0


def test_kl_identity_form_is_the_gathered_form():
    z_p, logs_q, m_p, logs_p, ft, t_y = kl_case(3, 16, 65, 7, 8)
    kl, rows, m_exp, logs_exp = run_kl(z_p, logs_q, m_p, logs_p, ft, t_y)
    kl_i, rows_i, m_i, logs_i = run_kl(z_p, logs_q, m_exp.transpose(1, 2), logs_exp.transpose(1, 2), None, t_y)
    assert torch.equal(kl_i, kl) and torch.equal(rows_i, rows) and torch.equal(m_i, m_exp) and torch.equal(logs_i, logs_exp)
    kl_n, rows_n, none_m, none_l = run_kl(z_p, logs_q, m_p, logs_p, ft, t_y, expand=False)  # the losses alone
    assert none_m is None and none_l is None and torch.equal(kl_n, kl) and torch.equal(rows_n, rows)


@functools.lru_cache(maxsize=None)
def kl_model_dims():
    case = kl_case(4, 192, 150, 40, 9, t_y=[150, 149, 64, 40])
    return case, check_kl(case, "C=192 4x150x40")


def test_kl_model_dims():
    kl_model_dims()


def test_kl_batch_independence_and_repeatability():
    """Every utterance of the padded batch is bit for bit what it gets alone at T_y = its own length; a second call gives the same bits."""
    (z_p, logs_q, m_p, logs_p, ft, t_y), got = kl_model_dims()
    again = run_kl(z_p, logs_q, m_p, logs_p, ft, t_y)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two identical calls differ"
    for b, n in enumerate(t_y.tolist()):
        tx = int(ft[b, :n].max()) + 1
        kl, rows, m_exp, _ = run_kl(z_p[b:b + 1, :, :n], logs_q[b:b + 1, :, :n], m_p[b:b + 1, :, :tx], logs_p[b:b + 1, :, :tx], ft[b:b + 1, :n],
                                    t_y[b:b + 1])
        assert torch.equal(rows[0], got[1][b]) and torch.equal(kl[0], got[1][b]), b
        assert torch.equal(m_exp[0], got[2][b, :n]), b


def test_kl_workspace_fits_the_reported_bytes(monkeypatch):
    from hip_helpers import assert_workspace_fits
    from torch_tts_amd.engine import Handle

    case = kl_case(3, 16, 37, 5, 10)

    def run():
        return torch.cat([t.reshape(-1) for t in run_kl(*case)]).cuda()

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)


def test_kl_loss_drop_in():
    V = _V()
    z_p, logs_q, m_p, logs_p, ft, t_y = kl_case(3, 16, 33, 33, 11)
    mask = mask_of(t_y, 33)
    with torch.no_grad():
        got = V.kl_loss(z_p.cuda(), logs_q.cuda(), m_p.cuda(), logs_p.cuda(), mask.cuda())
    want = kl_restated(z_p, logs_q, m_p, logs_p, t_y)[2]
    print("kl_loss", rel(got.cpu(), want))
    assert got.dim() == 0 and got.is_cuda and rel(got.cpu(), want) <= REL
    holes = mask.clone()
    holes[0, 0, 3] = 0.0
    with torch.no_grad(), pytest.raises(ValueError):
        V.kl_loss(z_p.cuda(), logs_q.cuda(), m_p.cuda(), logs_p.cuda(), holes.cuda())
    with torch.no_grad(), pytest.raises(NotImplementedError):
        V.kl_loss(z_p.cuda().double(), logs_q.cuda(), m_p.cuda(), logs_p.cuda(), mask.cuda())
    with pytest.raises(NotImplementedError):
        V.kl_loss(z_p.cuda().requires_grad_(), logs_q.cuda(), m_p.cuda(), logs_p.cuda(), mask.cuda())


# ---------------------------------------------------------------------------------------------------------------------------
# slices
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [1, 5, 16, 37])
@pytest.mark.parametrize("ids_dtype", [torch.int64, torch.int32])
def test_slice_segments_is_the_reference_loop(seg, ids_dtype):
    """The reference's layout [B, C, T] (inner = 1: every start is an arbitrary element offset): starts 0, T - seg and odd ones."""
    V, T = _V(), 37
    x = torch.randn(4, 5, T, generator=torch.Generator().manual_seed(seg))
    ids = torch.tensor([0, T - seg, min(3, T - seg), min(7, T - seg)], dtype=ids_dtype)
    with torch.no_grad():
        got = V.slice_segments(x.cuda(), ids.cuda(), seg)
    assert torch.equal(got.cpu(), slice_restated(x, ids, seg))
    with torch.no_grad():  # ids from the host, as the reference also takes them
        assert torch.equal(V.slice_segments(x.cuda(), ids.tolist(), seg).cpu(), got.cpu())


@pytest.mark.parametrize("inner,scale,offset", [(16, 1, 0), (6, 1, 0), (16, 1, 1), (1, 8, 0), (1, 8, 3)])
def test_slice_views(inner, scale, offset):
    """Channel-last z (inner a multiple of 4: 16-byte elements), an inner that is not, a base that is only 4-byte aligned (offset
    floats into a buffer), and the waveform view with scale = 8 (the hop)."""
    B, outer, T, seg = 3, 2, 50, 16
    gen = torch.Generator().manual_seed(inner + scale + offset)
    buf = torch.randn(B * outer * T * inner + offset, generator=gen).cuda()
    x = buf[offset:].view(B, outer, T, inner)
    ids = torch.tensor([0, (T - seg) // scale, 1])
    out, status = engine().slice_segments(x, ids.cuda(), outer, T, inner, seg, scale)
    want = torch.stack([x[b, :, int(ids[b]) * scale:int(ids[b]) * scale + seg] for b in range(B)])
    assert int(status.item()) == 0 and torch.equal(out.view(B, outer, seg, inner), want)


def test_slice_out_of_range_start():
    V = _V()
    x = torch.randn(3, 4, 20, generator=torch.Generator().manual_seed(1)).cuda()
    for ids in ([0, 13, 2], [0, -1, 2]):  # beyond T - seg = 12; below 0
        out, status = engine().slice_segments(x.contiguous(), torch.tensor(ids).cuda(), 4, 20, 1, 8)
        out = out.view(3, 4, 8)
        assert int(status.item()) == 1 and float(out[1].abs().sum()) == 0.0
        assert torch.equal(out[0], x[0, :, :8]) and torch.equal(out[2], x[2, :, 2:10])
        with torch.no_grad(), pytest.raises(ValueError):
            V.slice_segments(x, torch.tensor(ids), 8)
    out, status = engine().slice_segments(x.contiguous(), torch.tensor([0, 2, 3]).cuda(), 4, 20, 1, 8, 8)  # 2 * 8, 3 * 8 > 12
    assert int(status.item()) == 1 and float(out.view(3, 4, 8)[1:].abs().sum()) == 0.0


@pytest.mark.parametrize("name", MODELS)
def test_rand_slice_segments_golden_draw(name):
    V = _V()
    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    seg = meta["net"]["segment_size"]
    with torch.no_grad():
        z_slice, ids = V.rand_slice_segments(k("z").cuda(), k("y_lengths").cuda(), seg, u=k("u"))
    assert torch.equal(ids.cpu(), k("ids_slice")) and torch.equal(z_slice.cpu(), slice_restated(k("z"), k("ids_slice"), seg))
    torch.manual_seed(3)
    with torch.no_grad():
        drawn, ids2 = V.rand_slice_segments(k("z").cuda(), None, seg)
    torch.manual_seed(3)
    assert torch.equal(ids2.cpu(), (torch.rand([4]) * (40 - seg + 1)).long()) and torch.equal(drawn.cpu(), slice_restated(k("z"), ids2.cpu(), seg))


def test_a_too_short_utterance_is_refused():
    """Below segment - 1 frames the reference's draw can be negative: u = 0.9 over x_lengths - segment + 1 = -2 is -1."""
    V = _V()
    x = torch.randn(2, 4, 40).cuda()
    with torch.no_grad(), pytest.raises(ValueError):
        V.rand_slice_segments(x, torch.tensor([40, 13]).cuda(), 16, u=torch.tensor([0.5, 0.9]))


# ---------------------------------------------------------------------------------------------------------------------------
# sliced L1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [1, 16, 33])
@pytest.mark.parametrize("C", [16, 80])
@pytest.mark.parametrize("with_ids", [True, False])
def test_sliced_l1(seg, C, with_ids):
    B, T_a = 3, seg + 9 if with_ids else seg
    gen = torch.Generator().manual_seed(100 * seg + C)
    a, y = torch.randn(B, C, T_a, generator=gen), torch.randn(B, C, seg, generator=gen)
    ids = torch.tensor([0, 9, 4]) if with_ids else None
    l1, rows, status = engine().sliced_l1(a.cuda(), y.cuda(), None if ids is None else ids.cuda())
    again = engine().sliced_l1(a.cuda(), y.cuda(), None if ids is None else ids.cuda())
    want_rows, want = sliced_l1_restated(a, y, ids)
    errs = {"mean": rel(l1[1].cpu(), want), "sum": rel(l1[0].cpu(), want_rows.sum()), "rows": rel(rows.cpu(), want_rows)}
    print(f"seg={seg} C={C} ids={with_ids}", errs)
    assert int(status.item()) == 0 and max(errs.values()) <= REL, errs
    assert torch.equal(again[0], l1) and torch.equal(again[1], rows)
    alone = engine().sliced_l1(a[1:2].cuda(), y[1:2].cuda(), None if ids is None else ids[1:2].cuda())
    assert torch.equal(alone[1][0], rows[1])


def test_sliced_l1_out_of_range_start():
    a, y = torch.randn(2, 4, 20).cuda(), torch.randn(2, 4, 8).cuda()
    l1, rows, status = engine().sliced_l1(a, y, torch.tensor([13, 0]).cuda())
    assert int(status.item()) == 1
    assert rel(rows[0].cpu(), y[0].abs().double().sum().cpu()) <= REL  # counted as a slice of zeros


# ---------------------------------------------------------------------------------------------------------------------------
# the whole forward and the loss terms on the golden models
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_run(name):
    """The fixture's model on the device and one synthesizer_forward / validation_losses call with every draw supplied - computed
    once, shared by the tests below and left unchanged."""
    V = _V()
    sd, meta = load_golden()
    c = meta["models"][name]
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    net = eval_net(meta, name).cuda()
    net_d = make_mpd(41).cuda()
    sid = k("sid").cuda() if c["n_speakers"] else None
    noise = (k("e_post").cuda(), k("e_q"), k("e_w")) if c["use_sdp"] else (k("e_post").cuda(), None, None)
    args = (k("x").cuda(), k("x_lengths").cuda(), k("spec").cuda(), k("y_lengths").cuda())
    audio = dict(meta["audio"], mel_basis=sd["basis"].cuda())
    with torch.no_grad():
        fwd = V.synthesizer_forward(net, *args, sid, noise=noise, ids_slice=k("ids_slice"))
        losses = V.validation_losses(net, net_d, *args, k("wav").cuda(), **audio, c_mel=1.0, c_kl=1.0, sid=sid, noise=noise, ids_slice=k("ids_slice"))
    return net, net_d, args, sid, noise, audio, fwd, losses


@pytest.mark.parametrize("name", MODELS)
def test_synthesizer_forward_golden(name):
    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    o, l_length, attn, ids_slice, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q), (hidden_x, logw, logw_) = golden_run(name)[6]
    assert torch.equal(attn.cpu(), k("attn").float()) and torch.equal(ids_slice.cpu(), k("ids_slice")) and ids_slice.dtype == torch.int64
    assert torch.equal(x_mask.cpu(), k("x_mask")) and torch.equal(y_mask.cpu(), k("y_mask"))
    got = dict(z=z, z_p=z_p, m_p=m_p, logs_p=logs_p, m_q=m_q, logs_q=logs_q, o=o, logw_=logw_)
    for n, t in got.items():
        print(name, n, tuple(t.shape), "max abs err", float((t.cpu() - k(n)).abs().max()))
    for n, t in got.items():
        assert t.shape == k(n).shape, n
        torch.testing.assert_close(t.cpu(), k(n), rtol=RTOL, atol=ATOL, msg=lambda m, n=n: f"{name} {n}: {m}")
    torch.testing.assert_close(hidden_x.cpu(), k("hidden_x"), rtol=RTOL, atol=10 * ATOL)
    print(name, "l_length", rel(l_length.cpu(), k("l_length")), "logw", rel(logw.cpu(), k("logw")))
    assert rel(l_length.cpu(), k("l_length")) <= REL and rel(logw.cpu(), k("logw")) <= REL
    # the expanded prior is the text encoder's rows, gathered: exact zeros at padded frames
    ft = frame_token_of(k("attn"), k("y_lengths"))
    assert float(m_p.cpu()[(ft < 0)[:, None, :].expand_as(m_p)].abs().sum()) == 0.0


@pytest.mark.parametrize("name", MODELS)
def test_validation_losses_golden(name):
    V = _V()
    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    net, net_d, args, sid, noise, audio, fwd, losses = golden_run(name)
    for n in ("loss_mel", "loss_kl", "loss_dur"):
        print(name, n, float(losses[n]), float(k(n)), "rel", rel(losses[n].cpu(), k(n)), "rel to fp64", rel(losses[n].cpu(), k(n + "64")))
    for n in ("loss_mel", "loss_kl", "loss_dur"):
        assert losses[n].dim() == 0 and losses[n].is_cuda
        assert rel(losses[n].cpu(), k(n)) <= REL, n
    assert torch.equal(losses["ids_slice"].cpu(), k("ids_slice"))
    # the discriminator terms are the drop-ins' own (tests/test_disc_hip.py), composed as train.py:376-422 composes them
    o = fwd[0]
    y = slice_restated(k("wav"), k("ids_slice") * audio["hop_size"], audio["segment_size"]).cuda()
    with torch.no_grad():
        y_d_hat_r, y_d_hat_g, fmap_r, fmap_g = net_d(y, o)
        dr, dg = V.discriminator_loss(y_d_hat_r, y_d_hat_g)
        want = {"loss_disc": dr.sum() + dg.sum(), "loss_gen": V.generator_loss(y_d_hat_g).sum(), "loss_fm": V.feature_loss(fmap_r, fmap_g)}
    for n, v in want.items():
        assert torch.equal(losses[n], v), n
    total = losses["loss_gen"] + losses["loss_fm"] + losses["loss_mel"] + losses["loss_dur"] + losses["loss_kl"]
    assert torch.equal(losses["loss_gen_all"], total) and set(losses) == set(want) | {"loss_mel", "loss_kl", "loss_dur", "loss_gen_all", "ids_slice"}
    # the coefficients, and the draw of the segment when none is given
    real = torch.rand
    try:
        torch.rand = lambda *a, **kw: k("u").clone()
        with torch.no_grad():
            scaled = V.validation_losses(net, net_d, *args, k("wav").cuda(), **audio, sid=sid, noise=noise)
    finally:
        torch.rand = real
    assert torch.equal(scaled["ids_slice"].cpu(), k("ids_slice"))
    assert torch.equal(scaled["loss_mel"], losses["loss_mel"] * 10.0) and torch.equal(scaled["loss_kl"], losses["loss_kl"] * 0.2)


def test_validation_losses_with_a_duration_discriminator():
    import torch_tts_amd as T

    V = _V()
    net, net_d, args, sid, noise, audio, fwd, losses = golden_run("model_lin")
    sd, _ = load_golden()
    dd = T.DurationDiscriminatorV2(32, 32, 3, 0.1, gin_channels=0).cuda().eval()
    with torch.no_grad():
        got = V.validation_losses(net, net_d, *args, sd["model_lin/wav"].cuda(), **audio, c_mel=1.0, c_kl=1.0, sid=sid, noise=noise,
                                  ids_slice=sd["model_lin/ids_slice"], net_dur_disc=dd)
        y_dur_hat_r, y_dur_hat_g = dd(fwd[7][0], fwd[4], fwd[7][2], fwd[7][1])
        dr, dg = V.discriminator_loss(y_dur_hat_r, y_dur_hat_g)
    assert torch.equal(got["loss_dur_disc"], dr.sum() + dg.sum()) and torch.equal(got["loss_dur_gen"], V.generator_loss(y_dur_hat_g).sum())
    assert torch.equal(got["loss_gen_all"], losses["loss_gen_all"] + got["loss_dur_gen"])
    for n in ("loss_mel", "loss_kl", "loss_dur", "loss_disc"):
        assert torch.equal(got[n], losses[n]), n


@pytest.mark.parametrize("name", MODELS)
def test_validation_losses_from_audio(name):
    """The spectrogram made on the device from each utterance's own samples is the fixture's (made by the reference from each
    utterance alone): the same losses within the bar."""
    V = _V()
    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    net, net_d, args, sid, noise, audio, _, _ = golden_run(name)
    with torch.no_grad():
        got = V.validation_losses_from_audio(net, net_d, args[0], args[1], k("wav").cuda(), (k("y_lengths") * audio["hop_size"]).cuda(), **audio,
                                             c_mel=1.0, c_kl=1.0, sid=sid, noise=noise, ids_slice=k("ids_slice"))
    for n in ("loss_mel", "loss_kl", "loss_dur"):
        print(name, "from audio", n, rel(got[n].cpu(), k(n)))
        assert rel(got[n].cpu(), k(n)) <= REL, n


def test_refusals():
    V = _V()
    sd, meta = load_golden()
    k = lambda n: sd[f"model_lin/{n}"]  # noqa: E731
    net, net_d, args, sid, noise, audio, _, _ = golden_run("model_lin")
    dec = net.dec
    try:
        net.dec = torch.nn.Conv1d(16, 1, 1).cuda()
        with torch.no_grad(), pytest.raises(TypeError):
            V.synthesizer_forward(net, *args, sid, noise=noise, ids_slice=k("ids_slice"))
    finally:
        net.dec = dec
    with torch.no_grad(), pytest.raises(TypeError):
        V.validation_losses(net, torch.nn.Identity(), *args, k("wav").cuda(), **audio, sid=sid)
    with pytest.raises(NotImplementedError):  # gradients enabled, parameters that require them
        V.synthesizer_forward(net, *args, sid, noise=noise, ids_slice=k("ids_slice"))
    with torch.no_grad(), pytest.raises(ValueError):  # a segment that starts beyond T_y - segment
        V.synthesizer_forward(net, *args, sid, noise=noise, ids_slice=torch.tensor([0, 0, 25, 0]))
    with torch.no_grad(), pytest.raises(ValueError):  # segment_size in samples is not net_g.segment_size frames
        V.validation_losses(net, net_d, *args, k("wav").cuda(), **dict(audio, segment_size=64), sid=sid)
    with torch.no_grad(), pytest.raises(ValueError):
        V.synthesizer_forward(net, *args, sid, noise=noise[:2])
