"""GPU tests of monotonic alignment search on HIP (ttsvits_neg_cent / ttsvits_maximum_path / ttsvits_align; vits2.maximum_path, align,
forced_alignment).  The search given neg_cent is compared EXACTLY (path, frame_token, dur; no tolerance, no cell left out) with the
restatement of tests/test_align_host.py, which that file pins against the reference's compiled core.pyx.  neg_cent is compared with
an fp64 evaluation of models.py:1226-1239; its bar is 4 x the error of the reference's own fp32 torch-CPU evaluation on the same
inputs (tests/golden/align_meta.json, measured by make_golden_align.py).  End to end, the asserted criterion is derived, not
measured: with e = max |neg_cent_hip - neg_cent_f64| over the valid cells, the fp64 score of the HIP path is at least the fp64 optimum
minus 2 T_y e; equality with the golden path is counted and printed only (a near-tie may fall either way)."""
import numpy as np
import pytest
import torch

from test_align_host import (align_net, alone_cases, alone_costs, best_score, forced_alignment_host, load_golden, mas_batch, neg_cent_inputs,
                             neg_cent_torch, path_score, rel_err)

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5  # the stage tolerances of tests/test_vc_hip.py


def _V():
    import torch_tts_amd as T

    return T.vits2


def _mask(t_y, t_x, T_y, T_x):
    t_y, t_x = torch.as_tensor(t_y), torch.as_tensor(t_x)
    return ((torch.arange(T_y)[None, :, None] < t_y[:, None, None]) & (torch.arange(T_x)[None, None, :] < t_x[:, None, None])).float()


def _structure(ft, dur, path, t_y, t_x):
    B, T_y, T_x = path.shape
    for b in range(B):
        ty, tx = int(t_y[b]), int(t_x[b])
        f = ft[b, :ty]
        assert f[0] == 0 and f[-1] == tx - 1 and set(np.diff(f).tolist()) <= {0, 1}, b  # starts at token 0, ends at t_x - 1, steps 0 / 1
        assert (path[b, :ty].sum(1) == 1).all() and path[b, ty:].sum() == 0 and path[b, :, tx:].sum() == 0, b  # one token per frame
        assert (ft[b, ty:] == -1).all() and (dur[b, tx:] == 0).all() and dur[b].sum() == ty and (dur[b, :tx] >= 1).all(), b


def _check_search(nc, t_y, t_x, what):
    """path, frame_token and dur of the HIP search on nc [B, T_y, T_x] (numpy fp32): exactly the restatement's, through the
    engine call and through vits2.maximum_path(neg_cent, mask)."""
    V = _V()
    nc = np.ascontiguousarray(nc, np.float32)
    B, T_y, T_x = nc.shape
    ft0, dur0, path0 = mas_batch(nc, t_y, t_x)
    dev = torch.device("cuda", 0)
    ncd = torch.from_numpy(nc).to(dev)
    keep = ncd.clone()
    eng = V._align_engine(dev)
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)  # noqa: E731
    path, ft, dur = eng.maximum_path(ncd, i32(t_y), i32(t_x))
    path2 = V.maximum_path(ncd, _mask(t_y, t_x, T_y, T_x).to(dev))
    torch.cuda.synchronize()
    assert torch.equal(ncd, keep), what  # (the reference accumulates in its copy; the input is not touched)
    ft, dur, path = ft.cpu().numpy(), dur.cpu().numpy(), path.cpu().numpy()
    assert np.array_equal(ft, ft0), (what, int((ft != ft0).sum()))
    assert np.array_equal(dur, dur0), what
    assert np.array_equal(path, path0), what
    assert path2.dtype == torch.float32 and np.array_equal(path2.cpu().numpy(), path0), what
    _structure(ft, dur, path, t_y, t_x)
    return ft


def _ragged_lengths(rng, B, T_y, T_x):
    t_x = rng.integers(1, T_x + 1, B)
    t_x[0] = T_x
    t_y = np.array([rng.integers(tx, T_y + 1) for tx in t_x])
    t_y[0] = T_y
    if B > 2:
        t_y[1] = t_x[1]  # a square one: the diagonal rule at every row
        t_x[2] = 1
    return t_y.astype(np.int32), t_x.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the search given neg_cent
# ---------------------------------------------------------------------------------------------------------------------------
def test_search_equals_the_reference_on_every_golden_case():
    sd, meta = load_golden()
    for name, ty, tx in alone_cases():
        ft = _check_search(alone_costs(name, ty, tx)[None], [ty], [tx], name)
        assert np.array_equal(ft[0], sd[f"alone/{name}/frame_token"].astype(np.int32)), name
    for key in ("ragged", "model"):
        ft = _check_search(sd[f"{key}/neg_cent"], sd[f"{key}/t_y"], sd[f"{key}/t_x"], key)
        assert np.array_equal(ft, sd[f"{key}/frame_token"].astype(np.int32)), key
    # the stand-alone cases again, padded into one batch (another T_x, so other column runs per lane)
    cases = alone_cases()
    T_y, T_x = max(c[1] for c in cases), max(c[2] for c in cases)
    nc = np.random.default_rng(1).standard_normal((len(cases), T_y, T_x)).astype(np.float32)  # (padding cells: never read)
    for i, (name, ty, tx) in enumerate(cases):
        nc[i, :ty, :tx] = alone_costs(name, ty, tx)
    ft = _check_search(nc, [c[1] for c in cases], [c[2] for c in cases], "alone, batched")
    for i, (name, ty, tx) in enumerate(cases):
        assert np.array_equal(ft[i, :ty], sd[f"alone/{name}/frame_token"].astype(np.int32)), name


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("T_x", [1, 63, 64, 65, 128, 129, 150, 256, 257, 512, 513, 1023, 1024])
def test_search_random_ragged_batches(B, T_x):
    """T_x across the lane (64) and column-run (64 x 1, 2, 4, 8, 16) boundaries up to the supported maximum."""
    rng = np.random.default_rng(100 * B + T_x)
    T_y = int(T_x + rng.integers(0, 200)) if B == 64 else int(min(2000, max(T_x, 3 * T_x // 2 + rng.integers(0, 300))))
    t_y, t_x = _ragged_lengths(rng, B, T_y, T_x)
    _check_search(rng.standard_normal((B, T_y, T_x)).astype(np.float32) * 4, t_y, t_x, f"B={B} T_y={T_y} T_x={T_x}")


@pytest.mark.parametrize("T_y,T_x", [(2000, 150), (2000, 1024), (1999, 513), (257, 256), (129, 2)])
def test_search_long_utterances_and_tie_heavy_integer_costs(T_y, T_x):
    rng = np.random.default_rng(T_y + T_x)
    t_y, t_x = _ragged_lengths(rng, 3, T_y, T_x)
    _check_search(rng.standard_normal((3, T_y, T_x)).astype(np.float32), t_y, t_x, f"float {T_y}x{T_x}")
    _check_search(rng.integers(-2, 3, (3, T_y, T_x)).astype(np.float32), t_y, t_x, f"integer {T_y}x{T_x}")
    _check_search(np.zeros((3, T_y, T_x), np.float32), t_y, t_x, f"all ties {T_y}x{T_x}")


def test_search_benchmark_shape():
    rng = np.random.default_rng(7)
    B, T_y, T_x = 64, 600, 150
    nc = rng.standard_normal((B, T_y, T_x)).astype(np.float32) * 30 - 200
    _check_search(nc, np.full(B, T_y), np.full(B, T_x), "64 x 600 x 150")
    t_y, t_x = _ragged_lengths(rng, B, T_y, T_x)
    _check_search(nc, t_y, t_x, "64 x 600 x 150 ragged")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_path_comes_back_in_the_callers_dtype(dtype):
    V = _V()
    rng = np.random.default_rng(5)
    nc = rng.integers(-3, 4, (3, 50, 20)).astype(np.float32)  # (integers: exact in every dtype)
    t_y, t_x = [50, 20, 33], [20, 20, 7]
    _, _, path0 = mas_batch(nc, t_y, t_x)
    out = V.maximum_path(torch.from_numpy(nc).cuda().to(dtype), _mask(t_y, t_x, 50, 20).cuda().to(dtype))
    assert out.dtype == dtype and out.is_cuda and np.array_equal(out.float().cpu().numpy(), path0)


def test_refusals():
    from torch_tts_amd import _lib

    V = _V()
    nc = torch.randn(2, 12, 8, device="cuda")
    keep = nc.clone()
    with pytest.raises(ValueError, match="fewer frames than tokens"):
        V.maximum_path(nc, _mask([12, 5], [8, 6], 12, 8).cuda())
    with pytest.raises(ValueError, match="no frames or no tokens"):
        V.maximum_path(nc, _mask([12, 5], [8, 0], 12, 8).cuda())
    eng = V._align_engine(nc.device)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="exceeds the tensor"):
        eng.maximum_path(nc, i32([13, 5]), i32([8, 2]))
    # a refused call writes its outputs only: guard bands around the raw call's buffers stay as they were
    B, T_y, T_x = 2, 12, 8
    big = torch.full((4096,), -7, dtype=torch.int32, device="cuda")
    ft, dur, status = big[1024:1024 + B * T_y], big[2048:2048 + B * T_x], big[3072:3073]
    path = torch.full((3, B * T_y * T_x), 5.0, device="cuda")
    ws = torch.zeros(int(eng._lib.ttsvits_align_workspace_bytes(eng._h, B, T_y, T_x)), dtype=torch.uint8, device="cuda")
    t_y, t_x = i32([12, 5]), i32([8, 6])
    rc = eng._lib.ttsvits_maximum_path(eng._h, nc.data_ptr(), t_y.data_ptr(), t_x.data_ptr(), B, T_y, T_x, path[1].data_ptr(),
                                      _lib.PATH_F32, ft.data_ptr(), dur.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.OK and int(status) == 2
    inside = torch.zeros(4096, dtype=torch.bool, device="cuda")
    inside[1024:1024 + B * T_y] = inside[2048:2048 + B * T_x] = inside[3072:3073] = True
    assert bool((big[~inside] == -7).all()) and bool((path[0] == 5).all()) and bool((path[2] == 5).all())
    assert bool((ft.view(B, T_y)[1] == -1).all()) and bool((dur.view(B, T_x)[1] == 0).all()) and bool((path[1].view(B, T_y, T_x)[1] == 0).all())
    assert torch.equal(nc, keep)
    with pytest.raises(_lib.DimsNotBuilt):
        V.maximum_path(torch.zeros(1, 1100, 1025, device="cuda"), torch.ones(1, 1100, 1025, device="cuda"))
    with pytest.raises(NotImplementedError):
        V.maximum_path(nc.cpu(), _mask([12, 12], [8, 8], 12, 8))
    # and the engine still serves the next call
    _check_search(nc.cpu().numpy(), [12, 9], [8, 8], "after refusals")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. neg_cent
# ---------------------------------------------------------------------------------------------------------------------------
def _neg_cent_hip(z_p, m_p, logs_p, t_y=None, t_x=None):
    V = _V()
    dev = torch.device("cuda", 0)
    cl = lambda t: t.transpose(1, 2).contiguous().to(dev)  # noqa: E731
    i32 = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)  # noqa: E731
    return V._align_engine(dev).neg_cent(cl(z_p), cl(m_p), cl(logs_p), i32(t_y), i32(t_x)).cpu()


def test_neg_cent_within_four_times_the_reference_fp32_error():
    """Bar: 4 x (max abs error / max |value|) of the reference's fp32 torch-CPU evaluation against fp64, recorded in align_meta.json
    on these same inputs.  The contraction order over 2C products and the re-associated four-term sum cannot be made identical."""
    sd, meta = load_golden()
    bar = meta["neg_cent_cpu_f32_err"]
    t = lambda k: torch.from_numpy(sd[k])  # noqa: E731
    cases = {"golden": (t("model/z_p"), t("model/m_p"), t("model/logs_p")), "c192_600x150": neg_cent_inputs(11, 2, 192, 600, 150)}
    errs = {}
    for name, (z_p, m_p, logs_p) in cases.items():
        ref = neg_cent_torch(z_p.double(), m_p.double(), logs_p.double())
        errs[name] = rel_err(_neg_cent_hip(z_p, m_p, logs_p), ref)
        print(f"neg_cent {name}: HIP {errs[name]:.3e}, reference fp32 CPU {bar[name]:.3e}, bar {4 * bar[name]:.3e}, max |value| {float(ref.abs().max()):.4e}")
    for name in cases:
        assert errs[name] <= 4 * bar[name], (name, errs[name], 4 * bar[name])


def test_neg_cent_ragged_cells_outside_an_utterance_are_zero():
    z_p, m_p, logs_p = neg_cent_inputs(3, 5, 24, 70, 45)
    t_y, t_x = [70, 33, 1, 64, 65], [45, 32, 1, 33, 7]
    out = _neg_cent_hip(z_p, m_p, logs_p, t_y, t_x)
    full = _neg_cent_hip(z_p, m_p, logs_p)
    ref = neg_cent_torch(z_p.double(), m_p.double(), logs_p.double())
    assert rel_err(full, ref) < 1e-5
    m = _mask(t_y, t_x, 70, 45).bool()
    assert torch.equal(out[m], full[m]) and bool((out[~m] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------------------
def _score_bound(path, nc_hip, nc64, t_y, t_x, what):
    """The derived criterion (module docstring); prints the scores.  path [B, T_y, T_x] 0 / 1, nc_hip / nc64 [B, T_y, T_x]."""
    path, nc_hip, nc64 = path.cpu().numpy(), nc_hip.double().cpu().numpy(), nc64.cpu().numpy()
    for b in range(path.shape[0]):
        ty, tx = int(t_y[b]), int(t_x[b])
        e = float(np.abs(nc_hip[b, :ty, :tx] - nc64[b, :ty, :tx]).max())
        ft = path[b, :ty].argmax(1)
        got, best = path_score(nc64[b], ft), best_score(nc64[b], ty, tx)
        print(f"{what} b={b}: fp64 score of the HIP path {got:.6f}, fp64 optimum {best:.6f}, e {e:.3e}, slack allowed {2 * ty * e:.3e}")
        assert got >= best - 2 * ty * e and got <= best + 1e-9 * abs(best), (what, b, got, best, e)


def _count_equal(path, ft_ref, t_y, what):
    ft = path.cpu().numpy().argmax(2)
    same = sum(int((ft[b, :t] == ft_ref[b, :t]).sum()) for b, t in enumerate(t_y))
    print(f"{what}: {same} of {int(np.sum(t_y))} frames on the reference's token")


def test_align_golden_and_random():
    V = _V()
    sd, meta = load_golden()
    t = lambda k: torch.from_numpy(sd[k])  # noqa: E731
    t_y, t_x = sd["model/t_y"], sd["model/t_x"]
    z_p, m_p, logs_p = t("model/z_p"), t("model/m_p"), t("model/logs_p")
    T_y, T_x = z_p.shape[2], m_p.shape[2]
    x_mask = (torch.arange(T_x)[None, :] < torch.from_numpy(t_x)[:, None]).float().unsqueeze(1)
    y_mask = (torch.arange(T_y)[None, :] < torch.from_numpy(t_y)[:, None]).float().unsqueeze(1)
    attn = V.align(z_p.cuda(), m_p.cuda(), logs_p.cuda(), x_mask.cuda(), y_mask.cuda())
    assert attn.shape == (len(t_y), 1, T_y, T_x)
    _count_equal(attn[:, 0], sd["model/frame_token"], t_y, "align, golden")
    nc64 = neg_cent_torch(z_p.double(), m_p.double(), logs_p.double())
    nc_hip = _neg_cent_hip(z_p, m_p, logs_p)
    _score_bound(attn[:, 0], nc_hip, nc64, t_y, t_x, "align, golden")
    assert torch.equal(attn.sum(2).cpu(), attn.sum(2).cpu().round())
    # mas_noise_scale: the torch-op term between the two kernels; a zero scale leaves the path as it is
    attn0 = V.align(z_p.cuda(), m_p.cuda(), logs_p.cuda(), x_mask.cuda(), y_mask.cuda(), 0.0, noise=torch.randn(len(t_y), T_y, T_x))
    assert torch.equal(attn0, attn)
    attn1 = V.align(z_p.cuda(), m_p.cuda(), logs_p.cuda(), x_mask.cuda(), y_mask.cuda(), 0.01)
    _structure(*_ft_dur(attn1[:, 0]), attn1[:, 0].cpu().numpy(), t_y, t_x)
    # ModelConfig width, the benchmark's lengths, ragged
    z_p, m_p, logs_p = neg_cent_inputs(5, 3, 192, 600, 150)
    t_y, t_x = np.array([600, 431, 150]), np.array([150, 97, 150])
    x_mask = (torch.arange(150)[None, :] < torch.from_numpy(t_x)[:, None]).float().unsqueeze(1)
    y_mask = (torch.arange(600)[None, :] < torch.from_numpy(t_y)[:, None]).float().unsqueeze(1)
    attn = V.align(z_p.cuda(), m_p.cuda(), logs_p.cuda(), x_mask.cuda(), y_mask.cuda())
    nc64 = neg_cent_torch(z_p.double(), m_p.double(), logs_p.double())
    ft_ref, _, _ = mas_batch(neg_cent_torch(z_p, m_p, logs_p).numpy(), t_y, t_x)
    _count_equal(attn[:, 0], ft_ref, t_y, "align, C = 192, 600 x 150 (against the search on the fp32 CPU neg_cent)")
    _score_bound(attn[:, 0], _neg_cent_hip(z_p, m_p, logs_p), nc64, t_y, t_x, "align, C = 192")
    _structure(*_ft_dur(attn[:, 0]), attn[:, 0].cpu().numpy(), t_y, t_x)


def _ft_dur(path):
    p = path.cpu().numpy()
    ft = p.argmax(2).astype(np.int32)
    ft[p.sum(2) == 0] = -1
    return ft, p.sum(1).astype(np.int32)


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{what}: max abs err {err.max().item():.3e} (ref max {b.abs().max().item():.3e}), {int(bad.sum())} elements out"


def test_forced_alignment_golden_and_host_restatement():
    V = _V()
    sd, meta = load_golden()
    t = lambda k: torch.from_numpy(sd[k])  # noqa: E731
    net = align_net(meta).cuda()
    x, xl, y, yl, sid, noise = (t(f"model/{k}") for k in ("x", "x_lengths", "y", "y_lengths", "sid", "noise"))
    with torch.no_grad():
        attn, w, logw_, (z, z_p, m_p, logs_p) = V.forced_alignment(net, x.cuda(), xl.cuda(), y.cuda(), yl.cuda(), sid=sid.cuda(), noise=noise.cuda())
        ref = forced_alignment_host(net, x, xl, y, yl, sid, noise)
    B, T_y, T_x = len(xl), y.shape[2], x.shape[1]
    assert attn.shape == (B, 1, T_y, T_x) and w.shape == (B, 1, T_x) and logw_.shape == (B, 1, T_x)
    for name, a, r in zip(("z", "z_p", "m_p", "logs_p"), (z, z_p, m_p, logs_p), ref[:4]):
        _close(a, t(f"model/{name}"), f"forced_alignment {name} against the reference")
        _close(a, r, f"forced_alignment {name} against the host restatement")
    t_y, t_x = sd["model/t_y"], sd["model/t_x"]
    _count_equal(attn[:, 0], sd["model/frame_token"], t_y, "forced_alignment, golden")
    ft, dur = _ft_dur(attn[:, 0])
    _structure(ft, dur, attn[:, 0].cpu().numpy(), t_y, t_x)
    # w and logw_ follow from the path exactly
    assert torch.equal(w, attn.sum(2))
    x_mask = (torch.arange(T_x)[None, :] < xl[:, None]).float().unsqueeze(1).cuda()
    assert torch.equal(logw_, torch.log(w + 1e-6) * x_mask)
    # the derived criterion against the fp64 chain of the stage oracles; e carries the stages' own error here
    nc_hip = _neg_cent_hip(z_p.cpu(), m_p.cpu(), logs_p.cpu())
    _score_bound(attn[:, 0], nc_hip, ref[4], t_y, t_x, "forced_alignment, golden")
    # a second call gives the same bits
    with torch.no_grad():
        again = V.forced_alignment(net, x.cuda(), xl.cuda(), y.cuda(), yl.cuda(), sid=sid.cuda(), noise=noise.cuda())
    assert torch.equal(again[0], attn)
