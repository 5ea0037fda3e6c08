"""GPU parity of the generator's opt-in split-fp16 mode (ttsvits_generator_* through torch_tts_amd.Generator with precision =
"split_f16").  The yardsticks are the exact path's: the reference's own outputs at the golden small dims and the fp64 restatement of
tests/test_generator_host.py, under the same rtol 1e-4 / atol 1e-5 (tests/test_generator_split_host.py shows why no wider bar is
needed) - never the fp32 HIP path, except where a test is about the two being the same call or different calls."""
import pytest
import torch

from test_generator_host import load_golden, make_generator, reference_forward, scaled_weights, weights

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
FULL = dict(initial_channel=192, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
            upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    print(f"{what}: worst |err| / (atol + rtol |ref|) = {float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()):.3f}")
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _all_close(gen, sd, dims, x, g, what):
    """The waveform and every stage's activated output of one split-fp16 call against the fp64 restatement."""
    y_ref, acts = reference_forward(sd, dims, x.cpu(), None if g is None else g.cpu(), stages=True)
    with torch.no_grad():
        _close(gen(x, g), y_ref, what)
        for s, ref in enumerate(acts):
            _close(gen.stage_outputs(x, g, n_stages=s), ref, f"{what} stage {s}")


def _state(gen):
    return {k: v.detach().cpu() for k, v in gen.state_dict().items()}


@pytest.fixture(scope="module")
def full_gen():
    gen = make_generator(FULL)
    scaled_weights(gen, 5)
    gen = gen.cuda().eval()
    gen.precision = "split_f16"
    return gen, _state(gen)


@pytest.fixture(scope="module")
def small_gen():
    gsd, meta = load_golden()
    gen = make_generator(meta["dims"], 4)
    gen.load_state_dict(weights(gsd, 4), strict=True)
    gen = gen.cuda().eval()
    gen.precision = "split_f16"
    return gen, meta["dims"]


def test_golden_small_dims():
    gsd, meta = load_golden()
    for gin in (0, 4):
        gen = make_generator(meta["dims"], gin)
        gen.load_state_dict(weights(gsd, gin), strict=True)
        gen = gen.cuda().eval()
        gen.precision = "split_f16"
        for T in meta["T"]:
            x = gsd[f"x{gin}/T{T}"].cuda()
            g = gsd[f"g{gin}/T{T}"].cuda() if gin else None
            with torch.no_grad():
                _close(gen(x, g), gsd[f"y{gin}/T{T}"], f"gin={gin} T={T} against the reference's output")
            _all_close(gen, weights(gsd, gin), meta["dims"], x, g, f"gin={gin} T={T}")
        # remove_weight_norm: same module, plain weights, the fp32 blob repacked - and the planes with it
        x, g = gsd[f"x{gin}/T9"].cuda(), gsd[f"g{gin}/T9"].cuda() if gin else None
        gen.remove_weight_norm()
        with torch.no_grad():
            y0 = gen(x, g)
        _close(y0, gsd[f"y{gin}/T9"], f"gin={gin} after remove_weight_norm")
        # (same effective weights as before, so stale planes would pass above: change one weight and the output must follow)
        with torch.no_grad():
            gen.resblocks[1].convs2[0].weight.data[:, :, 3] *= -1.0
        gen.invalidate()
        with torch.no_grad():
            y1 = gen(x, g)
        assert not torch.equal(y0, y1), "the planes were not rebuilt after the fp32 blob was repacked"
        _all_close(gen, _state(gen), meta["dims"], x, g, f"gin={gin} after a weight edit")


@pytest.mark.parametrize("T", [1, 3, 37])
def test_fulldims_b2(full_gen, T):
    """ModelConfig dims: C = 256 / 128 / 64 walk the taps with jumps (64 | C), C = 32 has two whole taps per 64-k tile and one per 32-k
    tile; T = 1 and 3 put every dilated tap of the early stages outside the utterance; at T = 37 stage 1 (N = 128, M = 4736) is on
    the 128 x 128 tile, stages 0 and 2 on the 64 x 64 tile, stage 3 on the 128 x 32 tile."""
    gen, sd = full_gen
    z = torch.randn(2, 192, T, generator=torch.Generator().manual_seed(20 + T))
    _all_close(gen, sd, FULL, z.cuda(), None, f"T={T}")


def test_fulldims_big_tile_at_256_channels_and_noncontiguous_input(full_gen):
    gen, sd = full_gen
    rng = torch.Generator().manual_seed(7)
    # B = 8 x T = 37: stage 0 has M = 2368 rows, so N = 256 takes the 128 x 128 tile too (four 64-k tiles per tap)
    z = torch.randn(8, 192, 37, generator=rng)
    with torch.no_grad():
        y = gen(z.cuda()).cpu()
        a0 = gen.stage_outputs(z.cuda(), n_stages=1).cpu()
    for b in (0, 7):
        y_ref, acts = reference_forward(sd, FULL, z[b : b + 1], stages=True)
        _close(y[b : b + 1], y_ref, f"B=8 b={b}")
        _close(a0[b : b + 1], acts[1], f"B=8 b={b} stage 1")
    # SynthesizerTrn.infer passes (z * y_mask)[:, :, :max_len]: a non-contiguous slice
    zz = torch.randn(2, 192, 50, generator=rng)
    with torch.no_grad():
        _close(gen(zz.cuda()[:, :, :41]), reference_forward(sd, FULL, zz[:, :, :41]), "sliced input")


def test_f32_is_the_exact_path_and_split_is_not(small_gen):
    """precision "f32" through ttsvits_generator_forward is ttsgen_forward on the same blob, bit for bit; split-fp16 is another
    arithmetic (had the mode fallen back silently, the two would agree in every sample)."""
    from torch_tts_amd import _lib
    from torch_tts_amd.engine import _stream

    gen, dims = small_gen
    rng = torch.Generator().manual_seed(11)
    x, g = torch.randn(3, dims["initial_channel"], 37, generator=rng).cuda(), torch.randn(3, 4, 1, generator=rng).cuda()
    with torch.no_grad():
        y_split = gen(x, g)
        gen.precision = "f32"
        try:
            y_f32 = gen(x, g)
        finally:
            gen.precision = "split_f16"
    eng = gen._engines.get(gen._cfg, x.device)
    z_cl, g2 = x.transpose(1, 2).contiguous(), g[:, :, 0].contiguous()
    nbytes = int(eng._lib.ttsgen_workspace_bytes(eng._h, 3, 37))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(3, 37 * 8, device=x.device)
    rc = eng._lib.ttsgen_forward(eng._h, z_cl.data_ptr(), g2.data_ptr(), 3, 37, out.data_ptr(), ws.data_ptr(), nbytes, _stream(x.device))
    assert rc == _lib.OK
    assert torch.equal(y_f32[:, 0], out)
    assert not torch.equal(y_split, y_f32)


def test_mixed_handle_falls_back_per_layer():
    """upsample_initial_channel = 24, one stage of 12 channels: conv_pre (16 input channels) and ups[0] (24) run in split-fp16, the
    resblocks (12: not a multiple of 8) keep the exact tiles inside the same call."""
    dims = dict(initial_channel=16, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 1, 1]] * 3,
                upsample_rates=[2], upsample_initial_channel=24, upsample_kernel_sizes=[4])
    gen = make_generator(dims)
    scaled_weights(gen, 9)
    gen = gen.cuda().eval()
    gen.precision = "split_f16"
    x = torch.randn(3, 16, 37, generator=torch.Generator().manual_seed(12)).cuda()
    _all_close(gen, _state(gen), dims, x, None, "mixed")
    # the other order - an exact layer whose result a split layer reads: conv_pre at 12 input channels in front of ups[0]
    dims2 = dict(dims, initial_channel=12)
    gen2 = make_generator(dims2)
    scaled_weights(gen2, 10)
    gen2 = gen2.cuda().eval()
    gen2.precision = "split_f16"
    x2 = torch.randn(3, 12, 37, generator=torch.Generator().manual_seed(13)).cuda()
    _all_close(gen2, _state(gen2), dims2, x2, None, "mixed, exact conv_pre in front of a split ups[0]")
    with torch.no_grad():
        y_split = gen2(x2)
        gen2.precision = "f32"
        assert not torch.equal(gen2(x2), y_split)


def test_groups_workspace_and_neighbours(small_gen, monkeypatch):
    from hip_helpers import assert_workspace_fits
    from torch_tts_amd.engine import Handle

    gen, dims = small_gen
    rng = torch.Generator().manual_seed(4)
    x, g = torch.randn(3, dims["initial_channel"], 37, generator=rng).cuda(), torch.randn(3, 4, 1, generator=rng).cuda()

    def run():
        with torch.no_grad():
            return gen(x, g)

    y = run()
    assert torch.equal(y, run()), "two identical calls differ"
    with monkeypatch.context() as mp:
        # groups of two: a full group, then a short last one whose buffers lie closer together than the reported size's
        mp.setenv("TTSGEN_GROUP_FORCE", "2")
        assert torch.equal(run(), y), "result depends on the group size"
        assert_workspace_fits(mp, Handle, "workspace", lambda eng, name, nbytes: nbytes, run)
    z = torch.randn(5, dims["initial_channel"], 37, generator=rng).cuda()
    g5 = torch.randn(5, 4, 1, generator=rng).cuda()
    with torch.no_grad():
        y0 = gen(z, g5)
        z2 = z.clone()
        z2[1], z2[3] = torch.randn_like(z2[1]), torch.randn_like(z2[3])
        y1 = gen(z2, g5)
    assert torch.equal(y0[2], y1[2]) and not torch.equal(y0[1], y1[1])


def test_infer_end_to_end_with_a_split_generator():
    """vits2.infer picks the mode up through net.dec: the waveform stays within the bar of the exact path's (which the existing tests
    hold to the reference), and nothing in front of the generator moves by a bit."""
    import torch_tts_amd as T
    from test_duration_host import infer_net
    from test_duration_host import load_golden as load_duration_golden

    sd, meta = load_duration_golden()
    name = "infer_sdp"
    c = meta["infer"][name]
    net = infer_net(meta, name).cuda().eval()
    ids, lengths = sd[f"{name}/ids"].cuda(), sd[f"{name}/lengths"].cuda()
    sid = sd[f"{name}/sid"].cuda() if c["n_speakers"] else None
    noise = (sd[f"{name}/e_w"], sd[f"{name}/e_z"].cuda())
    with torch.no_grad():
        ref = T.vits2.infer(net, ids, lengths, sid=sid, **c["args"], noise=noise)
        net.dec.precision = "split_f16"
        got = T.vits2.infer(net, ids, lengths, sid=sid, **c["args"], noise=noise)
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    for a, b in zip(got[3], ref[3]):
        assert torch.equal(a, b)
    _close(got[0], ref[0], "infer waveform, split-fp16 generator against the exact one")
    assert not torch.equal(got[0], ref[0])
