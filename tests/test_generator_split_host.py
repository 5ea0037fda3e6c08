"""Host-side checks of the generator's opt-in split-fp16 mode (ttsvits_generator_*, include/ttsdec.h): the four entry points, their
sizes and refusals, the module's `precision` attribute, and a CPU emulation of the arithmetic - every conv with both operands as
hi / lo fp16 planes, the trunk in fp32 - against the fp64 restatement under the generator's own parity bar.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from test_generator_host import LRELU_SLOPE, _gen_dims, load_golden, make_generator, reference_forward, scaled_weights

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-4, 1e-5  # tests/test_generator_hip.py
NEW = ("ttsvits_generator_planes_bytes", "ttsvits_generator_pack_planes", "ttsvits_generator_workspace_bytes", "ttsvits_generator_forward")
FULL = dict(initial_channel=192, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
            upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])


def _lib():
    from torch_tts_amd import _lib

    return _lib, _lib.load()


def _handle(dims):
    _l, lib = _lib()
    h = C.c_void_p()
    assert lib.ttsgen_create(C.byref(dims), C.byref(h)) == _l.OK
    return h


def _small_dims(initial=8, c0=32, rates=(4, 2), dil=(1, 3, 5)):
    """ttsgen_dims with the golden small layout (tests/golden/generator_meta.json "dims") unless told otherwise."""
    _l, _ = _lib()
    d = _l.GenDims()
    d.initial_channel, d.upsample_initial_channel, d.n_up, d.n_res = initial, c0, len(rates), 3
    for i, u in enumerate(rates):
        d.up_rates[i], d.up_kernels[i] = u, 2 * u
    for j, k in enumerate([3, 7, 11]):
        d.res_kernels[j] = k
        for l, dl in enumerate(dil):
            d.res_dilations[j][l] = dl
    d.n_dil, d.resblock, d.gin_channels = 3, 1, 0
    return d


def _up256(nbytes):
    return (nbytes + 255) // 256 * 256


def test_symbols_declared_bound_and_exported():
    _l, lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tts[a-z]+_[a-z_0-9]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in _l.FAMILY_SYMBOLS["ttsvits"] and hasattr(lib, s), s
    assert len(_l.FAMILY_SYMBOLS["ttsgen"]) == 10 and len(_l.FAMILIES) == 6


def test_f32_workspace_is_the_ttsgen_workspace():
    _l, lib = _lib()
    for dims in (_gen_dims(), _small_dims()):
        h = _handle(dims)
        try:
            for B, T in ((64, 600), (5, 600), (1, 1)):
                want = lib.ttsgen_workspace_bytes(h, B, T)
                assert want > 0 and lib.ttsvits_generator_workspace_bytes(h, _l.PREC_F32, B, T) == want, (B, T)
                # split-fp16, every layer split: the same six buffers and cond rows, plus the planes of z (one group's)
                G = min(B, 27) if dims.upsample_initial_channel == 512 else B
                extra = _up256(4 * G * T * dims.initial_channel)
                assert lib.ttsvits_generator_workspace_bytes(h, _l.PREC_SPLIT_F16, B, T) == want + extra, (B, T)
            assert lib.ttsvits_generator_workspace_bytes(h, 7, 5, 600) == 0
        finally:
            lib.ttsgen_destroy(h)


def test_planes_bytes_from_the_dims():
    """Per conv that runs in split-fp16: 2 planes x 2 bytes x its packed weight elements, rounded as the carver rounds (256 bytes).
    conv_post and cond are no GEMMs and have no planes."""
    _l, lib = _lib()
    h = _handle(_gen_dims())
    try:
        n = [512 * 7 * 192]
        cin = 512
        for i, u in enumerate([8, 8, 2, 2]):
            c = 512 >> (i + 1)
            n.append(u * c * 3 * cin)  # the polyphase 3-tap weight [u * Cout, 3 * Cin]
            n += [c * k * c for k in (3, 7, 11) for _ in range(6)]
            cin = c
        assert lib.ttsvits_generator_planes_bytes(h) == sum(_up256(2 * 2 * e) for e in n)
        assert lib.ttsvits_generator_planes_bytes(None) == 0
    finally:
        lib.ttsgen_destroy(h)


def test_planes_bytes_of_channels_that_are_4_mod_8():
    """initial_channel = 12 and stage channels 12: conv_pre and the resblocks stay exact fp32.  upsample_initial_channel is twice the
    first stage's channels - a multiple of 8 for any dims ttsgen_create accepts - so ups[0] still runs in split-fp16 and its planes
    are all there is (planes_bytes cannot be 0).  A dilation the 64-k tiles do not line up with keeps a stage exact as well."""
    _l, lib = _lib()
    h = _handle(_small_dims(initial=12, c0=24, rates=(2,), dil=(1, 1, 1)))
    try:
        assert lib.ttsvits_generator_planes_bytes(h) == _up256(4 * (2 * 12 * 3 * 24))
        # mixed handle: one more activation buffer on top of the fp32 layout (no planes of z: conv_pre is exact)
        F_ = 5 * max(7 * 24, 14 * 12)
        assert lib.ttsvits_generator_workspace_bytes(h, _l.PREC_SPLIT_F16, 5, 7) == lib.ttsgen_workspace_bytes(h, 5, 7) + _up256(4 * F_)
    finally:
        lib.ttsgen_destroy(h)
    h = _handle(_small_dims(initial=8, c0=192, rates=(2,), dil=(1, 3, 1)))  # C = 96: 32 | 96 (exact tiles), neither 96 | 64 nor 64 | 96
    try:
        assert lib.ttsvits_generator_planes_bytes(h) == _up256(4 * 192 * 7 * 8) + _up256(4 * 2 * 96 * 3 * 192)
    finally:
        lib.ttsgen_destroy(h)


def test_refusals_without_a_device():
    _l, lib = _lib()
    h = _handle(_small_dims())
    p = C.c_void_p(256)
    big = 1 << 40
    try:
        fwd = lib.ttsvits_generator_forward
        assert lib.ttsvits_generator_pack_planes(h, p, None) == _l.ERR_NOT_BOUND
        assert lib.ttsvits_generator_pack_planes(None, p, None) == _l.ERR_INVALID_ARG
        for prec in (_l.PREC_F32, _l.PREC_SPLIT_F16):
            assert fwd(h, prec, p, p, None, 1, 4, 2, p, p, big, None) == _l.ERR_NOT_BOUND, prec
        assert lib.ttsgen_bind_weights(h, p) == _l.OK
        assert lib.ttsvits_generator_pack_planes(h, None, None) == _l.ERR_INVALID_ARG
        for bad in (-1, 2, 7):
            assert fwd(h, bad, p, p, None, 1, 4, 2, p, p, big, None) == _l.ERR_INVALID_ARG, bad
        assert fwd(h, _l.PREC_SPLIT_F16, None, p, None, 1, 4, 2, p, p, big, None) == _l.ERR_INVALID_ARG
        for n_stages in (-1, 3):
            assert fwd(h, _l.PREC_SPLIT_F16, p, p, None, 1, 4, n_stages, p, p, big, None) == _l.ERR_INVALID_ARG, n_stages
        for prec in (_l.PREC_F32, _l.PREC_SPLIT_F16):
            need = lib.ttsvits_generator_workspace_bytes(h, prec, 1, 4)
            assert fwd(h, prec, p, p, None, 1, 4, 2, p, p, need - 1, None) == _l.ERR_WORKSPACE, prec
            assert fwd(h, prec, p, p, None, 1, 4, 1, None, p, need - 1, None) == _l.ERR_WORKSPACE, prec
        # (the fp32 size is too short for a split-fp16 call: it lacks the planes of z)
        assert fwd(h, _l.PREC_SPLIT_F16, p, p, None, 1, 4, 2, p, p, lib.ttsgen_workspace_bytes(h, 1, 4), None) == _l.ERR_WORKSPACE
    finally:
        lib.ttsgen_destroy(h)


def test_module_precision_attribute():
    _, meta = load_golden()
    gen = make_generator(meta["dims"])
    assert gen.precision == "f32"
    gen.precision = "split_f16"  # (the attribute is plain; its value is checked where a call reads it)
    gen.precision = "fp16"
    with pytest.raises(ValueError):
        gen(torch.zeros(1, meta["dims"]["initial_channel"], 4))
    from torch_tts_amd.vits2 import _precision_code

    for bad in ("", "bf16", None, 1):
        with pytest.raises(ValueError):
            _precision_code(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the arithmetic, emulated
# ---------------------------------------------------------------------------------------------------------------------------
def _split(x):
    """fp32 -> (hi, lo) as the library splits (common.h split_f16, saturating), lo already scaled back by 2^-11."""
    x = x.float().clamp(-65504.0, 65504.0)
    hi = x.half().float()
    lo = ((x - hi) * 2048.0).half().float() / 2048.0
    return hi.double(), lo.double()


def _sconv(fn, a, w, **kw):
    """fn(a, w) with both operands split: a_hi w_hi + a_hi w_lo + a_lo w_hi (a_lo w_lo is dropped), summed in fp64, result fp32."""
    ah, al = _split(a)
    wh, wl = _split(w)
    return (fn(ah, wh, **kw) + (fn(ah, wl, **kw) + fn(al, wh, **kw))).float()


def _w32(sd, prefix):
    if prefix + ".weight_g" in sd:
        return torch._weight_norm(sd[prefix + ".weight_v"].float(), sd[prefix + ".weight_g"].float(), 0)
    return sd[prefix + ".weight"].float()


def split_forward(sd, dims, x):
    """reference_forward's layers with every conv through _sconv and the trunk - bias, residual, branch sum, division, leaky ReLU - in
    fp32; returns (waveform, the last stage's activated output)."""
    def b(p):
        return sd[p + ".bias"].float()[None, :, None]

    x = _sconv(F.conv1d, x, _w32(sd, "conv_pre"), padding=3) + b("conv_pre")
    nk = len(dims["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(dims["upsample_rates"], dims["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, LRELU_SLOPE)
        x = _sconv(F.conv_transpose1d, x, _w32(sd, f"ups.{i}"), stride=u, padding=(k - u) // 2) + b(f"ups.{i}")
        xs = None
        for j, (kr, dil) in enumerate(zip(dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            xr = x
            for l, d in enumerate(dil):
                xt = F.leaky_relu(xr, LRELU_SLOPE)
                xt = _sconv(F.conv1d, xt, _w32(sd, f"{p}.convs1.{l}"), dilation=d, padding=(kr * d - d) // 2) + b(f"{p}.convs1.{l}")
                xt = F.leaky_relu(xt, LRELU_SLOPE)
                xt = _sconv(F.conv1d, xt, _w32(sd, f"{p}.convs2.{l}"), padding=(kr - 1) // 2) + b(f"{p}.convs2.{l}")
                xr = xt + xr
            xs = xr if xs is None else xs + xr
        x = xs / nk
    x = F.leaky_relu(x)
    return torch.tanh(F.conv1d(x, _w32(sd, "conv_post"), padding=3)), x.transpose(1, 2)


def _worst(a, ref):
    return float(((a.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())


@pytest.mark.parametrize("T", [8, 24])
def test_split_operand_emulation_meets_the_generator_bar(T):
    """ModelConfig dims, B = 1: the split of the GEMM operands alone (products summed in fp64) stays far inside rtol 1e-4 / atol 1e-5 -
    the figures printed here were 0.04 (last stage) and 0.03 (waveform) of the bar when the mode was specified, against 0.14 / 0.08
    for all-fp32 convs - so split mode is held to the exact path's bar, no new number."""
    gen = make_generator(FULL)
    scaled_weights(gen, 5)
    sd = {k: v.detach() for k, v in gen.state_dict().items()}
    z = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        y_ref, acts = reference_forward(sd, FULL, z, stages=True)
        y, last = split_forward(sd, FULL, z)
    assert float(last.abs().max()) < 65504.0
    wy, wl = _worst(y, y_ref), _worst(last, acts[-1])
    print(f"T={T}: worst |err| / (atol + rtol |ref|): waveform {wy:.3f}, last stage {wl:.3f}")
    assert wy < 1.0 and wl < 1.0
