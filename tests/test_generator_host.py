"""Host-side checks of the VITS2 HiFi-GAN generator (vits2/models.py:900-974): the drop-in's parameters against the reference's,
the ttsgen_* C ABI's refusals, and the fp64 restatement below - the oracle of tests/test_generator_hip.py - against the reference's
own outputs (tests/golden/make_golden_generator.py).  No GPU needed."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
LRELU_SLOPE = 0.1


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "generator_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "generator_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def weights(sd, gin):
    """{state-dict key: tensor} of one generator from the golden file's `w<gin>/` entries."""
    pre = f"w{gin}/"
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def _w(sd, prefix):
    if prefix + ".weight_g" in sd:  # torch.nn.utils.weight_norm, dim 0 (ConvTranspose1d: per input channel)
        return torch._weight_norm(sd[prefix + ".weight_v"].double(), sd[prefix + ".weight_g"].double(), 0)
    return sd[prefix + ".weight"].double()


def reference_forward(sd, dims, x, g=None, stages=False):
    """fp64 restatement of Generator.forward (models.py:947-968, ResBlock1.forward modules.py:296-309 without x_mask) with torch
    functional ops.  x [B, C, T], g [B, gin, 1] or None -> [B, 1, T'] fp64; stages=True also returns the activated output of
    conv_pre and of every stage, channel-last [B, T_s, C_s] (what Generator.stage_outputs reads back)."""
    x = x.double()
    x = F.conv1d(x, _w(sd, "conv_pre"), sd["conv_pre.bias"].double(), padding=3)
    if g is not None:
        x = x + F.conv1d(g.double(), _w(sd, "cond"), sd["cond.bias"].double())
    acts = []
    nk = len(dims["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(dims["upsample_rates"], dims["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, LRELU_SLOPE)
        acts.append(x.transpose(1, 2))
        x = F.conv_transpose1d(x, _w(sd, f"ups.{i}"), sd[f"ups.{i}.bias"].double(), stride=u, padding=(k - u) // 2)
        xs = None
        for j, (kr, dil) in enumerate(zip(dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            xr = x
            for l, d in enumerate(dil):
                xt = F.leaky_relu(xr, LRELU_SLOPE)
                xt = F.conv1d(xt, _w(sd, f"{p}.convs1.{l}"), sd[f"{p}.convs1.{l}.bias"].double(), dilation=d, padding=(kr * d - d) // 2)
                xt = F.leaky_relu(xt, LRELU_SLOPE)
                xt = F.conv1d(xt, _w(sd, f"{p}.convs2.{l}"), sd[f"{p}.convs2.{l}.bias"].double(), padding=(kr - 1) // 2)
                xr = xt + xr
            xs = xr if xs is None else xs + xr
        x = xs / nk
    x = F.leaky_relu(x)  # models.py:963: default slope 0.01
    acts.append(x.transpose(1, 2))
    y = torch.tanh(F.conv1d(x, _w(sd, "conv_post"), padding=3))
    return (y, acts) if stages else y


def scaled_weights(gen, seed):
    """The golden file's weight scaling (make_golden_generator.randomize) for a drop-in Generator: every stage's activations
    O(1), few saturated output samples."""
    gsd = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in gen.named_parameters():
            if n.endswith("weight_g"):
                p.copy_(0.6 + 0.4 * torch.rand(p.shape, generator=gsd))
            elif n.endswith("weight_v") or n.endswith("weight"):
                fan_in = p[0].numel() if not n.startswith("ups") else p.shape[0] * p.shape[2]
                p.copy_(torch.randn(p.shape, generator=gsd) / fan_in**0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gsd))


def _T():
    import torch_tts_amd as T

    return T


def make_generator(dims, gin=0):
    T = _T()
    return T.Generator(dims["initial_channel"], dims["resblock"], dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"],
                       dims["upsample_rates"], dims["upsample_initial_channel"], dims["upsample_kernel_sizes"], gin_channels=gin)


def test_state_dict_matches_reference_record():
    _, meta = load_golden()
    gen = make_generator(meta["fulldims"])
    got = [[k, list(v.shape)] for k, v in gen.state_dict().items()]
    assert got == meta["fulldims_state_dict"]
    assert len(got) == 231 and sum(math.prod(s) for _, s in got) == 14337024
    assert list(gen.state_dict()["ups.0.weight_g"].shape) == [512, 1, 1]
    sd, _ = load_golden()
    for gin in (0, 4):
        small = make_generator(meta["dims"], gin)
        ref = weights(sd, gin)
        assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == [(k, tuple(v.shape)) for k, v in ref.items()]


def test_reference_state_dict_loads_before_and_after_remove_weight_norm():
    sd, meta = load_golden()
    ref = weights(sd, 4)
    gen = make_generator(meta["dims"], 4)
    gen.load_state_dict(ref, strict=True)
    eff = [t.detach().clone() for t in gen.weight_tensors()]
    assert len(eff) == 2 + 2 * 2 + 12 * 2 * 3 + 1 + 2
    assert torch.allclose(eff[2], torch._weight_norm(ref["ups.0.weight_v"], ref["ups.0.weight_g"], 0))
    gen.remove_weight_norm()
    keys = list(gen.state_dict())
    assert "ups.0.weight" in keys and not any(k.endswith(("weight_g", "weight_v")) for k in keys)
    for a, b in zip(eff, gen.weight_tensors()):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)
    plain = make_generator(meta["dims"], 4)
    plain.remove_weight_norm()
    plain.load_state_dict(gen.state_dict(), strict=True)  # the plain-weight form loads too
    for a, b in zip(eff, plain.weight_tensors()):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)


def test_resblock2_refused_by_module():
    _, meta = load_golden()
    d = dict(meta["dims"], resblock="2")
    with pytest.raises(NotImplementedError):
        make_generator(d)


def _gen_dims(**over):
    from torch_tts_amd import _lib

    d = _lib.GenDims()
    d.initial_channel, d.upsample_initial_channel, d.n_up, d.n_res = 192, 512, 4, 3
    for i, (u, k) in enumerate(zip([8, 8, 2, 2], [16, 16, 4, 4])):
        d.up_rates[i], d.up_kernels[i] = u, k
    for j, k in enumerate([3, 7, 11]):
        d.res_kernels[j] = k
        for l, dl in enumerate([1, 3, 5]):
            d.res_dilations[j][l] = dl
    d.n_dil, d.resblock, d.gin_channels = 3, 1, 0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_c_abi_symbols_refusals_and_not_bound():
    from torch_tts_amd import _lib

    lib = _lib.load()
    import re

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(HERE), "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ttsgen_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.GEN_SYMBOLS) and len(declared) == 10, declared ^ set(_lib.GEN_SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), s
    h = C.c_void_p()
    for bad in (dict(resblock=2), dict(n_dil=2), dict(up_kernels=(0, 15)), dict(up_kernels=(2, 6)), dict(up_rates=(1, 3)),
                dict(res_kernels=(0, 4)), dict(upsample_initial_channel=510), dict(initial_channel=190)):
        assert lib.ttsgen_create(C.byref(_gen_dims(**bad)), C.byref(h)) == _lib.ERR_DIMS, bad
    assert lib.ttsgen_create(C.byref(_gen_dims()), C.byref(h)) == _lib.OK
    try:
        assert lib.ttsgen_num_weight_tensors(h) == 155
        # groups of 27 utterances at T = 600 (65535 row tiles of 64 over 153600 output frames): six activation buffers of
        # 153600 x 32 floats per utterance plus the cond rows - sized for one group, not for B
        assert lib.ttsgen_workspace_bytes(h, 64, 600) == (6 * 27 * 153600 * 32 + 27 * 512) * 4
        assert lib.ttsgen_workspace_bytes(h, 128, 600) == lib.ttsgen_workspace_bytes(h, 27, 600)
        assert lib.ttsgen_workspace_bytes(h, 5, 600) == (6 * 5 * 153600 * 32 + 5 * 512) * 4
        rc = lib.ttsgen_forward(h, C.c_void_p(256), None, 1, 4, C.c_void_p(256), C.c_void_p(256), 1 << 40, None)
        assert rc == _lib.ERR_NOT_BOUND
    finally:
        lib.ttsgen_destroy(h)


def test_restatement_reproduces_reference_outputs():
    sd, meta = load_golden()
    for gin in (0, 4):
        w = weights(sd, gin)
        for T in meta["T"]:
            x = sd[f"x{gin}/T{T}"]
            g = sd[f"g{gin}/T{T}"] if gin else None
            y = reference_forward(w, meta["dims"], x, g)
            ref = sd[f"y{gin}/T{T}"].double()
            assert y.shape == ref.shape
            assert (y - ref).abs().max().item() < 1e-6, (gin, T)
