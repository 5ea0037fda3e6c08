"""Host-side checks of the VITS2 waveform discriminators (vits2/models.py:977-1110): the drop-ins' parameters against the
reference's record, the ttsvits_disc_* C ABI's symbols, sizes and refusals, and the fp64 restatement below - the oracle of
tests/test_disc_hip.py - against the reference's own outputs (tests/golden/make_golden_disc.py).  No GPU needed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipes
import torch_tts_amd as T
from torch_tts_amd import _lib, vits2

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LRELU_SLOPE = 0.1
PERIODS = [0, 2, 3, 5, 7, 11]  # discriminators.0 is DiscriminatorS
RTOL, ATOL = 1e-4, 1e-5


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "disc_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "disc_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def make_mpd(seed, gain=1.2):
    """The drop-in with the recipe weights the golden file was made with (its state-dict keys are the reference's)."""
    mpd = T.MultiPeriodDiscriminator().eval()
    recipes.fill_by_key(mpd, seed, gain=gain)
    return mpd


def _conv(sd, prefix):
    w = torch._weight_norm(sd[prefix + ".weight_v"].double(), sd[prefix + ".weight_g"].double(), 0)
    return w, sd[prefix + ".bias"].double()


def reference_disc(sd, d, x, period=None, stride=3, prefix=None):
    """fp64 restatement of discriminators.<d> (models.py:1034-1053 for d >= 1, :1072-1083 for d = 0) with torch functional ops on
    the state dict sd of a MultiPeriodDiscriminator.  x [B, 1, T] -> (scores [B, L], fmap list) in the reference's shapes.
    A DiscriminatorP of other dims (d >= 1): its `period` (default PERIODS[d]) and `stride` as arguments, the kernel size from the
    weights, and `prefix` where its keys start ("" for the state dict of a DiscriminatorP on its own)."""
    x = x.double()
    pre = f"discriminators.{d}." if prefix is None else prefix
    fmap = []
    if d == 0:
        for i, (stride, groups, pad) in enumerate([(1, 1, 7), (4, 4, 20), (4, 16, 20), (4, 64, 20), (4, 256, 20), (1, 1, 2)]):
            w, b = _conv(sd, f"{pre}convs.{i}")
            x = F.leaky_relu(F.conv1d(x, w, b, stride=stride, padding=pad, groups=groups), LRELU_SLOPE)
            fmap.append(x)
        w, b = _conv(sd, pre + "conv_post")
        x = F.conv1d(x, w, b, padding=1)
    else:
        p = PERIODS[d] if period is None else period
        b_, c, t = x.shape
        if t % p != 0:
            x = F.pad(x, (0, p - t % p), "reflect")
        x = x.view(b_, c, -1, p)
        for i in range(5):
            w, b = _conv(sd, f"{pre}convs.{i}")
            k = w.shape[2]
            x = F.leaky_relu(F.conv2d(x, w, b, stride=(stride if i < 4 else 1, 1), padding=((k - 1) // 2, 0)), LRELU_SLOPE)
            fmap.append(x)
        w, b = _conv(sd, pre + "conv_post")
        x = F.conv2d(x, w, b, padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def reference_mpd(sd, y, y_hat):
    """The four lists of MultiPeriodDiscriminator.forward (models.py:1097-1110), fp64."""
    outs = [[], [], [], []]
    for d in range(len(PERIODS)):
        s_r, f_r = reference_disc(sd, d, y)
        s_g, f_g = reference_disc(sd, d, y_hat)
        for lst, v in zip(outs, (s_r, s_g, f_r, f_g)):
            lst.append(v)
    return outs


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _dims(period=2, kernel_size=5, stride=3):
    return _lib.DiscDims(period, kernel_size, stride)


def test_state_dict_matches_the_reference_record():
    _, meta = load_golden()
    mpd = T.MultiPeriodDiscriminator()
    assert [[k, list(v.shape)] for k, v in mpd.state_dict().items()] == meta["state_dict"]
    assert sum(p.numel() for p in mpd.parameters()) == meta["n_params"] == 46747132
    assert "discriminators.3.convs.2.weight_g" in mpd.state_dict() and "discriminators.0.conv_post.weight_v" in mpd.state_dict()
    for cls in (T.DiscriminatorS, T.DiscriminatorP, T.MultiPeriodDiscriminator):
        assert getattr(vits2, cls.__name__) is cls
    assert T.DiscriminatorP(7).period == 7


def test_restatement_matches_the_reference():
    """The fp64 restatement against the reference's fp32 outputs: all scores, the stride-13 samples and mean |.| of every
    feature map, and the three loss terms (vits2.feature_loss / discriminator_loss / generator_loss on the restated lists)."""
    g, meta = load_golden()
    sd = make_mpd(meta["seed"], meta["gain"]).state_dict()
    stride = meta["stride"]
    assert stride == 13
    for name, case in meta["cases"].items():
        y, y_hat = g[f"y/{name}"], g[f"y_hat/{name}"]
        s_r, s_g, f_r, f_g = reference_mpd(sd, y, y_hat)
        for side, scores, fmaps in (("r", s_r, f_r), ("g", s_g, f_g)):
            for d in range(len(PERIODS)):
                _close(scores[d], g[f"score_{side}/{name}/{d}"], f"{name} score_{side} {d}")
                assert len(fmaps[d]) == (7 if d == 0 else 6)
                for l, f in enumerate(fmaps[d]):
                    rec = case["fmaps"][f"{side}/{d}/{l}"]
                    assert list(f.shape) == rec["shape"]
                    _close(f.reshape(-1)[::stride], g[f"fmap_{side}/{name}/{d}/{l}"], f"{name} fmap_{side} {d}/{l}")
                    assert float(f.abs().mean()) == pytest.approx(rec["mean_abs"], rel=1e-5)
        assert float(vits2.feature_loss(f_r, f_g)) == pytest.approx(case["feature_loss"], rel=1e-5)
        dr, dg = vits2.discriminator_loss(s_r, s_g)
        assert dr.shape == dg.shape == (6,)
        torch.testing.assert_close(dr, torch.tensor(case["discriminator_loss"][0], dtype=torch.float64), rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(dg, torch.tensor(case["discriminator_loss"][1], dtype=torch.float64), rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(vits2.generator_loss(s_g), torch.tensor(case["generator_loss"], dtype=torch.float64), rtol=1e-5, atol=1e-7)


def test_symbols_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ttsvits_disc_[a-z_0-9]+)\s*\(", hdr))
    want = {"ttsvits_disc_" + n for n in ("create", "destroy", "last_hip_error", "num_weight_tensors", "packed_bytes", "pack_weights",
                                          "bind_weights", "workspace_bytes", "forward")}
    assert declared == want
    assert want <= set(_lib.FAMILY_SYMBOLS["ttsvits"]) and "ttsvits_disc_set_precision" not in _lib.ALL_SYMBOLS
    lib = _lib.load()
    for s in want:
        assert hasattr(lib, s), s
    # the pins of the other families stay
    assert len(_lib.FAMILIES) == 6 and [f.prefix for f in _lib.FAMILIES] == ["ttsdec", "ttsenc", "ttsvits", "ttsgen", "ttsdur", "ttspost"]
    assert lib.ttsdec_version() == 2
    assert len(_lib.FAMILY_SYMBOLS["ttsgen"]) == 10 and len(_lib.FAMILY_SYMBOLS["ttsdur"]) == 12
    assert len([s for s in _lib.FAMILY_SYMBOLS["ttsenc"] if s.startswith("ttsenc_style_")]) == 9
    assert set(re.findall(r"\b(tts[a-z]+_[a-z_0-9]+)\s*\(", hdr)) == set(_lib.ALL_SYMBOLS)


def test_sizes_and_c_abi_refusals():
    lib = _lib.load()
    h = C.c_void_p()
    for bad in (dict(period=-1), dict(kernel_size=4), dict(kernel_size=17), dict(stride=0), dict(stride=17), dict(period=5000)):
        assert lib.ttsvits_disc_create(C.byref(_dims(**bad)), C.byref(h)) == _lib.ERR_DIMS, bad
    assert lib.ttsvits_disc_workspace_bytes(None, 1, 100) == 0 and lib.ttsvits_disc_packed_bytes(None) == 0
    n_params = {0: 0, 2: 0}
    sd = T.MultiPeriodDiscriminator().state_dict()
    for d, p in ((0, 0), (1, 2)):  # elements of the effective weights and biases: the blob holds each, padded to 256 bytes
        n_params[p] = sum(v.numel() for k, v in sd.items() if k.startswith(f"discriminators.{d}.") and not k.endswith("weight_g"))
    for p in (0, 2, 11):
        assert lib.ttsvits_disc_create(C.byref(_dims(period=p)), C.byref(h)) == _lib.OK
        try:
            assert lib.ttsvits_disc_num_weight_tensors(h) == (14 if p == 0 else 12)
            nb = lib.ttsvits_disc_packed_bytes(h)
            want = n_params[0 if p == 0 else 2]
            assert nb % 256 == 0 and 4 * want <= nb <= 4 * want + 14 * 256
            prev = 0
            for B, Tn in ((1, 12), (1, 97), (2, 97), (2, 2310), (3, 2310), (3, 2311), (64, 8192)):  # monotone in B and in T
                ws = lib.ttsvits_disc_workspace_bytes(h, B, Tn)
                assert ws % 256 == 0 and ws >= prev > -1 and ws > 0, (p, B, Tn)
                prev = ws
            assert lib.ttsvits_disc_workspace_bytes(h, 0, 100) == 0 and lib.ttsvits_disc_workspace_bytes(h, 1, 0) == 0
            # indices beyond 32 bits: reported by the size function, refused by the call
            assert lib.ttsvits_disc_workspace_bytes(h, 1 << 16, 1 << 15) == 0
            if p:  # the reflect pad the reference itself refuses: p - T % p >= T
                assert lib.ttsvits_disc_workspace_bytes(h, 1, 1) == 0
                assert lib.ttsvits_disc_workspace_bytes(h, 1, p) > 0  # (no pad at all)
            vp = C.c_void_p(256)
            assert lib.ttsvits_disc_forward(h, vp, 1, 100, vp, None, vp, 1 << 40, None) == _lib.ERR_NOT_BOUND
            assert lib.ttsvits_disc_forward(h, None, 1, 100, vp, None, vp, 1 << 40, None) == _lib.ERR_INVALID_ARG
            assert lib.ttsvits_disc_forward(h, vp, 0, 100, vp, None, vp, 1 << 40, None) == _lib.ERR_INVALID_ARG
            assert lib.ttsvits_disc_pack_weights(h, None, 12, vp, None) != _lib.OK
        finally:
            lib.ttsvits_disc_destroy(h)


def test_engine_host_queries():
    e = vits2.DiscEngine(dict(period=3, kernel_size=5, stride=3), None)
    assert e.num_weight_tensors() == 12 and e.heights(2310) == [257, 86, 29, 10, 10, 10]
    # conv i writes buffer i & 1: [B, p, H_i, C_i] floats, each buffer rounded up to 256 bytes
    up = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    assert e.workspace_bytes(2, 2310) == up(2 * 3 * max(257 * 32, 29 * 512, 10 * 1024)) + up(2 * 3 * max(86 * 128, 10 * 1024))
    s = vits2.DiscEngine(dict(period=0, kernel_size=0, stride=0), None)
    assert s.num_weight_tensors() == 14 and s.heights(2310) == [2310, 578, 145, 37, 10, 10, 10]


def test_module_refusals():
    for cls, args in ((T.DiscriminatorS, ()), (T.DiscriminatorP, (3,)), (T.MultiPeriodDiscriminator, ())):
        with pytest.raises(NotImplementedError):
            cls(*args, use_spectral_norm=True)
    dp, ds = T.DiscriminatorP(5).eval(), T.DiscriminatorS().eval()
    x = torch.randn(2, 1, 100)
    with torch.no_grad():
        for m in (dp, ds):
            with pytest.raises(NotImplementedError):  # CPU tensors: no fallback
                m(x)
            with pytest.raises(ValueError):
                m(torch.randn(2, 100))
        with pytest.raises(ValueError):  # T = 2, period 5: the pad (3) is not smaller than T
            dp(torch.randn(1, 1, 2))
        with pytest.raises(NotImplementedError):
            T.MultiPeriodDiscriminator()(x, x)
        with pytest.raises(ValueError):
            T.MultiPeriodDiscriminator()(x, x[:, :, :50])
