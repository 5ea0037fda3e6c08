"""Host-side checks of the VITS2 duration discriminators (vits2/models.py:183-329): the drop-ins' parameters against the
reference's record, the ttsvits_durdisc_* C ABI's symbols, sizes and refusals, and the fp64 restatement below - the oracle of
tests/test_durdisc_hip.py - against the reference's own outputs (tests/golden/make_golden_durdisc.py).  No GPU needed."""
import ctypes as C
import functools
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
RTOL, ATOL = 1e-4, 1e-5  # the project's bar (tests/test_disc_host.py)
CLASSES = {1: T.DurationDiscriminatorV1, 2: T.DurationDiscriminatorV2}


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "durdisc_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "durdisc_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def make_net(version, C_in, F_ch, seed, gain=1.2):
    """The drop-in with recipe weights (its state-dict keys are the reference's, so fill_by_key draws the reference's values)."""
    net = CLASSES[version](C_in, F_ch, 3, 0.1).eval()
    recipes.fill_by_key(net, seed, gain=gain)
    return net


def length_mask(lengths, T_):
    return (torch.arange(T_)[None, :] < torch.as_tensor(lengths)[:, None]).unsqueeze(1).float()


def _norm(sd, name, x):  # modules.LayerNorm: over the channels, eps 1e-5
    return F.layer_norm(x.transpose(1, -1), (x.shape[1],), sd[name + ".gamma"].to(x.dtype), sd[name + ".beta"].to(x.dtype), 1e-5).transpose(1, -1)


def _conv(sd, name, x):
    return F.conv1d(x, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), padding=1)


def reference_durdisc(sd, version, x, x_mask, durs, dtype=torch.float64):
    """Restatement of DurationDiscriminatorV<version>.forward (models.py:238-257 / 312-329) and forward_probability
    (:222-236 / 298-310) with torch functional ops on a state dict, in fp64 (the oracle; torch.float32: the same ops, for the margin
    condition below): x [B, C, T], x_mask [B, 1, T], durs: [B, 1, T] each -> (trunk h [B, F, T], logits and probabilities
    [B, T, 1] per duration)."""
    x, m = x.to(dtype), x_mask.to(dtype)
    v2 = version == 2
    h = _conv(sd, "conv_1", x * m)
    if v2:
        h = _norm(sd, "norm_1", torch.relu(h))
    h = _conv(sd, "conv_2", h * m)
    if v2:
        h = _norm(sd, "norm_2", torch.relu(h))
    logits, probs = [], []
    for dur in durs:
        logit = reference_logit(sd, version, h, m, dur, dtype)
        logits.append(logit)
        probs.append(torch.sigmoid(logit))
    return h, logits, probs


def reference_logit(sd, version, h, m, dur, dtype=torch.float64):
    """forward_probability up to the Sigmoid: h [B, F, T] -> [B, T, 1]."""
    v2 = version == 2
    h, m = h.to(dtype), m.to(dtype)
    d = F.conv1d(dur.to(dtype), sd["dur_proj.weight"].to(dtype), sd["dur_proj.bias"].to(dtype))
    u = _conv(sd, "pre_out_conv_1", torch.cat([h, d], 1) * m)
    if v2:
        u = _norm(sd, "pre_out_norm_1", torch.relu(u))
    u = _conv(sd, "pre_out_conv_2", u * m)
    if v2:
        u = _norm(sd, "pre_out_norm_2", torch.relu(u))
    return F.linear((u * m).transpose(1, 2), sd["output_layer.0.weight"].to(dtype), sd["output_layer.0.bias"].to(dtype))


# The parity table of tests/test_durdisc_hip.py (here, so that the margin condition below sees the same cases) - in_channels,
# filter_channels, T, lengths:
#   in != filter, N no multiple of 32, K = 72 no multiple of the K tile;  the model's own widths, M = 111 no multiple of a row
#   tile, one utterance of a single token;  one token in all: the convs see only padding;  F = 256;  the row kernels' two- and
#   four-piece forms (F > 256, F > 512), each with a last piece only some lanes hold;
#   the ends of what ttsvits_durdisc_create accepts: C = F = 4;  F = 512 (two whole pieces), 768 (three whole), 772 (the fourth
#   piece partial) and 1024 (four whole);  C = 1024 into F = 4;  C = F = 1024
SHAPES = {"c24f40": (24, 40, 9, [9, 4]), "c192": (192, 192, 37, [37, 20, 1]), "one": (24, 40, 1, [1]), "f256": (192, 256, 5, [5, 2]),
          "f260": (8, 260, 3, [3, 1]), "f516": (8, 516, 2, [2, 1]),
          "c4f4": (4, 4, 5, [5, 2, 1]), "f512": (8, 512, 3, [3, 1]), "f768": (12, 768, 2, [2, 1]), "f772": (8, 772, 2, [2, 1]),
          "c1024f4": (1024, 4, 3, [3, 1]), "max": (1024, 1024, 3, [3, 1])}
MARGIN = 0.5  # of the bar: how far the fp32 restatement may lie from the fp64 one


@functools.lru_cache(maxsize=None)
def shape_case(version, shape):
    """The CPU module of a SHAPES entry with its seeded inputs and the oracle's results - computed once, shared, never modified."""
    C_in, F_ch, T_, lengths = SHAPES[shape]
    B, s = len(lengths), 100 * version + sum(ord(c) for c in shape)
    net = make_net(version, C_in, F_ch, 70 + s)
    x = recipes.seeded_randn(6000 + s, B, C_in, T_)
    dur_r = torch.log(recipes.seeded_ids(7000 + s, 8, B, 1, T_, low=1).float())
    dur_hat = 0.8 + 0.7 * recipes.seeded_randn(8000 + s, B, 1, T_)
    mask = length_mask(lengths, T_)
    h, logits, probs = reference_durdisc(net.state_dict(), version, x, mask, [dur_r, dur_hat])
    return dict(net=net, x=x, mask=mask, dur_r=dur_r, dur_hat=dur_hat, lengths=lengths, h=h, logits=logits, probs=probs)


def bar_ratio(got, ref):
    """max |got - ref| / (ATOL + RTOL |ref|): <= 1 is inside the parity bar."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


@pytest.mark.parametrize("version,shape", [(v, s) for v in (1, 2) for s in SHAPES])
def test_fp32_restatement_stays_within_half_of_the_bar_of_fp64(version, shape):
    """The condition the GPU parity bar rests on - a condition on the case, not a measurement: the same ops in fp32 on the CPU
    differ from the fp64 oracle by at most half of the bar on the trunk (times the mask, as the GPU test compares it), on both
    logits and on both probabilities."""
    c = shape_case(version, shape)
    h, logits, probs = reference_durdisc(c["net"].state_dict(), version, c["x"], c["mask"], [c["dur_r"], c["dur_hat"]], torch.float32)
    assert h.dtype == torch.float32 and c["h"].dtype == torch.float64
    m = c["mask"].double()
    worst = {"trunk": bar_ratio(h * c["mask"], c["h"] * m), "logit": max(bar_ratio(a, b) for a, b in zip(logits, c["logits"])),
             "prob": max(bar_ratio(a, b) for a, b in zip(probs, c["probs"]))}
    print(f"v{version} {shape}: fp32 restatement at " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()) + " of the bar")
    assert max(worst.values()) <= MARGIN, (version, shape, worst)


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel():
        print(f"{what}: {float(((a - b).abs() / (ATOL + RTOL * b.abs())).max()):.4f} of the bar")
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def _dims(version=2, in_channels=192, filter_channels=192, kernel_size=3):
    return _lib.DurDiscDims(version, in_channels, filter_channels, kernel_size)


def test_state_dict_matches_the_reference_record_and_loads_strictly():
    _, meta = load_golden()
    for name, case in meta["cases"].items():
        for v, cls in CLASSES.items():
            net = cls(case["in_channels"], case["filter_channels"], 3, 0.1, gin_channels=7)
            rec = meta["state_dict"][f"v{v}/{name}"]
            assert [[k, list(t.shape)] for k, t in net.state_dict().items()] == rec
            assert sum(p.numel() for p in net.parameters()) == case[f"v{v}"]["n_params"]
            # a reference-shaped state dict loads strictly - V1's unused pre_out norms included
            sd = {k: torch.full(shape, 0.25) for k, shape in rec}
            assert "pre_out_norm_2.beta" in sd and ("norm_1.gamma" in sd) == (v == 2)
            net.load_state_dict(sd, strict=True)
            assert float(net.pre_out_norm_1.gamma.detach()[0]) == 0.25
            assert (net.in_channels, net.filter_channels, net.kernel_size, net.p_dropout, net.gin_channels) == (
                case["in_channels"], case["filter_channels"], 3, 0.1, 7)
            assert getattr(vits2, cls.__name__) is cls
            assert len(net.weight_tensors()) == (12 if v == 1 else 20)
    assert hasattr(T.DurationDiscriminatorV1(8, 8, 3, 0.1), "drop") and not hasattr(T.DurationDiscriminatorV2(8, 8, 3, 0.1), "drop")


def test_restatement_matches_the_reference():
    """The fp64 restatement against the reference's fp32 trunk output, logits, probabilities and loss values; at masked tokens
    its logit is the output layer's bias itself."""
    g, meta = load_golden()
    assert meta["gain"] == 1.2 and -8.5 < meta["logit_range"][0] < -2 and 2 < meta["logit_range"][1] < 8.5
    for name, case in meta["cases"].items():
        x, dur_r, dur_hat = g[f"x/{name}"], g[f"dur_r/{name}"], g[f"dur_hat/{name}"]
        mask = length_mask(case["lengths"], case["T"])
        for v in (1, 2):
            sd = make_net(v, case["in_channels"], case["filter_channels"], meta["seed"], meta["gain"]).state_dict()
            h, logits, probs = reference_durdisc(sd, v, x, mask, [dur_r, dur_hat])
            _close(h.reshape(-1)[::case["trunk_stride"]], g[f"trunk/{name}/v{v}"], f"{name} v{v} trunk")
            for side, lg, p in (("r", logits[0], probs[0]), ("hat", logits[1], probs[1])):
                _close(lg, g[f"logit_{side}/{name}/v{v}"], f"{name} v{v} logit_{side}")
                _close(p, g[f"prob_{side}/{name}/v{v}"], f"{name} v{v} prob_{side}")
                masked = (mask[:, 0] == 0)
                assert int(masked.sum()) == case["T"] * len(case["lengths"]) - sum(case["lengths"])
                if masked.any():
                    assert torch.equal(lg[..., 0][masked], sd["output_layer.0.bias"].double().expand(int(masked.sum())))
            out = (probs[0], probs[1]) if v == 1 else ([probs[0]], [probs[1]])  # forward's nesting, as train.py:394 / 424 takes it
            dr, dg = vits2.discriminator_loss(out[0], out[1])
            want = case[f"v{v}"]
            torch.testing.assert_close(dr, torch.tensor(want["discriminator_loss"][0], dtype=torch.float64), rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(dg, torch.tensor(want["discriminator_loss"][1], dtype=torch.float64), rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(vits2.generator_loss(out[1]), torch.tensor(want["generator_loss"], dtype=torch.float64), rtol=1e-5,
                                       atol=1e-7)


def test_symbols_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ttsvits_durdisc_[a-z_0-9]+)\s*\(", hdr))
    want = {"ttsvits_durdisc_" + n for n in ("create", "destroy", "last_hip_error", "num_weight_tensors", "packed_bytes", "pack_weights",
                                             "bind_weights", "workspace_bytes", "trunk", "prob")}
    assert declared == want
    assert want <= set(_lib.FAMILY_SYMBOLS["ttsvits"]) and "ttsvits_durdisc_set_precision" not in _lib.ALL_SYMBOLS
    lib = _lib.load()
    for s in want:
        assert hasattr(lib, s), s
    assert vits2.DurDiscEngine.PREFIX == "ttsvits_durdisc"
    # the pins of the other families stay
    assert len(_lib.FAMILIES) == 6 and [f.prefix for f in _lib.FAMILIES] == ["ttsdec", "ttsenc", "ttsvits", "ttsgen", "ttsdur", "ttspost"]
    assert lib.ttsdec_version() == 2
    assert len(_lib.FAMILY_SYMBOLS["ttsgen"]) == 10 and len(_lib.FAMILY_SYMBOLS["ttsdur"]) == 12
    assert {s for s in _lib.ALL_SYMBOLS if s.startswith("ttsvits_disc_")} == {"ttsvits_disc_" + n for n in (
        "create", "destroy", "last_hip_error", "num_weight_tensors", "packed_bytes", "pack_weights", "bind_weights", "workspace_bytes", "forward")}
    assert set(re.findall(r"\b(tts[a-z]+_[a-z_0-9]+)\s*\(", hdr)) == set(_lib.ALL_SYMBOLS)


def test_sizes_and_c_abi_refusals():
    lib = _lib.load()
    h = C.c_void_p()
    for bad in (dict(kernel_size=1), dict(kernel_size=5), dict(kernel_size=0), dict(version=0), dict(version=3), dict(in_channels=190),
                dict(filter_channels=6), dict(in_channels=0), dict(filter_channels=-4), dict(in_channels=1028), dict(filter_channels=2048)):
        assert lib.ttsvits_durdisc_create(C.byref(_dims(**bad)), C.byref(h)) == _lib.ERR_DIMS, bad
        assert not h.value
    assert lib.ttsvits_durdisc_workspace_bytes(None, 1, 100, 2) == 0 and lib.ttsvits_durdisc_packed_bytes(None) == 0
    vp = C.c_void_p(256)
    for v, C_in, F_ch in ((1, 192, 192), (2, 192, 256), (2, 24, 40), (1, 1024, 1024)):
        assert lib.ttsvits_durdisc_create(C.byref(_dims(v, C_in, F_ch)), C.byref(h)) == _lib.OK
        try:
            n_w = 12 if v == 1 else 20
            assert lib.ttsvits_durdisc_num_weight_tensors(h) == n_w
            # the blob: the three F x F x 3 convs, conv_1, the two folded tables in place of pre_out_conv_1's second half and of
            # dur_proj, the vectors - each tensor padded to 256 bytes
            want = 3 * F_ch * F_ch * 3 + F_ch * C_in * 3 + 2 * 3 * F_ch + 5 * F_ch + 1 + (8 * F_ch if v == 2 else 0)
            nb = lib.ttsvits_durdisc_packed_bytes(h)
            assert nb % 256 == 0 and 4 * want <= nb <= 4 * want + 24 * 256
            for n_dur in (1, 2):  # monotone in B, in T and in n_dur
                prev = 0
                for B, Tn in ((1, 1), (1, 9), (2, 9), (2, 150), (3, 150), (3, 151), (64, 150)):
                    ws = lib.ttsvits_durdisc_workspace_bytes(h, B, Tn, n_dur)
                    assert ws % 256 == 0 and ws >= prev and ws > 0, (v, B, Tn, n_dur)
                    assert n_dur == 1 or ws >= lib.ttsvits_durdisc_workspace_bytes(h, B, Tn, 1)
                    prev = ws
            M = 64 * 150  # what the two calls carve at n_dur = 2: mask, x * m, three [M, F] buffers, two [2 M, F]
            assert lib.ttsvits_durdisc_workspace_bytes(h, 64, 150, 2) == 4 * (M + M * max(C_in, F_ch) + 3 * M * F_ch + 4 * M * F_ch)
            for B, Tn, n_dur in ((0, 100, 1), (1, 0, 1), (-1, 5, 2), (1, 100, 0), (1, 100, 3)):
                assert lib.ttsvits_durdisc_workspace_bytes(h, B, Tn, n_dur) == 0
            # row indices beyond 32 bits: reported by the size function, refused by the calls
            assert lib.ttsvits_durdisc_workspace_bytes(h, 1 << 10, 1 << 9, 2) == 0 and lib.ttsvits_durdisc_workspace_bytes(h, 1 << 10, 1 << 9, 1) == 0
            big = 1 << 40
            assert lib.ttsvits_durdisc_trunk(h, vp, vp, 1, 100, vp, vp, big, None) == _lib.ERR_NOT_BOUND
            assert lib.ttsvits_durdisc_prob(h, vp, vp, vp, 2, 1, 100, vp, None, vp, big, None) == _lib.ERR_NOT_BOUND
            assert lib.ttsvits_durdisc_pack_weights(h, None, n_w, vp, None) != _lib.OK
            assert lib.ttsvits_durdisc_bind_weights(h, vp) == _lib.OK  # (a pointer no call below gets as far as reading)
            need = lib.ttsvits_durdisc_workspace_bytes(h, 1, 100, 2)
            for args in ((None, vp, 1, 100, vp, vp, big), (vp, None, 1, 100, vp, vp, big), (vp, vp, 1, 100, None, vp, big),
                         (vp, vp, 0, 100, vp, vp, big), (vp, vp, 1, 0, vp, vp, big), (vp, vp, 1, 100, vp, None, big),
                         (vp, vp, 1, 100, vp, vp, lib.ttsvits_durdisc_workspace_bytes(h, 1, 100, 1) - 1)):
                assert lib.ttsvits_durdisc_trunk(h, *args, None) == _lib.ERR_INVALID_ARG, args
            for args in ((None, vp, vp, 2, 1, 100, vp, None, vp, big), (vp, None, vp, 2, 1, 100, vp, None, vp, big),
                         (vp, vp, None, 2, 1, 100, vp, None, vp, big), (vp, vp, vp, 2, 1, 100, None, None, vp, big),
                         (vp, vp, vp, 0, 1, 100, vp, None, vp, big), (vp, vp, vp, 3, 1, 100, vp, None, vp, big),
                         (vp, vp, vp, 2, 0, 100, vp, None, vp, big), (vp, vp, vp, 2, 1, -1, vp, None, vp, big),
                         (vp, vp, vp, 2, 1, 100, vp, None, None, big), (vp, vp, vp, 2, 1, 100, vp, None, vp, need - 1),
                         (vp, vp, vp, 2, 1, 100, vp, vp, vp, need - 256)):
                assert lib.ttsvits_durdisc_prob(h, *args, None) == _lib.ERR_INVALID_ARG, args
            assert lib.ttsvits_durdisc_prob(h, vp, vp, vp, 2, 1 << 10, 1 << 9, vp, None, vp, big, None) == _lib.ERR_DIMS
        finally:
            lib.ttsvits_durdisc_destroy(h)


def test_engine_host_queries():
    e = vits2.DurDiscEngine(dict(version=2, in_channels=192, filter_channels=192, kernel_size=3), None)
    assert e.num_weight_tensors() == 20 and e.workspace_bytes(64, 150) == e.workspace_bytes(64, 150, 2) > e.workspace_bytes(64, 150, 1) > 0
    with pytest.raises(NotImplementedError):  # (DimsNotBuilt: a refusal, never another computation)
        vits2.DurDiscEngine(dict(version=1, in_channels=192, filter_channels=192, kernel_size=5), None)


def test_module_refusals():
    for v, cls in CLASSES.items():
        net = cls(24, 40, 3, 0.1).eval()
        x, m, d = torch.randn(2, 24, 9), torch.ones(2, 1, 9), torch.randn(2, 1, 9)
        with torch.no_grad():
            with pytest.raises(NotImplementedError):  # CPU tensors: no fallback
                net(x, m, d, d)
            with pytest.raises(NotImplementedError):
                net.forward_probability(torch.randn(2, 40, 9), m, d)
            for bad in ((x[0], m, d, d), (x[:, :20], m, d, d), (x, m[:, 0], d, d), (x, m, d[:, 0], d), (x, m, d, d[:, :, :5]),
                        (x, m[:1], d, d)):  # wrong ranks and shapes
                with pytest.raises(ValueError):
                    net(*bad)
            with pytest.raises(ValueError):
                net.forward_probability(x, m, d)  # (takes the trunk's output [B, F, T], not x)
            with pytest.raises(NotImplementedError):  # fp64 (on the device the dtype guard names it: tests/test_durdisc_hip.py)
                net.double()(x.double(), m.double(), d.double(), d.double())
        with pytest.raises(NotImplementedError):  # grad enabled
            net.float()(x, m, d, d)
    with pytest.raises(TypeError):
        vits2.duration_discriminator_scores(torch.nn.Module(), torch.nn.Module(), x, None, x, None)
