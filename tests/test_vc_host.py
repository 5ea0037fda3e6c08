"""Host-side checks of VITS2 voice conversion (vits2/models.py:1328-1336): the torch-op restatement below - the oracle of
tests/test_vc_hip.py - of the PosteriorEncoder (models.py:858-897), of the flow's forward direction (models.py:803-806 over :506-526) and
of the whole conversion, against the reference's own outputs (tests/golden/make_golden_vc.py); the drop-in's state-dict keys against the
reference's enc_q; the ttspost_* C ABI's exports and tensor count; and voice_conversion's refusals.  No GPU needed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import vits2_oracle as V
from test_duration_host import randomize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "vc_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "vc_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def weights(sd, prefix):
    pre = f"{prefix}/w/"
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


# ---------------------------------------------------------------------------------------------------------------------------
# torch-op restatement (any float dtype: the weights are cast to y's)
# ---------------------------------------------------------------------------------------------------------------------------
def _cast(wts, dt):
    return {k: v.to(dt) for k, v in wts.items()}


def posterior_encoder(wts, y, lengths, g, noise, n_layers, kernel):
    """PosteriorEncoder.forward (models.py:887-897) with the draw given: -> z, m, logs, x_mask ([B, C, T])."""
    wts = _cast(wts, y.dtype)
    T = y.shape[2]
    x_mask = V.sequence_mask(lengths.cpu(), T).unsqueeze(1).to(device=y.device, dtype=y.dtype)
    x = F.conv1d(y, wts["pre.weight"], wts["pre.bias"]) * x_mask
    x = V.wn(x, x_mask, wts, "enc", n_layers, kernel, g=None if g is None else g.to(y.dtype))
    stats = F.conv1d(x, wts["proj.weight"], wts["proj.bias"]) * x_mask
    m, logs = torch.split(stats, stats.shape[1] // 2, dim=1)
    z = (m + noise[:, :, :T].to(y.dtype) * torch.exp(logs)) * x_mask
    return z, m, logs, x_mask


def flow_dims(channels, hidden, kernel, n_layers, n_flows=4, gin=0):
    return V.Vits2Dims(inter_channels=channels, flow_hidden=hidden, flow_kernel=kernel, flow_wn_layers=n_layers, n_flows=n_flows,
                       gin_channels=gin)


def coupling_forward(x, x_mask, wts, prefix, d, g=None):
    """ResidualCouplingTransformersLayer.forward(reverse=False), mean-only (models.py:506-526), without the logdet."""
    half = d.inter_channels // 2
    x0, x1 = torch.split(x, [half, half], 1)
    x0_ = V.encoder_stack(x0 * x_mask, x_mask, wts, prefix + ".pre_transformer", d.flow_tf_layers, d.flow_tf_heads, None, d.flow_tf_kernel)
    x0_ = x0_ + x0
    h = F.conv1d(x0_, wts[prefix + ".pre.weight"], wts[prefix + ".pre.bias"]) * x_mask
    h = V.wn(h, x_mask, wts, prefix + ".enc", d.flow_wn_layers, d.flow_kernel, g=g)
    m = F.conv1d(h, wts[prefix + ".post.weight"], wts[prefix + ".post.bias"]) * x_mask
    x1 = m + x1 * x_mask  # logs = 0 in mean-only mode: exp(logs) = 1
    return torch.cat([x0, x1], 1)


def flow_forward(x, x_mask, wts, d, prefix="flow", g=None):
    """ResidualCouplingTransformersBlock.forward(reverse=False) (models.py:803-806): layer_0, Flip, layer_1, Flip, ..."""
    wts = _cast(wts, x.dtype)
    g = None if g is None else g.to(x.dtype)
    for i in range(d.n_flows):
        x = coupling_forward(x, x_mask, wts, f"{prefix}.flows.{2 * i}", d, g=g)
        x = torch.flip(x, [1])  # modules.Flip (modules.py:374-381)
    return x


def generator(wts, x, g=None, upsample_rates=(), n_res=3, res_kernels=(), res_dilations=()):
    """Generator.forward (models.py:947-968) on weight-normed or plain weights, in x's dtype."""
    wts = _cast(wts, x.dtype)
    x = F.conv1d(x, wts["conv_pre.weight"], wts["conv_pre.bias"], padding=3)
    if g is not None:
        x = x + F.conv1d(g.to(x.dtype), wts["cond.weight"], wts["cond.bias"])
    for i, u in enumerate(upsample_rates):
        x = F.leaky_relu(x, 0.1)
        k = 2 * u
        x = F.conv_transpose1d(x, V.weight_norm_weight(wts, f"ups.{i}"), wts[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        xs = None
        for j in range(n_res):
            p = f"resblocks.{i * n_res + j}"
            xr = x
            for l, dl in enumerate(res_dilations[j]):
                kk = res_kernels[j]
                xt = F.leaky_relu(xr, 0.1)
                xt = F.conv1d(xt, V.weight_norm_weight(wts, f"{p}.convs1.{l}"), wts[f"{p}.convs1.{l}.bias"], dilation=dl, padding=(kk * dl - dl) // 2)
                xt = F.leaky_relu(xt, 0.1)
                xt = F.conv1d(xt, V.weight_norm_weight(wts, f"{p}.convs2.{l}"), wts[f"{p}.convs2.{l}.bias"], padding=(kk - 1) // 2)
                xr = xt + xr
            xs = xr if xs is None else xs + xr
        x = xs / n_res
    x = F.leaky_relu(x)
    x = F.conv1d(x, wts["conv_post.weight"], None, padding=3)
    return torch.tanh(x)


def voice_conversion(net, y, lengths, sid_src, sid_tgt, noise, dtype=torch.float64):
    """SynthesizerTrn.voice_conversion (models.py:1328-1336) over a model's state dicts, in dtype: -> o_hat, y_mask, (z, z_p, z_hat)."""
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    part = lambda p: {k[len(p) + 1:]: v for k, v in sd.items() if k.startswith(p + ".")}  # noqa: E731
    emb = sd["emb_g.weight"].to(dtype)
    g_src, g_tgt = emb[sid_src.cpu()].unsqueeze(-1), emb[sid_tgt.cpu()].unsqueeze(-1)
    eq = net.enc_q
    y = y.detach().cpu().to(dtype)
    lengths = lengths.cpu()
    z, _, _, y_mask = posterior_encoder(part("enc_q"), y, lengths, g_src, noise.cpu(), eq.n_layers, eq.kernel_size)
    fl = net.flow
    d = flow_dims(fl.channels, fl.hidden_channels, fl.kernel_size, fl.n_layers, fl.n_flows, fl.gin_channels)
    fw = {f"flow.{k}": v for k, v in part("flow").items()}
    z_p = flow_forward(z, y_mask, fw, d, g=g_src)
    z_hat = V.flow_reverse(z_p, y_mask, _cast(fw, dtype), d, g=g_tgt)
    c = net.dec._cfg
    o_hat = generator(part("dec"), z_hat * y_mask, g_tgt, c["upsample_rates"], len(c["resblock_kernel_sizes"]), c["resblock_kernel_sizes"],
                      c["resblock_dilation_sizes"])
    return o_hat, y_mask, (z, z_p, z_hat)


class VcNet(nn.Module):
    """The voice-conversion half of SynthesizerTrn (models.py:1159-1212) built from the drop-ins: enc_q, flow, dec, emb_g."""

    def __init__(self, d, n_speakers, gin_channels):
        super().__init__()
        import torch_tts_amd as T

        Vm = T.vits2
        self.n_speakers = n_speakers
        self.enc_q = Vm.PosteriorEncoder(d["spec_channels"], d["inter_channels"], d["hidden_channels"], 5, 1, 16, gin_channels=gin_channels)
        self.dec = Vm.Generator(d["inter_channels"], d["resblock"], d["resblock_kernel_sizes"], d["resblock_dilation_sizes"], d["upsample_rates"],
                                d["upsample_initial_channel"], d["upsample_kernel_sizes"], gin_channels=gin_channels)
        self.flow = Vm.ResidualCouplingTransformersBlock(d["inter_channels"], d["hidden_channels"], 5, 1, 4, gin_channels=gin_channels,
                                                         use_transformer_flows=True, transformer_flow_type="pre_conv")
        if n_speakers > 1:
            self.emb_g = nn.Embedding(n_speakers, gin_channels)


def vc_net(meta):
    """The drop-in model of the vc fixture, its weights redrawn and checked against the recorded checksums."""
    c = meta["vc"]
    net = VcNet(meta["net"], c["n_speakers"], c["gin_channels"])
    for part, seed in c["seeds"].items():
        randomize(getattr(net, part), seed)
    for part, want in c["checksums"].items():
        vs = [v.double() for v in getattr(net, part).state_dict().values()]
        got = [len(vs), sum(v.numel() for v in vs), float(sum(v.sum() for v in vs)), float(sum(v.abs().sum() for v in vs)),
               float(sum((i + 1) * v.sum() for i, v in enumerate(vs)))]
        assert got[:2] == want[:2] and all(abs(a - b) <= 1e-9 * max(1.0, abs(want[3]) * len(vs)) for a, b in zip(got[2:], want[2:])), part
    return net.eval()


def _rel(a, b):
    return float(((a.double() - b.double()).abs() / (1e-5 / 1e-4 + b.double().abs())).max())


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_reference_posterior_encoder():
    sd, meta = load_golden()
    p = meta["post"]
    for S in p["spec"]:
        for gin in p["gin"]:
            g = sd["post/g8"] if gin else None
            got = posterior_encoder(weights(sd, f"post{S}_{gin}"), sd[f"post{S}/y"].double(), sd[f"post{S}/lengths"], g, sd["post/noise"],
                                    p["n_layers"], p["kernel"])
            for name, a in zip(("z", "m", "logs", "x_mask"), got):
                ref = sd[f"post{S}_{gin}/{name}"]
                assert _rel(a, ref) < 1e-5, (S, gin, name, _rel(a, ref))
            # padded frames are zero in the reference; y is not (the reference masks after pre)
            assert float(sd[f"post{S}_{gin}/z"][2, :, 1:].abs().max()) == 0.0 and float(sd[f"post{S}/y"][2, :, 1:].abs().max()) > 0


def test_restatement_reproduces_reference_flow_forward():
    sd, meta = load_golden()
    f = meta["flow"]
    d = flow_dims(f["channels"], f["hidden"], f["kernel"], f["n_layers"], f["n_flows"], f["gin"])
    wts = {f"flow.{k}": v for k, v in weights(sd, "flow").items()}
    got = flow_forward(sd["flow/x"].double(), sd["flow/x_mask"].double(), wts, d, g=sd["flow/g"].double())
    assert _rel(got, sd["flow/out"]) < 1e-5
    # the direction matters: the reverse pass of the same weights does not reproduce it, and undoes it
    back = V.flow_reverse(got, sd["flow/x_mask"].double(), _cast(wts, torch.float64), d, g=sd["flow/g"].double())
    assert _rel(back, sd["flow/x"]) < 1e-9
    assert _rel(V.flow_reverse(sd["flow/x"].double(), sd["flow/x_mask"].double(), _cast(wts, torch.float64), d, g=sd["flow/g"].double()),
                sd["flow/out"]) > 1e-2


def test_restatement_reproduces_reference_voice_conversion():
    sd, meta = load_golden()
    net = vc_net(meta)
    o_hat, y_mask, (z, z_p, z_hat) = voice_conversion(net, sd["vc/y"], sd["vc/lengths"], sd["vc/sid_src"], sd["vc/sid_tgt"], sd["vc/noise"])
    # (fp64 against the reference's fp32 run: through 16 WN layers and two passes of the flow the reference's own rounding reaches
    # ~1.2e-5 of the values - the 1e-4 bar of the GPU tests, with room)
    for name, a in dict(o_hat=o_hat, y_mask=y_mask, z=z, z_p=z_p, z_hat=z_hat).items():
        assert _rel(a, sd[f"vc/{name}"]) < 1e-4, (name, _rel(a, sd[f"vc/{name}"]))


def test_posterior_encoder_state_dict_matches_reference():
    import torch_tts_amd as T

    _, meta = load_golden()
    pe = T.vits2.PosteriorEncoder(80, 192, 192, 5, 1, 16, gin_channels=256)
    assert [[k, list(v.shape)] for k, v in pe.state_dict().items()] == meta["fulldims_post_state_dict"]
    assert pe.precision == "f32"
    with pytest.raises(NotImplementedError):
        T.vits2.PosteriorEncoder(80, 192, 192, 5, 2, 16)  # dilated WN


def test_ttspost_symbols_exported_and_tensor_count_matches_header():
    from torch_tts_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ttsdec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ttspost_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.POST_SYMBOLS), declared ^ set(_lib.POST_SYMBOLS)
    assert "ttsvits_flow_forward" in _lib.SYMBOLS and not set(_lib.POST_SYMBOLS) & set(_lib.SYMBOLS)
    lib = _lib.load()
    for sym in _lib.POST_SYMBOLS + ("ttsvits_flow_forward",):
        assert hasattr(lib, sym), sym
    import torch_tts_amd as T

    for gin in (0, 256):
        d = _lib.PostDims(spec_channels=513, inter_channels=192, hidden_channels=192, kernel_size=5, n_layers=16, gin_channels=gin)
        h = C.c_void_p()
        assert lib.ttspost_create(C.byref(d), C.byref(h)) == _lib.OK
        pe = T.vits2.PosteriorEncoder(513, 192, 192, 5, 1, 16, gin_channels=gin)
        n = lib.ttspost_num_weight_tensors(h)
        assert n == len(pe.weight_tensors()) == 4 + 4 * 16 + (2 if gin else 0)
        assert lib.ttspost_packed_bytes(h) % 256 == 0 and lib.ttspost_workspace_bytes(h, 2, 13) > 0
        assert lib.ttspost_get_precision(h) == _lib.PREC_F32
        assert lib.ttspost_set_precision(h, 7) == _lib.ERR_INVALID_ARG
        # no blob bound yet: refused before anything is launched
        assert lib.ttspost_forward(h, 1, 1, None, 1, 13, 2, 13, 1, 1, 1, 256, 1 << 30, None) == _lib.ERR_NOT_BOUND
        lib.ttspost_destroy(h)
    for bad in (dict(n_layers=33), dict(kernel_size=4), dict(hidden_channels=190), dict(gin_channels=3), dict(spec_channels=0)):
        kw = dict(spec_channels=80, inter_channels=192, hidden_channels=192, kernel_size=5, n_layers=16, gin_channels=0)
        kw.update(bad)
        h = C.c_void_p()
        assert lib.ttspost_create(C.byref(_lib.PostDims(**kw)), C.byref(h)) == _lib.ERR_DIMS, bad


# (name, B, T) -> bytes of ttsvits_text_encoder / ttsvits_flow / ttspost workspaces, as the library reported them before the size
# functions became the carve routines' totals: the layouts may be rewritten, the reported sizes may not change
WORKSPACE_BYTES = [
    ("small", 1, 1, 5952, 7840, 3840),
    ("small", 2, 37, 150912, 127040, 68864),
    ("small", 3, 200, 1196800, 986880, 541440),
    ("small_g", 1, 1, 5952, 7840, 3840),
    ("small_g", 2, 37, 150912, 127040, 68864),
    ("small_g", 3, 200, 1196800, 986880, 541440),
    ("modelconfig", 1, 1, 22784, 25216, 40960),
    ("modelconfig", 2, 37, 1369344, 1152768, 1193984),
    ("modelconfig", 3, 200, 11067392, 9240320, 9349888),
    ("modelconfig_g", 1, 1, 22784, 25216, 40960),
    ("modelconfig_g", 2, 37, 1369344, 1152768, 1193984),
    ("modelconfig_g", 3, 200, 11067392, 9240320, 9349888),
]


def test_workspace_sizes_are_the_recorded_ones():
    import dataclasses

    from torch_tts_amd import _lib

    lib = _lib.load()
    vm = json.load(open(os.path.join(HERE, "golden", "vits2_meta.json")))
    vits = {"small": vm["dims"], "small_g": vm["dims_g"], "modelconfig": dataclasses.asdict(V.Vits2Dims()),
            "modelconfig_g": dataclasses.asdict(V.Vits2Dims(gin_channels=256))}
    small_post = dict(inter_channels=8, hidden_channels=16, kernel_size=5, n_layers=3)  # vc_meta.json "post"
    full_post = dict(spec_channels=513, inter_channels=192, hidden_channels=192, kernel_size=5, n_layers=16)
    post = {"small": dict(small_post, spec_channels=13, gin_channels=0), "small_g": dict(small_post, spec_channels=16, gin_channels=8),
            "modelconfig": dict(full_post, gin_channels=0), "modelconfig_g": dict(full_post, gin_channels=256)}
    handles = {}
    for name in vits:
        d = dict(dict(gin_channels=0, cond_layer_idx=0), **vits[name])
        hv, hp = C.c_void_p(), C.c_void_p()
        assert lib.ttsvits_create(C.byref(_lib.VitsDims(*[int(d[n]) for n, _ in _lib.VitsDims._fields_])), C.byref(hv)) == _lib.OK
        assert lib.ttspost_create(C.byref(_lib.PostDims(**post[name])), C.byref(hp)) == _lib.OK
        handles[name] = (hv, hp)
    for name, B, T, te, fl, po in WORKSPACE_BYTES:
        hv, hp = handles[name]
        got = (lib.ttsvits_text_encoder_workspace_bytes(hv, B, T), lib.ttsvits_flow_workspace_bytes(hv, B, T), lib.ttspost_workspace_bytes(hp, B, T))
        assert got == (te, fl, po), (name, B, T, got)
    for hv, hp in handles.values():
        assert lib.ttsvits_text_encoder_workspace_bytes(hv, 0, 5) == 0 and lib.ttsvits_flow_workspace_bytes(hv, 2, 0) == 0
        assert lib.ttspost_workspace_bytes(hp, -1, 5) == 0
        lib.ttsvits_destroy(hv)
        lib.ttspost_destroy(hp)


def test_voice_conversion_refuses_what_is_not_on_the_path():
    import torch_tts_amd as T

    _, meta = load_golden()
    net = VcNet(meta["net"], 3, 4)
    y, lengths, sid = torch.zeros(1, 16, 5), torch.tensor([5]), torch.tensor([0])
    real_dec = net.dec
    net.dec = nn.Identity()
    with pytest.raises(TypeError):
        T.vits2.voice_conversion(net, y, lengths, sid, sid)
    net.dec = real_dec
    net.n_speakers = 0
    with pytest.raises(AssertionError):
        T.vits2.voice_conversion(net, y, lengths, sid, sid)
    # a model without the attribute (the reference's SynthesizerTrn never stores it) and without emb_g has no speakers either
    del net.n_speakers
    del net.emb_g
    with pytest.raises(AssertionError):
        T.vits2.voice_conversion(net, y, lengths, sid, sid)
    # the forward direction of the flow module keeps refusing forward(reverse=False): it is forward_cl
    fl = net.flow
    with torch.no_grad(), pytest.raises(NotImplementedError, match="forward_cl"):
        fl(torch.zeros(1, 16, 5), torch.ones(1, 1, 5), reverse=False)
