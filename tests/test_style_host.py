"""The style encoders (torch-tts_amd/style.py) without a GPU: state-dict compatibility with the reference, the pack order against
the header's enum, ``_stock_forward`` against the reference's recorded outputs (tests/golden/make_golden_style.py), the condition
the GPU tests' bar rests on (fp32 against fp64 on the fixture's own inputs), ``build_tacotron`` with a style encoder, and the
host-only part of the C ABI.  Also holds what tests/test_style_hip.py shares: the fixture loader and the error measure."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import torch_tts_amd as T
from torch_tts_amd import _lib
from torch_tts_amd import style as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL, ATOL = 1e-4, 1e-5  # the project's parity bar (tests/test_hip_parity.py)
CASES = ("enc", "gst", "gstvae", "vae")


def bar_ratio(got, ref):
    """max |got - ref| / (ATOL + RTOL |ref|): <= 1 is inside the parity bar."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "style_small.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "style_meta.json")))
    t = {k: torch.from_numpy(z[k].astype(np.float32) if z[k].dtype == np.float16 else z[k]) for k in z.files}
    return t, meta


def weights_of(case):
    t, _ = fixture()
    p = case + "/w/"
    return {k[len(p):]: v for k, v in t.items() if k.startswith(p)}


def make_module(case, dtype=torch.float32):
    """The drop-in of one fixture case with the reference's recorded weights, in eval mode on the CPU."""
    _, meta = fixture()
    s = meta["small"]
    small = dict(num_mels=s["num_mels"], dim_out=s["dim_out"], ref_enc_filters=s["ref_enc_filters"])
    if case == "enc":
        m = S.ReferenceEncoder(**small)
    elif case == "vae":
        m = S.VAE(num_mels=80, dim_vae=16)
    else:
        cls = S.GST if case == "gst" else S.GST_VAE
        kw = dict(num_mels=s["num_mels"], dim_emb=s["dim_emb"], dim_enc=s["dim_out"], num_tokens=s["num_tokens"], num_heads=s["num_heads"])
        if case == "gstvae":
            kw["dim_vae"] = s["dim_vae"]
        m = cls(**kw)
        m.encoder = S.ReferenceEncoder(**small)  # (as the fixture's generator does with the reference's module)
    missing, unexpected = m.load_state_dict(weights_of(case), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def case_inputs(case):
    """(x, lengths, eps or None) of a fixture case."""
    t, _ = fixture()
    if case == "vae":
        return t["vae/x_in"], t["vae/lengths"], t["vae/eps"]
    return t["x"], t["lengths"], t.get(case + "/eps")


def stock_outputs(m, x, lengths, eps=None):
    """{"enc_out", "x", "kl"} (those the module has) of _stock_forward in the module's own dtype, on the module's device."""
    dt = next(m.parameters()).dtype
    x = x.to(dt)
    with torch.no_grad():
        if isinstance(m, S.ReferenceEncoder):
            return {"enc_out": m._stock_forward(x, lengths)}
        out = {"enc_out": m.encoder._stock_forward(x, lengths)}
        xo, extra = m._stock_forward(x, lengths, None if eps is None else eps.to(dt))
        out["x"] = xo
        if "kl" in extra:
            out["kl"] = extra["kl"]
        return out


def test_state_dict_keys_and_shapes_are_the_references():
    _, meta = fixture()
    for case in CASES:
        m = make_module(case)
        got = {k: list(v.shape) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
        assert got == meta["keys"][case], case
    # the constructor defaults are the reference's too (style.py:22, 84, 113, 126, 156)
    assert [c.out_channels for c in S.ReferenceEncoder().convs] == [32, 32, 64, 64, 128, 128] and S.ReferenceEncoder().gru.input_size == 256
    assert S.STL().embed.shape == (10, 64) and S.GST_VAE().mean_linear.in_features == 256 and S.VAE().fc_out.weight.shape == (256, 16)


def test_pack_order_is_the_headers_enum():
    hdr = open(os.path.join(ROOT, "include", "ttsdec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = re.findall(r"\bTTSENC_STYLE_W_([A-Z_0-9]+)\b\s*(?:=\s*0\s*)?,?", hdr)
    head = names[:names.index("STAGES")]
    stage = names[names.index("STAGES") + 1:names.index("PER_STAGE")]
    key_of = {"LSTM_IH": "encoder.gru.weight_ih_l0", "LSTM_HH": "encoder.gru.weight_hh_l0", "LSTM_BIH": "encoder.gru.bias_ih_l0",
              "LSTM_BHH": "encoder.gru.bias_hh_l0", "MEAN_W": "mean_linear.weight", "MEAN_B": "mean_linear.bias",
              "LOGVAR_W": "logvar_linear.weight", "LOGVAR_B": "logvar_linear.bias", "FC_OUT": "fc_out.weight", "EMBED": "stl.embed",
              "QUERY": "stl.attention.W_query.weight", "KEY": "stl.attention.W_key.weight", "VALUE": "stl.attention.W_value.weight"}
    stage_of = {"CONV_W": "encoder.convs.{i}.weight", "CONV_B": "encoder.convs.{i}.bias", "BN_W": "encoder.bns.{i}.weight",
                "BN_B": "encoder.bns.{i}.bias", "BN_MEAN": "encoder.bns.{i}.running_mean", "BN_VAR": "encoder.bns.{i}.running_var"}
    assert len(head) == _lib.STYLE_W_STAGES == 13 and len(stage) == _lib.STYLE_W_PER_STAGE == 6
    for case in CASES:
        m = make_module(case)
        K = len(m._ref_encoder().convs)
        want = [key_of[n] for n in head] + [stage_of[n].format(i=i) for i in range(K) for n in stage]
        assert m.weight_names() == want, case
        sd = m.state_dict()
        pre = "encoder." if case == "enc" else ""
        for name, t in zip(want, m.weight_tensors()):
            key = name[len(pre):] if name.startswith(pre) and pre else name
            have = key in sd and not (case == "enc" and not name.startswith("encoder."))
            assert (t is not None) == have, (case, name)
            if t is not None:
                assert t.data_ptr() == sd[key].data_ptr(), (case, name)
        assert StyleEngineNoGpu(m).num_weight_tensors() == len(want)


def StyleEngineNoGpu(m):
    return S.StyleEngine(m.style_dims(), None)


@pytest.mark.parametrize("case", CASES)
def test_stock_forward_reproduces_the_reference(case):
    t, _ = fixture()
    m = make_module(case)
    x, lengths, eps = case_inputs(case)
    got = stock_outputs(m, x, lengths, eps)
    for name, v in got.items():
        r = bar_ratio(v, t[f"{case}/{name}"])
        print(f"{case}/{name}: stock fp32 vs reference {r:.4f} of the bar")
        assert r <= 1.0, (case, name, r)
    if case == "enc":
        assert bar_ratio(m._stock_forward(x, None), t["enc/enc_out_nolen"]) <= 1.0
        assert bar_ratio(m(x, lengths.tolist()), t["enc/enc_out"]) <= 1.0  # forward on the CPU is the stock path; a list of lengths


@pytest.mark.parametrize("case", CASES)
def test_fp32_stays_within_a_quarter_of_the_bar_of_fp64(case):
    """The condition the GPU parity tests rest on, met by the fixture's choice of weights and inputs: the stock forward in fp32
    differs from itself in fp64 by at most a quarter of the bar on every output, and kl does not sit near zero, where its
    cancellation 1 + logvar - mean^2 - exp(logvar) would leave a relative bar nothing to hold on to."""
    x, lengths, eps = case_inputs(case)
    got32 = stock_outputs(make_module(case), x, lengths, eps)
    got64 = stock_outputs(make_module(case, torch.float64), x, lengths, eps)
    for name in got32:
        r = bar_ratio(got32[name], got64[name])
        print(f"{case}/{name}: fp32 vs fp64 {r:.4f} of the bar, mean |ref| {float(got64[name].abs().mean()):.4f}")
        assert r <= 0.25, (case, name, r)
    if "kl" in got64:
        assert float(got64["kl"].abs().min()) > 1e-2


def _config(style=True):
    cfg = {
        "text": {"alphabet": "abcdefgh"},
        "audio": {"num_mels": 20},
        "model": {
            "encoder": {"dim_emb": 16, "dim_out": 256},  # (VAE's dim_emb is 256: the embedding is added to `memory`)
            "decoder": {"type": "tacotron2prod", "r": 1, "dim_pre": 32, "dim_att": 64, "dim_rnn": [64, 48]},
        },
    }
    if style:
        cfg["model"]["style_encoder"] = {"dim_vae": 8}
    return cfg


def test_build_tacotron_with_a_style_encoder():
    torch.manual_seed(3)
    model = T.build_tacotron(_config()).eval()
    assert isinstance(model.refencoder, T.VAE) and model.refencoder.fc_out.weight.shape == (256, 8)
    assert model.refencoder.encoder.num_mels == 20 and model.refencoder.encoder.gru.input_size == 128 * 1
    assert T.build_tacotron(_config(style=False)).refencoder is None
    # forward on the CPU with the decoder stubbed out: what reaches it is memory + style embedding
    seen = {}

    def fake_decoder(memory, mmask, x, max_steps, p_no_forcing=None):
        seen["memory"] = memory
        B = memory.shape[0]
        return torch.zeros(B, 2, 20), torch.zeros(B, 2), torch.zeros(B, 2, memory.shape[1])

    model.decoder.forward = fake_decoder
    ids = torch.tensor([[1, 2, 3, 4, 5], [3, 2, 1, 0, 0]])
    lens = torch.tensor([5, 3])
    xref = torch.randn(2, 70, 20)
    with torch.no_grad():
        plain = model.encoder(ids, lens)
        torch.manual_seed(11)
        embed, extra = model.refencoder(xref, torch.tensor([70, 40]))
        torch.manual_seed(11)  # (the same eps draw)
        y, y_post, s, out = model(ids, lens, xref=xref, xref_lengths=torch.tensor([70, 40]), max_steps=2)
    assert embed.shape == (2, 1, 256) and float(embed.abs().max()) > 0
    assert torch.equal(seen["memory"], plain + embed)
    assert out["kl_loss"].ndim == 0 and bool(torch.isfinite(out["kl_loss"])) and torch.equal(out["kl_loss"], extra["kl"].mean())
    with torch.no_grad():  # without xref the style encoder stays out of it
        model(ids, lens, max_steps=2)
    assert torch.equal(seen["memory"], plain)


def test_training_mode_is_differentiable_and_uses_batch_statistics():
    m = make_module("gstvae").train()
    x, lengths, eps = case_inputs("gstvae")
    before = m.encoder.bns[0].running_mean.clone()
    xo, extra = m(x, lengths, eps)
    (xo.sum() + extra["kl"].sum()).backward()
    assert m.encoder.convs[0].weight.grad is not None and float(m.encoder.convs[0].weight.grad.abs().sum()) > 0
    assert m.stl.embed.grad is not None and not torch.equal(m.encoder.bns[0].running_mean, before)


def test_host_length_above_T_raises():
    m = make_module("enc")
    x, _, _ = case_inputs("enc")
    with pytest.raises(ValueError):
        m(x, torch.tensor([201, 5, 5, 5, 5]))
    with pytest.raises(ValueError):
        m(x, [200, 5, 5, 5, 300])


def _dims(**kw):
    d = dict(n_mels=80, filters=(32, 32, 64, 64, 128, 128), d_enc=128, kind=_lib.STYLE_VAE, d_emb=256, d_vae=16, n_tokens=0, n_heads=0, bn_eps=1e-5)
    d.update(kw)
    return d


def test_dims_the_library_does_not_build():
    for bad in (dict(filters=(32, 30, 64)), dict(d_enc=126), dict(kind=_lib.STYLE_GST, n_tokens=10, n_heads=3, d_emb=256),
                dict(filters=(4,) * 9), dict(kind=7), dict(d_vae=0), dict(n_mels=0)):
        with pytest.raises(_lib.DimsNotBuilt):
            S.StyleEngine(_dims(**bad), None)
    # the module sees the same rule: it keeps the stock path instead of raising
    assert not S.ReferenceEncoder(num_mels=20, dim_out=16, ref_enc_filters=[4, 6])._dims_built()
    assert S.VAE()._dims_built() and S.GST()._dims_built() and S.GST_VAE()._dims_built()


def test_host_only_queries():
    e = S.StyleEngine(_dims(), None)
    assert e.num_weight_tensors() == 13 + 6 * 6
    n_w = 494080  # the VAE's parameters and BatchNorm buffers (style_meta.json vae_weights)
    assert fixture()[1]["vae_weights"] == n_w
    # + (alpha, beta) in place of the four BatchNorm vectors, b_ih + b_hh in place of the two: fewer floats, each tensor padded to 256 bytes
    assert 4 * (n_w - 6 * 128 * 3) < e.packed_bytes() < 4 * n_w + 60 * 256 and e.packed_bytes() % 256 == 0
    sizes = {(B, T_): e.workspace_bytes(B, T_) for B in (1, 2, 64) for T_ in (1, 130, 600)}
    assert all(v > 0 and v % 256 == 0 for v in sizes.values())
    assert sizes[(1, 1)] < sizes[(1, 130)] < sizes[(1, 600)] < sizes[(2, 600)] < sizes[(64, 600)]
    # the two activation buffers dominate: stage 0's output [B, 300, 40, 32] and stage 1's [B, 150, 20, 32]
    assert sizes[(64, 600)] >= 4 * 64 * (300 * 40 * 32 + 150 * 20 * 32)
    assert e.workspace_bytes(0, 600) == 0 and e.workspace_bytes(4, 0) == 0
    g = S.StyleEngine(_dims(kind=_lib.STYLE_GST_VAE, n_tokens=10, n_heads=4, d_vae=32), None)
    assert g.packed_bytes() > e.packed_bytes()


def test_unbound_handle_and_argument_checks_come_before_any_launch():
    lib = _lib.load()
    e = S.StyleEngine(_dims(), None)
    p = C.c_void_p(256)  # never dereferenced: every refusal below comes before the first launch
    fwd = lambda **kw: lib.ttsenc_style_forward(*[{**dict(h=e._h, x=p, ldx=80, lengths=None, eps=p, B=2, T=130, enc=p, xo=p, kl=p, ws=p, n=1 << 40, st=None), **kw}[k]  # noqa: E731
                                                  for k in ("h", "x", "ldx", "lengths", "eps", "B", "T", "enc", "xo", "kl", "ws", "n", "st")])
    assert fwd() == _lib.ERR_NOT_BOUND
    for bad in (dict(h=None), dict(x=None), dict(enc=None), dict(ws=None), dict(B=0), dict(T=0), dict(ldx=79), dict(eps=None), dict(xo=None), dict(kl=None)):
        assert fwd(**bad) == _lib.ERR_INVALID_ARG, bad
    assert lib.ttsenc_style_bind_weights(e._h, None) == _lib.ERR_INVALID_ARG
    assert lib.ttsenc_style_pack_weights(e._h, None, 49, p, None) == _lib.ERR_INVALID_ARG
    arr = (C.c_void_p * 49)()
    assert lib.ttsenc_style_pack_weights(e._h, arr, 48, p, None) == _lib.ERR_INVALID_ARG  # the tensor count
    assert lib.ttsenc_style_pack_weights(e._h, arr, 49, p, None) == _lib.ERR_INVALID_ARG  # NULL where this kind has a tensor
    assert lib.ttsenc_style_last_hip_error(e._h) == b""
    for sym in _lib.FAMILY_SYMBOLS["ttsenc"]:
        assert hasattr(lib, sym), sym
    assert sum(s.startswith("ttsenc_style_") for s in _lib.FAMILY_SYMBOLS["ttsenc"]) == 9
