"""Host-side checks of the VITS2 validation step's glue (ttsvits_kl_loss / ttsvits_slice_segments / ttsvits_sliced_l1 and
vits2.synthesizer_forward / validation_losses): the fp64 restatements below - the oracle of tests/test_evalstep_hip.py - against the
reference's own fp64 records (tests/golden/make_golden_evalstep.py), the C ABI's sizes and refusals on a handle without a device,
rand_slice_segments' formula against the recorded draw, and the fixture's checksums.  No GPU needed."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from test_align_host import AlignNet
from test_duration_host import randomize
from test_durnll_host import mask_of, rel, same_checksum

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REL = 1e-4  # the project's bar: |a - b| / (0.1 + |b|)
MODELS = ("model_mel", "model_lin")
NEW_SYMBOLS = ("ttsvits_kl_loss_workspace_bytes", "ttsvits_kl_loss", "ttsvits_slice_segments", "ttsvits_sliced_l1")


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "evalstep_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "evalstep_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 restatements (layouts of the reference: [B, C, T])
# ---------------------------------------------------------------------------------------------------------------------------
def gather_prior(p, frame_token):
    """models.py:1270-1271 as a gather: p [B, C, T_x], frame_token [B, T_y] (-1: no token) -> [B, C, T_y], zeros where there is no
    token.  In p's dtype: a one-hot row times a column is that column's value exactly."""
    B, C, _ = p.shape
    ft = torch.as_tensor(frame_token).long()
    idx = ft.clamp(min=0)[:, None, :].expand(B, C, ft.shape[1])
    return torch.where((ft >= 0)[:, None, :], p.gather(2, idx), torch.zeros((), dtype=p.dtype))


def frame_token_of(attn, t_y):
    """attn [B, 1, T_y, T_x] 0 / 1 -> frame_token [B, T_y] int32, -1 at frames >= t_y[b] (what ttsvits_maximum_path writes)."""
    ft = attn[:, 0].argmax(2).to(torch.int32)
    ft[torch.arange(attn.shape[2])[None, :] >= torch.as_tensor(t_y)[:, None]] = -1
    return ft


def kl_restated(z_p, logs_q, m_p, logs_p, t_y, frame_token=None):
    """losses.kl_loss in fp64 on the unexpanded prior -> (kl_rows [B], kl_sum, kl = kl_sum / sum(t_y))."""
    z_p, logs_q, m_p, logs_p = (t.double() for t in (z_p, logs_q, m_p, logs_p))
    if frame_token is not None:
        m_p, logs_p = gather_prior(m_p, frame_token), gather_prior(logs_p, frame_token)
    t_y = torch.as_tensor(t_y)
    kl = (logs_p - logs_q - 0.5 + 0.5 * (z_p - m_p) ** 2 * torch.exp(-2.0 * logs_p)) * mask_of(t_y, z_p.shape[2]).double()
    rows = kl.sum([1, 2])
    return rows, rows.sum(), rows.sum() / float(t_y.sum())


def slice_restated(x, ids_str, segment_size):
    """commons.slice_segments' loop, restated."""
    ret = torch.zeros_like(x[:, :, :segment_size])
    for i in range(x.size(0)):
        s = int(ids_str[i])
        ret[i] = x[i, :, s:s + segment_size]
    return ret


def sliced_l1_restated(a, y, ids_str=None):
    """F.l1_loss(slice_segments(a, ids_str, seg), y) in fp64 -> (l1_rows [B], the mean)."""
    a, y = a.double(), y.double()
    if ids_str is not None:
        a = slice_restated(a, ids_str, y.shape[2])
    d = (a - y).abs()
    return d.sum([1, 2]), d.sum() / d.numel()


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture's model from the drop-ins
# ---------------------------------------------------------------------------------------------------------------------------
class EvalNet(AlignNet):
    """What vits2.synthesizer_forward reads of a SynthesizerTrn: AlignNet, the duration predictor, the generator and segment_size."""

    def __init__(self, d, use_sdp, n_speakers, gin_channels):
        super().__init__(d, n_speakers, gin_channels)
        import torch_tts_amd as T

        V = T.vits2
        self.segment_size = d["segment_size"]
        self.dp = (V.StochasticDurationPredictor(d["hidden_channels"], 192, 3, 0.5, 4, gin_channels=gin_channels) if use_sdp else
                   V.DurationPredictor(d["hidden_channels"], 256, 3, 0.5, gin_channels=gin_channels))
        self.dec = V.Generator(d["inter_channels"], d["resblock"], d["resblock_kernel_sizes"], d["resblock_dilation_sizes"], d["upsample_rates"],
                               d["upsample_initial_channel"], d["upsample_kernel_sizes"], gin_channels=gin_channels)


def eval_net(meta, name):
    """The drop-in model of the fixture, its weights redrawn with the recorded seeds and checked against the reference's sums."""
    c = meta["models"][name]
    net = EvalNet(dict(meta["net"], spec_channels=c["spec_channels"]), c["use_sdp"], c["n_speakers"], c["gin_channels"])
    assert sorted(c["seeds"]) == sorted(p for p in ("enc_p", "enc_q", "flow", "dp", "dec", "emb_g") if hasattr(net, p))
    for part, seed in c["seeds"].items():
        randomize(getattr(net, part), seed)
        if part == "enc_q":  # (make_golden_evalstep.py: the posterior's last conv is scaled to a trained model's range)
            with torch.no_grad():
                net.enc_q.proj.weight.mul_(meta["enc_q_proj_scale"])
                net.enc_q.proj.bias.mul_(meta["enc_q_proj_scale"])
        assert same_checksum(getattr(net, part), c["checksums"][part]), (name, part)
    return net.eval()


# ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import torch_tts_amd as T
    from torch_tts_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsvits"] and hasattr(lib, sym), sym
    for name in ("kl_loss", "slice_segments", "rand_slice_segments", "synthesizer_forward", "validation_losses", "validation_losses_from_audio"):
        assert callable(getattr(T.vits2, name)), name
    assert "evalstep.hip" in open(os.path.join(ROOT, "torch-tts_amd", "build.py")).read()


def test_refusals_come_before_any_launch():
    """Sizes, then pointers, then the workspace - on a handle without a device, where a call that passed every check answers
    TTSDEC_ERR_DEVICE instead of launching."""
    import torch_tts_amd as T
    from torch_tts_amd import _lib

    lib = _lib.load()
    eng = T.vits2.VitsEngine(T.vits2._ALIGN_DIMS, None)
    h, one, big = eng._h, 256, 1 << 30  # (non-null, aligned placeholders: nothing is dereferenced)
    INV, DIMS, WS, DEV = _lib.ERR_INVALID_ARG, _lib.ERR_DIMS, _lib.ERR_WORKSPACE, _lib.ERR_DEVICE
    assert lib.ttsvits_kl_loss_workspace_bytes(h, 64, 600) == 64 * 600 * 4
    assert lib.ttsvits_kl_loss_workspace_bytes(h, 3, 5) == 256 and lib.ttsvits_kl_loss_workspace_bytes(h, 0, 5) == 0
    assert lib.ttsvits_kl_loss_workspace_bytes(None, 1, 5) == 0 and lib.ttsvits_kl_loss_workspace_bytes(h, 1, -1) == 0

    def kl(B=2, Ty=10, Tx=4, C=8, z=one, lq=one, m=one, lp=one, ft=one, ty=one, rows=one, out=one, ws=one, nbytes=big, hh=h):
        return lib.ttsvits_kl_loss(hh, z, lq, m, lp, ft, ty, B, Ty, Tx, C, None, None, rows, out, ws, nbytes, None)

    assert kl() == DEV
    assert kl(hh=None) == INV
    for bad in (dict(B=0), dict(Ty=0), dict(Tx=-1), dict(C=0)):
        assert kl(**bad, z=None) == INV, bad  # (sizes before pointers: the NULL pointer is not what is reported for DIMS below)
    for bad in (dict(C=6), dict(C=2), dict(C=4100), dict(B=65536)):
        assert kl(**bad, z=None) == DIMS, bad
    for ptr in ("z", "lq", "m", "lp", "ty", "rows", "out"):
        assert kl(**{ptr: None}) == INV, ptr
    assert kl(z=260) == INV  # 4-byte aligned only
    assert kl(ft=None) == INV and kl(ft=None, Tx=10) == DEV  # the identity form needs T_x == T_y
    assert kl(ws=None) == WS and kl(nbytes=255) == WS and kl(ws=one + 16) == WS and kl(nbytes=256) == DEV
    assert kl(z=None, nbytes=0) == INV  # pointers before the workspace

    def sl(B=2, outer=3, T=10, inner=1, seg=4, scale=1, x=one, ids=one, out=one, status=one):
        return lib.ttsvits_slice_segments(h, x, ids, 1, B, outer, T, inner, seg, scale, out, status, None)

    assert sl() == DEV
    for bad in (dict(B=0), dict(outer=0), dict(T=0), dict(inner=0), dict(seg=0), dict(scale=0)):
        assert sl(**bad, x=None) == INV, bad
    assert sl(seg=11, x=None) == DIMS and sl(B=65536, x=None) == DIMS and sl(outer=1 << 20, T=1 << 20, x=None) == DIMS
    for ptr in ("x", "ids", "out", "status"):
        assert sl(**{ptr: None}) == INV, ptr

    def l1(B=2, C=3, Ta=10, seg=4, a=one, y=one, ids=one, rows=one, out=one, status=one):
        return lib.ttsvits_sliced_l1(h, a, y, ids, 1, B, C, Ta, seg, rows, out, status, None)

    assert l1() == DEV
    for bad in (dict(B=0), dict(C=0), dict(Ta=0), dict(seg=0)):
        assert l1(**bad, a=None) == INV, bad
    assert l1(seg=11, a=None) == DIMS and l1(B=65536, a=None) == DIMS
    for ptr in ("a", "y", "rows", "out", "status"):
        assert l1(**{ptr: None}) == INV, ptr
    assert l1(ids=None) == INV and l1(ids=None, seg=10) == DEV  # the plain form: one shape
    eng.close()


@pytest.mark.parametrize("name", MODELS)
def test_restatements_reproduce_the_reference_in_fp64(name):
    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    t_y, seg = k("y_lengths"), meta["net"]["segment_size"]
    ft = frame_token_of(k("attn"), t_y)
    attn = k("attn")[:, 0].double()
    for u, e in (("m_pu64", "m_p64"), ("logs_pu64", "logs_p64")):
        want = torch.matmul(attn, k(u).transpose(1, 2)).transpose(1, 2)  # the reference's line
        assert torch.equal(gather_prior(k(u), ft), want) and torch.equal(want, k(e)), u
    assert float((k("m_p").double() - k("m_p64")).abs().max()) < 1e-4  # (the fp32 record is the same expansion)
    rows, total, kl = kl_restated(k("z_p64"), k("logs_q64"), k("m_pu64"), k("logs_pu64"), t_y, ft)
    assert abs(float(kl) - float(k("loss_kl64"))) <= 1e-9 * max(1.0, abs(float(kl)))
    rows_i, total_i, kl_i = kl_restated(k("z_p64"), k("logs_q64"), k("m_p64"), k("logs_p64"), t_y)  # the identity form
    assert torch.equal(rows_i, rows) and float(kl_i) == float(kl) and abs(float(rows.sum()) - float(total)) <= 1e-9 * abs(float(total))
    ids = k("ids_slice")
    l1_rows, l1 = sliced_l1_restated(k("mel64"), k("y_hat_mel64"), ids)
    assert abs(float(l1) - float(k("loss_mel64"))) <= 1e-9 * max(1.0, abs(float(l1)))
    assert abs(float(l1_rows.sum()) / k("y_hat_mel64").numel() - float(l1)) <= 1e-12
    # the fp32 records: the slice, and the losses within the recorded yardstick
    mel32 = k("spec") if meta["models"][name]["spec_channels"] == meta["audio"]["n_mels"] else None
    if mel32 is not None:
        assert torch.equal(slice_restated(mel32, ids, seg), k("y_mel"))
    c = meta["models"][name]
    for loss in ("loss_mel", "loss_kl", "loss_dur"):
        assert rel(k(loss), k(loss + "64")) == pytest.approx(c["cpu_f32_err"][loss], rel=1e-6, abs=1e-12)
        assert c["cpu_f32_err"][loss] <= meta["yardstick_max"] == 2.5e-5 and 4 * meta["yardstick_max"] <= REL
    # every seed tried: [the three yardsticks, the fp64 search found the same path, the tensors' worst fraction of the bar]
    last = list(c["tried"].values())[-1]
    assert all(len(v) == 5 for v in c["tried"].values()) and last[3] is True and last[4] <= c["tol_ratio_max"] == 0.25
    assert max(c["cpu_f32_tol_ratio"].values()) == last[4]


@pytest.mark.parametrize("name", MODELS)
def test_rand_slice_formula_against_the_recorded_draw(name):
    import torch_tts_amd as T

    sd, meta = load_golden()
    k = lambda n: sd[f"{name}/{n}"]  # noqa: E731
    seg = meta["net"]["segment_size"]
    ids = T.vits2._draw_ids(4, k("y_lengths"), seg, torch.device("cpu"), k("u"))
    assert ids.dtype == torch.int64 and torch.equal(ids, k("ids_slice")) and ids.tolist() == meta["models"][name]["ids_slice"]
    assert int(ids[1]) == 0  # the utterance that is exactly one segment
    assert bool((ids >= 0).all()) and bool((ids <= k("y_lengths") - seg).all())
    # an utterance shorter than segment - 1 frames draws a negative start at u = 0.9
    assert T.vits2._draw_ids(1, torch.tensor([seg - 3]), seg, torch.device("cpu"), torch.tensor([0.9])).tolist() == [-1]


def test_fixture_checksums():
    sd, meta = load_golden()
    path = os.path.join(HERE, "golden", "evalstep_small.npz")
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == meta["npz_sha256"]
    assert os.path.getsize(path) < 1 << 20
    assert meta["audio"]["segment_size"] == meta["net"]["segment_size"] * meta["audio"]["hop_size"] == 128
    assert meta["y_lengths"][1] == meta["net"]["segment_size"] and meta["y_lengths"][0] == sd["model_mel/spec"].shape[2]
    assert sd["basis"].shape == (16, 129)
    for name in MODELS:
        eval_net(meta, name)  # asserts every part's checksum
        c = meta["models"][name]
        for loss, v in c["losses"].items():
            assert float(sd[f"{name}/{loss}"]) == pytest.approx(v, rel=1e-6)
    assert meta["models"]["model_mel"]["spec_channels"] == 16 and meta["models"]["model_lin"]["spec_channels"] == 129


def test_functions_refuse_what_is_not_on_the_path():
    import torch_tts_amd as T

    V = T.vits2
    a = torch.zeros(2, 4, 5)
    with pytest.raises(NotImplementedError):
        V.kl_loss(a, a, a, a, torch.ones(2, 1, 5))  # a CPU tensor
    with pytest.raises(NotImplementedError):
        V.slice_segments(a, torch.zeros(2, dtype=torch.long), 2)
    with pytest.raises(NotImplementedError):
        V.rand_slice_segments(a, torch.tensor([5, 4]), 2)
    with pytest.raises(TypeError):
        V.validation_losses(None, torch.nn.Identity(), None, None, a, None, a, n_fft=256, hop_size=8, win_size=256, sampling_rate=22050,
                            n_mels=16, segment_size=128)
