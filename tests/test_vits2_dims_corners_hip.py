"""GPU parity at the corners of the dims that ttsvits_create and ttspost_create accept (tests/vits2_dims_corner_cases.py): every case
through torch_tts_amd.vits2.TextEncoder, ResidualCouplingTransformersBlock (reverse and forward_cl) and PosteriorEncoder, in exact fp32
and in split-fp16, against the fp64 restatements of oracle/vits2_oracle.py and tests/test_vc_host.py under the bar that
tests/test_vits2_hip.py and tests/test_vc_hip.py hold the ModelConfig dims to against fp64: rtol 1e-4 / atol 1e-5 on every element of
every output, padded frames exactly zero.  tests/test_vits2_dims_corners_host.py shows that the restatements are the reference at
these dims and that the reference's own fp32 is within half of the bar.

The worst fraction of the bar over a case's outputs, as measured on an MI355X (f32 / split_f16; every run prints them per output):
  E1 0.451 / 0.451 (four channels: every GEMM stays exact, and a LayerNorm over four values is ill-conditioned)   E2 0.043 / 0.062
  E3 0.079 / 0.062   E4 0.084 / 0.084   E5 0.008 / 0.010   E6 0.216 / 0.155   E7 0.081 / 0.079
  F1 0.004 / 0.004   F2 0.070 / 0.078   F3 0.037 / 0.063   F4 0 / 0 (the input's bits)   F5 0.027 / 0.014   F6 0.049 / 0.048
  Q1 0.002 / 0.006   Q2 0.021 / 0.026   Q3 0.034 / 0.054   Q4 0.033 / 0.030   Q5 0.038 / 0.035
No corner was wrong."""
import pytest
import torch

import vits2_dims_corner_cases as K
from hip_helpers import assert_workspace_fits
from test_vits2_dims_corners_host import ATOL, CASES, IDS, MAKE, OUTPUTS, RTOL, load_golden, refs, stored
from torch_tts_amd import _lib, vits2
from torch_tts_amd.engine import Handle

pytestmark = pytest.mark.gpu
PRECISIONS = ["f32", "split_f16"]
_built = {}  # (family, case) -> the drop-in on the GPU; (family, case, precision) -> its outputs on the whole batch


@pytest.fixture(scope="module", autouse=True)
def _drop_modules():
    yield
    _built.clear()


def once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def fraction(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(((a - b).abs() / (ATOL + RTOL * b.abs())).max())


def _close(a, b, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL, msg=lambda m: f"{what}: {m}")


def module(fam, name):
    return once((fam, name), lambda: MAKE[fam](vits2, name).cuda().eval())


def _dev(t):
    return None if t is None else t.cuda()


def run(fam, name, precision, rows=slice(None), n=None):
    """The case's outputs ([B, C, T], on the CPU) for the utterances `rows`, cut to their first n frames (None: the case's T)."""
    mod = module(fam, name)
    i, _ = refs(fam, name)
    n = K.layout(K.FAMILIES[fam][name])[1] if n is None else n
    lengths, g = torch.clamp(i["lengths"][rows], max=n).cuda(), _dev(None if i["g"] is None else i["g"][rows])
    mod.precision = precision
    try:
        with torch.no_grad():
            if fam == "te":
                x, m, logs, _ = mod(i["ids"][rows, :n].cuda(), lengths, g=g)
                out = dict(x=x, m=m, logs=logs)
            elif fam == "flow":
                z = i["z"][rows, :, :n].contiguous().cuda()
                mask = K.mask_of(K.FLOW_CASES[name])[rows, :, :n].contiguous().cuda()
                rev = mod(z, mask, g=g, reverse=True)
                fwd = mod.forward_cl(z.transpose(1, 2).contiguous(), lengths, g).transpose(1, 2)
                out = dict(rev=rev, fwd=fwd)
            else:
                z, m, logs, _ = mod(i["y"][rows, :, :n].contiguous().cuda(), lengths, g=g, noise=i["eps"][rows, :, :n].contiguous().cuda())
                out = dict(z=z, m=m, logs=logs)
        return {k: v.contiguous().cpu() for k, v in out.items()}
    finally:
        mod.precision = "f32"


def batch(fam, name, precision):
    return once((fam, name, precision), lambda: run(fam, name, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_parity_with_the_fp64_restatement(fam, name, precision):
    g, _ = load_golden()
    _, ref = refs(fam, name)
    out = batch(fam, name, precision)
    _, _, lengths = K.layout(K.FAMILIES[fam][name])
    worst = {k: fraction(out[k], ref[k]) for k in OUTPUTS[fam]}  # every figure before the first assertion
    print(f"{name} {precision}: worst |err| / (atol + rtol |ref|) = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; against the reference's fp32: {max(fraction(stored(name, out[k]), g[f'{fam}/{name}/{k}']) for k in OUTPUTS[fam]):.3f}")
    for k in OUTPUTS[fam]:
        _close(out[k], ref[k], f"{name} {precision} {k}")
        for b, n in enumerate(lengths):  # padded frames: exactly zero
            assert float(out[k][b, :, n:].abs().sum()) == 0.0, (name, precision, k, b)
    if name == "F4":  # no flows: the input, bit for bit, in both directions
        i, _ = refs(fam, name)
        assert torch.equal(out["rev"], i["z"]) and torch.equal(out["fwd"], i["z"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fam,name", [("te", "E2"), ("te", "E3"), ("flow", "F2"), ("post", "Q2")], ids=["E2", "E3", "F2", "Q2"])
def test_rows_alone_and_twice(fam, name, precision):
    """Each utterance alone, at its own length, gives the bits it has in the padded batch; a second call gives the first's bits."""
    out = batch(fam, name, precision)
    again = run(fam, name, precision)
    for k in OUTPUTS[fam]:
        assert torch.equal(out[k], again[k]), f"{name} {precision} {k}: two identical calls differ"
    for b, n in enumerate(K.layout(K.FAMILIES[fam][name])[2]):
        alone = run(fam, name, precision, slice(b, b + 1), n)
        for k in OUTPUTS[fam]:
            assert alone[k].shape[2] == n and torch.equal(alone[k][0], out[k][b, :, :n]), f"{name} {precision} {k}: utterance {b} depends on the batch"


@pytest.mark.parametrize("fam,name", [("te", "E2"), ("flow", "F2"), ("post", "Q2")], ids=["E2", "F2", "Q2"])
def test_workspace_fits_in_split_fp16(monkeypatch, fam, name):
    """The cases in which planes and fp32 buffers are both live (F2: in both directions): the reported bytes hold the call."""
    want = batch(fam, name, "split_f16")
    got = []

    def call():
        got.append(run(fam, name, "split_f16"))
        return torch.cat([got[-1][k].reshape(-1) for k in OUTPUTS[fam]]).cuda()

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, kind, nbytes: nbytes, call)
    for k in OUTPUTS[fam]:
        assert torch.equal(got[0][k], want[k]), f"{name} {k}: the result depends on the workspace"


@pytest.mark.parametrize("name", ["E2", "E3"])
def test_the_mixed_chain_really_runs_mixed(name):
    """E2 (conv_1 exact, conv_2 on planes) and E3 (the reverse) in split-fp16: had the mode fallen back as a whole, the two results
    would agree in every bit; both are within the bar (test_parity_with_the_fp64_restatement)."""
    a, b = batch("te", name, "split_f16"), batch("te", name, "f32")
    assert not torch.equal(a["x"], b["x"]) and not torch.equal(a["m"], b["m"])
    _, ref = refs("te", name)
    for k in OUTPUTS["te"]:
        _close(a[k], ref[k], f"{name} split_f16 {k}")
        _close(b[k], ref[k], f"{name} f32 {k}")


def test_a_head_wider_than_256_is_refused_before_any_launch():
    """channels = 1032: half 516 over the flow's two heads is a head of 258 columns.  The drop-in raises at its engine's create,
    naming the head width - in front of the weight pack and of every kernel of the call - and leaves no handle and no error text
    behind; F5 (256) runs (test_parity_with_the_fp64_restatement)."""
    fl = vits2.ResidualCouplingTransformersBlock(1032, 8, 3, 1, 1, n_flows=1, use_transformer_flows=True).cuda().eval()
    z, mask = torch.zeros(1, 1032, 5, device="cuda"), torch.ones(1, 1, 5, device="cuda")
    torch.cuda.synchronize()
    for call in (lambda: fl(z, mask, reverse=True), lambda: fl.forward_cl(z.transpose(1, 2).contiguous(), torch.tensor([5]).cuda())):
        with torch.no_grad(), pytest.raises(_lib.DimsNotBuilt, match=r"head width 258 \(516 channels / 2 heads\)") as e:
            call()
        assert isinstance(e.value, NotImplementedError) and e.value.code == _lib.ERR_DIMS
    assert not list(fl._engines.engines()), "a handle was created"
    assert _lib.load().ttsvits_last_hip_error(None) == b""
    torch.cuda.synchronize()  # (nothing was queued: nothing to fail here either)
