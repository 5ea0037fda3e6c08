"""CPU tests of batched synthesis (per-utterance stop rule, Postnet with lengths): the C ABI is exported and bound, the Python
entry points refuse CPU tensors like their neighbours, and the decode cases the GPU tests run (ragged_cases.py) have, in the
oracle alone, the spread of stop steps that makes those tests mean something."""
import inspect

import pytest
import torch

import ragged_cases as R
import torch_tts_amd as T
from torch_tts_amd import _lib


def test_library_exports_and_binds_the_ragged_entry_points():
    lib = _lib.load()
    for sym in ("ttsdec_decode_each", "ttsdec_postnet_ragged", "ttsdec_zero_tail"):
        assert sym in _lib.FAMILY_SYMBOLS["ttsdec"], sym
        fn = getattr(lib, sym)
        assert fn.argtypes is not None and fn.restype is not None, sym
    # ttsdec_decode without check_stop, plus stop_steps in front of T_out; ttsdec_postnet plus lengths behind y
    own = _lib.FAMILIES[0].own
    dec, each = own["decode"][1], own["decode_each"][1]
    assert len(each) == len(dec) and each[:8] == dec[:8] and each[8:] == dec[9:18] + [_lib.vp] + dec[18:]
    post, ragged = own["postnet"][1], own["postnet_ragged"][1]
    assert ragged == post[:2] + [_lib.vp] + post[2:]


def test_python_surface_signatures():
    sig = inspect.signature(T.Decoder.forward_each)
    assert list(sig.parameters) == ["self", "memory", "mmask", "max_steps"] and sig.parameters["max_steps"].default == 0
    for cls in (T.MelPostnet, T.MelPostnet2):
        p = inspect.signature(cls.forward).parameters
        assert list(p) == ["self", "x", "lengths"] and p["lengths"].default is None
    p = inspect.signature(T.Tacotron.synthesize).parameters
    assert list(p) == ["self", "cond", "cond_lengths", "xref", "xref_lengths", "max_steps"]
    # Tacotron.forward is untouched
    assert list(inspect.signature(T.Tacotron.forward).parameters) == ["self", "cond", "cond_lengths", "x", "x_lengths", "xref",
                                                                     "xref_lengths", "max_steps"]


def test_cpu_tensors_are_refused():
    cell = T.Taco2ProdDecoderCell(16, 80, 1, [32, 32], dim_pre=128, dim_att=32)
    dec = T.Decoder(cell, 1, 80).eval()
    with pytest.raises(RuntimeError, match="HIP path only"):
        dec.forward_each(torch.zeros(2, 5, 16), None)
    for pn in (T.MelPostnet(80, 64, 5, 3).eval(), T.MelPostnet2(80, 64, 3).eval()):
        with pytest.raises(RuntimeError, match="HIP path only"):
            pn(torch.zeros(2, 7, 80), lengths=torch.tensor([7, 3]))
    cfg = {
        "text": {"alphabet": "abc"},
        "audio": {"num_mels": 80},
        "model": {"encoder": {"dim_emb": 16, "dim_out": 32},
                  "decoder": {"type": "tacotron2prod", "r": 1, "dim_pre": 128, "dim_att": 32, "dim_rnn": [32, 32]},
                  "postnet": {"type": "tacotron2", "dim_hidden": 64, "num_layers": 3}},
    }
    model = T.build_tacotron(cfg).eval()
    with pytest.raises(RuntimeError, match="HIP path only|ROCm device"):
        model.synthesize(torch.ones(2, 4, dtype=torch.long), torch.tensor([4, 3]))


def _cases():
    return [(f"prod r={r} d_pre={p}", lambda r=r, p=p: R.prod_case(r, p)) for r, p in R.DECODE_CASES] + [
        ("taco2", R.taco2_case), ("gemm projection", R.gemm_proj_case)]


@pytest.mark.parametrize("name,make", _cases(), ids=[n for n, _ in _cases()])
def test_the_decode_cases_spread_their_stop_steps(name, make):
    """The conditions of ragged_cases.conditions(), one by one, on the oracle's own run; and the cap threshold's."""
    c = make()
    assert c.s.shape == (R.B, R.T, c.dims.r) and c.w.shape == (R.B, R.T, R.L)
    conds = R.conditions(c.s, c.thr, c.dims.r)
    if c.dims.r == 2:
        assert any(k.startswith("r = 2") for k in conds)
    for what, ok in {**conds, **R.cap_conditions(c.s, c.thr_cap)}.items():
        assert ok, f"{name}: {what}"
    tb, fire = R.stop_steps(c.s, c.thr)
    print(f"{name}: threshold {c.thr:.6f}, stop steps {sorted(set(tb.tolist()))}, nearest logit "
          f"{float((c.s - c.thr).abs().min()):.2e} away; rows that fire again later: {R.recrossing_rows(fire, int(tb.max()))}")
    # restated without the helper: the first step below the threshold, row by row
    for b in (0, int(tb.argmax()), int(tb.argmin())):
        below = [t for t in range(R.T) if float(c.s[b, t].min()) < c.thr]
        assert below[0] == int(tb[b])
