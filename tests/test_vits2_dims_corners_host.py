"""Host-side checks of the dims corners of tests/vits2_dims_corner_cases.py (the text encoder, the coupling flow in both directions,
the posterior encoder): the fp64 restatements - the oracles of tests/test_vits2_dims_corners_hip.py - against the reference's own
outputs at these dims (tests/golden/make_golden_vits2_dims_corners.py) within half of the bar the kernels are held to, so the bar
judges the kernels and not the case; that each case still sits on the corner its comment names; that ttsvits_create / ttspost_create
accept every case and refuse a head wider than 256, at create and not in the middle of a call.  No GPU needed."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import vits2_dims_corner_cases as K
from torch_tts_amd import _lib, vits2

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-4, 1e-5  # the bar of tests/test_vits2_hip.py and tests/test_vc_hip.py against fp64
RATIO_MAX = 0.5
MAKE = {"te": K.make_text_encoder, "flow": K.make_flow, "post": K.make_post}
INPUTS = {"te": K.te_inputs, "flow": K.flow_inputs, "post": K.post_inputs}
REF64 = {"te": K.te_ref64, "flow": K.flow_ref64, "post": K.post_ref64}
OUTPUTS = {"te": ("x", "m", "logs"), "flow": ("rev", "fwd"), "post": ("z", "m", "logs")}
CASES = [(fam, name) for fam, table in K.FAMILIES.items() for name in table]
IDS = [name for _, name in CASES]


@functools.lru_cache(maxsize=None)
def load_golden():
    z = np.load(os.path.join(HERE, "golden", "vits2_dims_corners.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "vits2_dims_corners_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def state(mod):
    return {k: v.detach().clone().cpu() for k, v in mod.state_dict().items()}


def ratio_close(a, b):
    """a against the fp64 b as a fraction of the rtol / atol bar (make_golden_vits2_dims_corners.ratio_close)."""
    return float(((a.double() - b.double()).abs() / (ATOL + RTOL * b.double().abs())).max())


def stored(name, t):
    """t as the golden file holds a case's output: whole, or the big cases' elements at the stride"""
    return t.reshape(-1)[::K.STRIDE] if name in K.BIG else t


@functools.lru_cache(maxsize=None)
def refs(fam, name):
    """-> the case's inputs and the fp64 restatement of its outputs on the drop-in's seeded state dict, computed once"""
    i = INPUTS[fam](name)
    return i, dict(zip(OUTPUTS[fam], REF64[fam](name, state(MAKE[fam](vits2, name)), i)))


def test_tables_are_the_recorded_ones():
    g, meta = load_golden()
    assert (meta["ratio_max"], meta["stride"], meta["big"], meta["n_vocab"], meta["window"]) == (RATIO_MAX, K.STRIDE, list(K.BIG), K.N_VOCAB, K.WINDOW)
    for fam, table in K.FAMILIES.items():
        assert {n: {k: c[k] for k in table[n]} for n, c in meta[fam].items()} == table, fam
        for name in table:  # the recorded operands are the table's recipe
            for k, v in INPUTS[fam](name).items():
                assert (v is None and f"{fam}/{name}/{k}" not in g) or torch.equal(v, g[f"{fam}/{name}/{k}"]), (name, k)
    assert K.layout({}) == (3, 37, [37, 18, 1]) and K.mask_of({})[:, 0].sum(1).long().tolist() == [37, 18, 1]
    assert [n for t in K.FAMILIES.values() for n, c in t.items() if K.layout(c) != K.layout({})] == ["E6", "F5", "Q5"]
    assert K.layout(K.TE_CASES["E6"]) == K.layout(K.FLOW_CASES["F5"]) == (3, 9, [9, 4, 1]) and K.layout(K.POST_CASES["Q5"]) == (2, 19, [19, 8])
    assert os.path.getsize(os.path.join(HERE, "golden", "vits2_dims_corners.npz")) <= os.path.getsize(os.path.join(HERE, "golden", "dims_corners.npz"))


@pytest.mark.parametrize("fam,name", CASES, ids=IDS)
def test_restatement_matches_the_reference(fam, name):
    """The fp64 restatement on the drop-in's state dict against the reference's fp32 outputs: within half the bar, and the very
    ratio the golden script measured (both are fp32-against-fp64 differences; the fp64 side's own rounding moves them by far less
    than a percent).  Padded frames are exactly zero on both sides."""
    g, meta = load_golden()
    rec, c = meta[fam][name], K.FAMILIES[fam][name]
    mod = MAKE[fam](vits2, name)
    assert len(mod.state_dict()) == rec["n_tensors"]
    _, ref = refs(fam, name)
    _, _, lengths = K.layout(c)
    assert rec["ratio"] == max(rec["ratios"].values()) <= RATIO_MAX
    for k in OUTPUTS[fam]:
        got, want = g[f"{fam}/{name}/{k}"], stored(name, ref[k])
        assert list(ref[k].shape) == rec["shapes"][k] and got.shape == want.shape, (name, k)
        r = ratio_close(got, want)
        assert r <= RATIO_MAX, (name, k, r)
        if name in K.BIG:  # the recorded ratio is over every element, the samples are a thirteenth of them
            assert r <= rec["ratios"][k] * (1 + 1e-3) + 1e-6, (name, k, r)
        else:
            assert r == pytest.approx(rec["ratios"][k], rel=1e-3, abs=1e-6), (name, k, r)
            assert float(got.abs().max()) == pytest.approx(rec["abs_max"][k], rel=1e-6)
        assert 0.2 < rec["abs_max"][k] < 16.0, (name, k)  # (neither faded nor blown up)
        for b, n in enumerate(lengths):
            assert float(ref[k][b, :, n:].abs().sum()) == 0.0 and bool((ref[k][b, :, :n] != 0).any()), (name, k, b)


def test_f4_without_flows_is_the_identity():
    g, _ = load_golden()
    assert torch.equal(g["flow/F4/rev"], g["flow/F4/z"]) and torch.equal(g["flow/F4/fwd"], g["flow/F4/z"])
    _, ref = refs("flow", "F4")
    assert torch.equal(ref["rev"], g["flow/F4/z"].double()) and torch.equal(ref["fwd"], g["flow/F4/z"].double())


def ln_tier(C):
    """launch_layernorm's template argument (csrc/vits2.hip)"""
    return 2 if C <= 128 else 4 if C <= 256 else 16


def test_every_case_sits_on_the_corner_it_names():
    """Asserted from the dims, so that an edit of a table cannot move a case off its corner unnoticed."""
    E, F, Q = K.TE_CASES, K.FLOW_CASES, K.POST_CASES
    short = min(K.LENGTHS[:2])  # the shortest utterance with more than one frame
    dk = lambda c: c["hidden"] // c["heads"]  # noqa: E731
    mfma = (96, 48, 16, 8)  # the head widths of the matrix-core attention (run_stack): every other one takes the scalar kernel
    for c in list(E.values()) + list(F.values()):
        assert c.get("hidden", 4) % 4 == 0 and c.get("channels", 8) % 8 == 0
    # E1: smallest of everything, first = last layer, one tap, dk 4 on the scalar kernel
    assert (E["E1"]["hidden"], E["E1"]["filter"], E["E1"]["inter"], E["E1"]["layers"], E["E1"]["kernel"]) == (4, 4, 4, 1, 1) and dk(E["E1"]) == 4
    # E2: exact conv_1 (K = C, C % 8 != 0) writes planes for a split conv_2 (K = F, F % 8 == 0); a 32-wide k tile straddles taps
    assert E["E2"]["hidden"] % 8 and not E["E2"]["filter"] % 8 and 32 % E["E2"]["hidden"] and E["E2"]["hidden"] < 32 and E["E2"]["kernel"] > 1
    assert dk(E["E2"]) not in mfma and E["E2"]["layers"] >= 2
    # E3: split conv_1, exact conv_2 on the fp32 f; cond at layer 0; proj's N = 2 inter with inter % 8 != 0; seven taps
    assert not E["E3"]["hidden"] % 8 and E["E3"]["filter"] % 8 and E["E3"]["gin"] and E["E3"]["cond"] == 0 and E["E3"]["inter"] % 8
    assert E["E3"]["kernel"] == 7 and E["E3"]["layers"] > 2 and dk(E["E3"]) in mfma  # (the one case on the matrix-core attention)
    # E4: kMaxLayers, cond at the last layer, Cin 12
    assert E["E4"]["layers"] == 12 and E["E4"]["cond"] == 11 and E["E4"]["gin"] and E["E4"]["hidden"] == E["E4"]["filter"] == 12
    # E5: no layers
    assert E["E5"]["layers"] == 0 and not E["E5"]["gin"]
    # E6: LayerNorm <16> at C = 1024, its edge and dims_ok's; dk exactly 256; nine taps over F = 8 and over every utterance
    assert E["E6"]["hidden"] == 1024 and ln_tier(1024) == 16 and dk(E["E6"]) == _lib.VITS_MAX_HEAD_WIDTH == 256
    assert E["E6"]["kernel"] == 9 >= K.layout(E["E6"])[1] and E["E6"]["filter"] == 8 and E["E6"]["layers"] == 1
    # E7: LayerNorm <4>, dk 80 on the scalar kernel
    assert ln_tier(E["E7"]["hidden"]) == 4 and dk(E["E7"]) == 80 and E["E7"]["layers"] == 1
    assert {ln_tier(c["hidden"]) for c in E.values()} == {2, 4, 16}
    assert {c["layers"] for c in E.values()} >= {0, 1, 12} and {c["kernel"] for c in E.values()} >= {1, 3, 5, 7, 9}
    # the flow's stack has C = half, two heads (the reference's constant)
    half = lambda c: c["channels"] // 2  # noqa: E731
    assert (half(F["F1"]), F["F1"]["hidden"], F["F1"]["kernel"], F["F1"]["wn_layers"], F["F1"]["flows"]) == (4, 4, 1, 1, 1)
    assert half(F["F2"]) == 12 and F["F2"]["hidden"] % 8 and F["F2"]["wn_layers"] == 8 and F["F2"]["flows"] % 2 and F["F2"]["gin"] and F["F2"]["kernel"] == 7
    assert F["F3"]["flows"] == 8 and F["F4"]["flows"] == 0
    assert half(F["F5"]) == 512 and ln_tier(512) == 16 and half(F["F5"]) // 2 == 256 and F["F5"]["flows"] == 1
    assert half(F["F6"]) == 20 and F["F6"]["kernel"] == 31 and F["F6"]["kernel"] // 2 < K.T and F["F6"]["kernel"] > short and F["F6"]["gin"]
    assert {c["flows"] for c in F.values()} >= {0, 1, 2, 3, 8} and {c["wn_layers"] for c in F.values()} >= {1, 8}
    assert all((half(c) // 2) not in (48, 32, 64, 16) for c in F.values())  # (no case on the flash kernel: test_vits2_attention_hip.py has it)
    # the posterior encoder
    assert (Q["Q1"]["spec"], Q["Q1"]["inter"], Q["Q1"]["hidden"], Q["Q1"]["kernel"], Q["Q1"]["layers"]) == (1, 4, 4, 1, 1)
    assert Q["Q2"]["spec"] % 2 and Q["Q2"]["spec"] < 8 and Q["Q2"]["kernel"] == 31 and Q["Q2"]["hidden"] % 8 and Q["Q2"]["gin"]
    assert Q["Q3"]["layers"] == 32 and Q["Q4"]["hidden"] == 260 and Q["Q4"]["hidden"] % 8
    assert (Q["Q5"]["spec"], Q["Q5"]["inter"], Q["Q5"]["gin"], Q["Q5"]["kernel"], Q["Q5"]["layers"]) == (513, 192, 256, 9, 2)


def engines():
    """-> (name, a host-only engine of the case's drop-in, the tensors its pack call passes, B, T)"""
    for fam, name in CASES:
        mod = MAKE[fam](vits2, name)
        eng = vits2.PostEngine(mod._cfg, None) if fam == "post" else vits2.VitsEngine(mod._dims(), None)
        yield fam, name, eng, mod.weight_tensors(), K.layout(K.FAMILIES[fam][name])[:2]


def test_create_accepts_every_case():
    """ttsvits_create / ttspost_create return OK (a Handle raises otherwise); the tensor counts are the modules' pack lists'; the
    workspaces of the case's B and T are positive in both precisions."""
    for fam, name, eng, tensors, (b, t) in engines():
        try:
            assert eng.num_weight_tensors() == len(tensors), name
            assert eng.packed_bytes() > 0 and eng.packed_bytes() % 256 == 0, name
            for prec in ("f32", "split_f16"):
                eng.set_precision(prec)
                assert eng.precision() == prec
                if fam == "post":
                    assert int(eng._lib.ttspost_workspace_bytes(eng._h, b, t)) > 0, name
                else:
                    fn = eng._lib.ttsvits_text_encoder_workspace_bytes if fam == "te" else eng._lib.ttsvits_flow_workspace_bytes
                    assert int(fn(eng._h, b, t)) > 0, name
        finally:
            eng.close()


def _vits_create(**over):
    d = dict(K.make_flow(vits2, "F5")._dims(), **over)
    h = C.c_void_p()
    rc = _lib.load().ttsvits_create(C.byref(_lib.VitsDims(*[int(d[n]) for n, _ in _lib.VitsDims._fields_])), C.byref(h))
    if h:
        _lib.load().ttsvits_destroy(h)
    return rc


def test_a_head_wider_than_256_is_refused_at_create():
    """run_stack cannot run a head of more than 256 columns.  The flow's transformer has two heads (the reference's constant), so
    inter_channels above 1024 used to pass ttsvits_create and be refused in the middle of ttsvits_flow_*, behind the mask and split
    kernels of the first coupling; the text encoder's own stack likewise behind its embedding kernel.  Now it is the create's
    return code - and 256 itself (F5, E6) stays accepted."""
    assert _vits_create() == _lib.OK                                              # F5: 1024 / 2 / 2 = 256
    assert _vits_create(inter_channels=1032) == _lib.ERR_DIMS                      # 516 / 2 = 258
    assert _vits_create(inter_channels=2048, flow_tf_heads=4) == _lib.OK            # 1024 / 4 = 256
    assert _vits_create(inter_channels=2048, flow_tf_heads=2) == _lib.ERR_DIMS
    assert _vits_create(inter_channels=2048, n_flows=0) == _lib.OK                  # no coupling layer: the flow runs no stack
    te = K.make_text_encoder(vits2, "E6")._dims()
    assert _vits_create(**te) == _lib.OK                                            # E6: 1024 / 4 = 256
    assert _vits_create(**dict(te, n_heads=2)) == _lib.ERR_DIMS                     # 512
    assert _vits_create(**dict(te, n_heads=2, n_layers=0)) == _lib.ERR_DIMS         # (the call runs - and refused - the stack's set-up whatever n_layers)
    assert _vits_create(**dict(te, hidden_channels=516, n_heads=2)) == _lib.ERR_DIMS
    assert _vits_create(**dict(te, hidden_channels=512, n_heads=2)) == _lib.OK
    # the drop-in's exception names the head width
    with pytest.raises(_lib.DimsNotBuilt, match=r"head width 258 \(516 channels / 2 heads\) of the flow"):
        vits2.VitsEngine(dict(K.make_flow(vits2, "F5")._dims(), inter_channels=1032), None)
    with pytest.raises(NotImplementedError, match=r"head width 512 \(1024 channels / 2 heads\) of the text encoder"):
        vits2.VitsEngine(dict(te, n_heads=2), None)
    with pytest.raises(_lib.DimsNotBuilt, match="not built in the HIP library"):  # every other refusal keeps its message
        vits2.VitsEngine(dict(te, filter_channels=6), None)
