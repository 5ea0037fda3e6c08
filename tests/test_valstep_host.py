"""Host-side checks of the Tacotron validation step's loss terms (ttsdec_val_losses / ttsdec_mel_loss and tacotron.mel_loss_fn,
alignment_*_loss, stop_loss, validation_terms, run_validation_step, task_forward): the fp64 restatement of the term table below - the
oracle of tests/test_valstep_hip.py - against the reference's own fp64 records and its end-to-end record
(tests/golden/make_golden_valstep.py), the C ABI's sizes and refusals on a handle without a device, and the Python refusals.
No GPU needed."""
import hashlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REL = 1e-4  # the project's bar for the GPU tests: |a - b| <= REL |b| against the fp64 restatement
NEW_SYMBOLS = ("ttsdec_val_losses_workspace_bytes", "ttsdec_val_losses", "ttsdec_mel_loss")
NEW_FUNCTIONS = ("mel_loss_fn", "alignment_max_loss", "alignment_std_loss", "stop_loss", "validation_terms", "run_validation_step", "task_forward")
# terms[i] of ttsdec_val_losses -> the reference's record of make_golden_valstep.py
TERM_RECORDS = ("mel_o1_m", "melp_o1_m", "dmel_all", "dmelp_all", "dmel_m", "dmelp_m", "stop", "w_std", "w_max")


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "valstep_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "valstep_meta.json")))
    return {k: torch.from_numpy(z[k]) for k in z.files}, meta


def case_tensors(sd, name):
    return {k: sd[f"{name}/{k}"] for k in ("y", "y_post", "x", "s", "w", "lengths")}


# ---------------------------------------------------------------------------------------------------------------------------
# the term table of include/ttsdec.h ttsdec_val_losses, restated in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    return float("nan") if b == 0 else a / b


def restate(y, y_post, x, s, w, lengths, pos_weight=0.1):
    """-> (rows [B, 9], terms [16]) in fp64; an operand that is None leaves its entries zero.  lengths None: every frame counts."""
    ref = next(t for t in (y, s, w) if t is not None)
    B = ref.shape[0]
    rows, terms = torch.zeros(B, 9, dtype=torch.float64), [0.0] * 16
    T = y.shape[1] if y is not None else (s.shape[1] if s is not None else 1)
    ln = torch.full((B,), T, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).long().clamp(0, T)
    live = torch.arange(T)[None, :] < ln[:, None]  # [B, T]
    N, N1 = int(ln.sum()), int((ln - 1).clamp(min=0).sum())
    if y is not None:
        D = y.shape[2]
        xd = x[:, :T].double()
        for k, op in enumerate((y, y_post)):
            if op is None:
                continue
            e = (op.double() - xd).abs().sum(2)  # [B, T]
            d = ((op.double()[:, 1:] - op.double()[:, :-1]) - (xd[:, 1:] - xd[:, :-1])).abs().sum(2)  # [B, T - 1]
            rows[:, 0 + k] = (e * live).sum(1)
            rows[:, 2 + k] = d.sum(1)
            rows[:, 4 + k] = (d * live[:, 1:]).sum(1)
            terms[0 + k] = _div(float(rows[:, 0 + k].sum()), D * N)
            terms[2 + k] = _div(float(rows[:, 2 + k].sum()), B * (T - 1) * D)
            terms[4 + k] = _div(float(rows[:, 4 + k].sum()), D * N1)
    if s is not None:
        sv, z = s.double().reshape(B, T), live.double()
        sp = torch.log1p(torch.exp(-sv.abs())) + (-sv).clamp(min=0)
        rows[:, 6] = ((1 - z) * sv + (1 + (pos_weight - 1) * z) * sp).sum(1)
        terms[6] = float(rows[:, 6].sum()) / (B * T)
    if w is not None:
        wd = w.double()
        S, L = wd.shape[1:]
        pos = torch.arange(L, dtype=torch.float64)
        s0, m1 = wd.sum(2), (wd * pos).sum(2)
        var = (wd * (pos[None, None, :] - m1[:, :, None]) ** 2).sum(2) + m1 ** 2 * (1 - s0)
        rows[:, 7] = var.clamp(min=0).sum(1)
        rows[:, 8] = (1 - wd.max(2).values).sum(1)
        terms[7] = math.sqrt(float(rows[:, 7].sum()) / (B * S))
        terms[8] = float(rows[:, 8].sum()) / (B * S)
    terms[9], terms[10] = float(N), float(N1)
    return rows, terms


def mel_restated(y, x, lengths, order):
    """mel_loss_fn(y, x[:, :T], mask of lengths, order) in fp64 -> (rows [B], the value)."""
    B, T, D = y.shape
    d = y.double() - x[:, :T].double()
    if order == 0:
        vol = x[:, :T].double().mean(2, keepdim=True).clamp(min=0.1)
        el = torch.where(d > 0, vol * d, -d)
    else:
        el = d.abs() if order == 1 else d * d
    ln = torch.full((B,), T) if lengths is None else torch.as_tensor(lengths).long().clamp(0, T)
    rows = (el.sum(2) * (torch.arange(T)[None, :] < ln[:, None])).sum(1)
    v = _div(float(rows.sum()), D * int(ln.sum()))
    return rows, (math.sqrt(v) if order == 2 else v)


def same(a, b, rel):
    """a within rel of b, NaN matching NaN and an exact zero matching itself."""
    if math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= rel * abs(b)


def step_numbers(terms, kl=0.0):
    """The logged numbers of run_training_step and TacotronTask.train_forward (extra_loss False / True) from the term table."""
    mel, mel_post = terms[0] + terms[2], terms[1] + terms[3]
    run = {"loss_mel_db": 100 * mel, "loss_mel_post_db": 100 * mel_post, "loss_stop": terms[6], "loss_kl": kl, "loss_w": terms[7],
           "loss": 0.8 * mel + 0.2 * mel_post + 0.1 * terms[6] + 0.0002 * kl + 0.0001 * terms[7]}
    out = {"run_training_step": run}
    for extra in (0, 1):
        total = 0.8 * terms[0] + 0.2 * terms[1] + 0.1 * terms[6] + 0.0002 * kl
        if extra:
            total += 0.0001 * terms[7] + 0.4 * terms[4] + 0.1 * terms[5]
        out[f"train_forward_extra_{extra}"] = {"total": total, "mel_db": 100 * terms[0], "mel_post_db": 100 * terms[1], "stop": terms[6], "kl": kl,
                                               "w": terms[7], "loss": total}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    import torch_tts_amd as T
    from torch_tts_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsdec"] and hasattr(lib, sym), sym
    assert re.search(r"#define\s+TTSDEC_VERSION\s+2\b", hdr) and lib.ttsdec_version() == 2
    assert re.search(r"#define\s+TTSDEC_VAL_FRAME_RUN\s+32\b", hdr)
    for name in NEW_FUNCTIONS:
        assert callable(getattr(T, name)) and getattr(T, name) is getattr(T.tacotron, name) and name in T.__all__, name
    import importlib.util

    spec = importlib.util.spec_from_file_location("_build_for_test", os.path.join(ROOT, "torch-tts_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "valstep.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "torch-tts_amd", "csrc", "valstep.hip"))


def test_workspace_sizes_and_refusal_order():
    """Sizes, then pointers, then the workspace - on a handle without a device, where a call that passed every check answers
    TTSDEC_ERR_DEVICE instead of launching."""
    from torch_tts_amd import _lib
    from torch_tts_amd.engine import Engine, EngineDims

    lib = _lib.load()
    eng = Engine(EngineDims(), None)
    h, one, big = eng._h, 256, 1 << 30  # (non-null, aligned placeholders: nothing is dereferenced)
    INV, DIMS, WS, DEV = _lib.ERR_INVALID_ARG, _lib.ERR_DIMS, _lib.ERR_WORKSPACE, _lib.ERR_DEVICE
    wsb = lib.ttsdec_val_losses_workspace_bytes
    up = lambda n: (n + 63) // 64 * 64  # noqa: E731  (buffers of a workspace are 64 floats apart)
    assert wsb(h, 64, 600, 200) == 4 * (4 * 64 * 600 + 2 * 64 * 200) == 716800
    assert wsb(h, 256, 600, 600) == 4 * (4 * 256 * 600 + 2 * 256 * 600)
    assert wsb(h, 3, 5, 0) == 4 * 4 * up(15) == 1024 and wsb(h, 3, 5, 5) == 1536 and wsb(h, 1, 1, 1) == 1536
    for bad in ((None, 1, 5, 1), (h, 0, 5, 1), (h, 1, 0, 1), (h, 1, 5, -1), (h, 65536, 5, 1)):
        assert wsb(*bad) == 0, bad

    def vl(B=2, T=10, D=8, T_x=12, S=5, L=7, y=one, yp=one, x=one, s=one, w=one, ln=one, rows=one, terms=one, ws=one, nbytes=big, hh=h):
        return lib.ttsdec_val_losses(hh, y, yp, x, T_x, s, w, ln, B, T, D, S, L, 0.1, rows, terms, ws, nbytes, None)

    assert vl() == DEV
    assert vl(hh=None) == INV
    for bad in (dict(B=0), dict(T=0), dict(D=-1), dict(T_x=0), dict(T_x=9), dict(S=0), dict(L=0)):
        assert vl(**bad, rows=None) == INV, bad
    assert vl(S=0, L=0, w=None) == DEV  # S and L are read with w only
    for bad in (dict(B=65536), dict(D=1025), dict(B=4096, T_x=1 << 19, T=4), dict(S=1 << 16, L=1 << 16)):
        assert vl(**bad, rows=None) == DIMS, bad  # (sizes before pointers)
    assert vl(D=1024) == DEV
    for ptr in ("rows", "terms"):
        assert vl(**{ptr: None}) == INV, ptr
    assert vl(y=None) == INV and vl(x=None) == INV and vl(y=None, x=None) == INV  # y and x together; y_post needs y
    assert vl(y=None, x=None, yp=None) == DEV and vl(yp=None) == DEV and vl(s=None) == DEV and vl(ln=None) == DEV
    assert vl(y=None, x=None, yp=None, s=None, w=None) == INV  # nothing to do
    need = wsb(h, 2, 10, 5)
    assert vl(ws=None) == WS and vl(nbytes=need - 1) == WS and vl(ws=one + 16) == WS and vl(nbytes=need) == DEV
    assert vl(w=None, nbytes=wsb(h, 2, 10, 0)) == DEV
    assert vl(rows=None, nbytes=0) == INV  # pointers before the workspace

    def ml(B=2, T=10, D=8, T_x=10, order=1, y=one, x=one, ln=one, rows=one, out=one, ws=one, nbytes=big):
        return lib.ttsdec_mel_loss(h, y, x, T_x, ln, B, T, D, order, rows, out, ws, nbytes, None)

    assert ml() == DEV and ml(ln=None) == DEV and ml(order=0) == DEV and ml(order=2) == DEV
    for bad in (dict(B=0), dict(T=0), dict(D=0), dict(T_x=9), dict(order=3), dict(order=-1)):
        assert ml(**bad, y=None) == INV, bad
    assert ml(B=65536, y=None) == DIMS and ml(D=1025, y=None) == DIMS
    for ptr in ("y", "x", "rows", "out"):
        assert ml(**{ptr: None}) == INV, ptr
    assert ml(ws=None) == WS and ml(nbytes=wsb(h, 2, 10, 0) - 1) == WS and ml(nbytes=wsb(h, 2, 10, 0)) == DEV
    eng.close()


def test_restatement_reproduces_the_reference_in_fp64():
    sd, meta = load_golden()
    assert set(meta["cases"]) == {"d80", "d3", "d1", "d260", "t1", "zero", "onehot"}
    for name, c in meta["cases"].items():
        t = case_tensors(sd, name)
        assert t["y"].shape == (c["B"], c["T"], c["D"]) and t["x"].shape[1] == c["T_x"] and t["w"].shape == (c["B"], c["S"], c["L"])
        assert t["lengths"].tolist() == c["lengths"] and c["S"] == c["T"] // c["r"]
        rows, terms = restate(t["y"], t["y_post"], t["x"], t["s"], t["w"], t["lengths"], meta["pos_weight"])
        for i, rec in enumerate(TERM_RECORDS):
            # (the record's own form of the variance cancels, in fp64 too: 1e-7 where the variance is near 0)
            assert same(terms[i], c["ref64"][rec], 1e-7 if (name, rec) == ("onehot", "w_std") else 1e-10), (name, rec, terms[i], c["ref64"][rec])
        ln = torch.tensor(c["lengths"]).clamp(0, c["T"])
        assert terms[9] == float(ln.sum()) and terms[10] == float((ln - 1).clamp(min=0).sum()) and terms[11:] == [0.0] * 5
        for order in (0, 1, 2):
            assert same(mel_restated(t["y"], t["x"], None, order)[1], c["ref64"][f"mel_o{order}"], 1e-10), (name, order)
            assert same(mel_restated(t["y"], t["x"], t["lengths"], order)[1], c["ref64"][f"mel_o{order}_m"], 1e-10), (name, order)
        assert torch.equal(mel_restated(t["y"], t["x"], t["lengths"], 1)[0], rows[:, 0])
        # the yardstick: the reference's own fp32 is ten times inside the GPU bar
        assert all(v <= 1e-5 for v in c["rel_err"].values()) and 10 * 1e-5 <= REL
        # an operand left out leaves its entries zero and the others as they were
        rows_n, terms_n = restate(t["y"], None, t["x"], t["s"], None, t["lengths"], meta["pos_weight"])
        assert terms_n[1] == terms_n[3] == terms_n[5] == terms_n[7] == terms_n[8] == 0.0 and terms_n[6] == terms[6]
    # what the cases are there for
    c = meta["cases"]
    assert c["d80"]["T"] == 32 + 1 and max(c["d80"]["lengths"]) > c["d80"]["T"] and 1 in c["d80"]["lengths"] and 0 in c["d3"]["lengths"]
    assert c["d80"]["T_x"] > c["d80"]["T"] and c["d260"]["D"] > 256 and c["d3"]["D"] % 4 and c["d1"]["D"] == 1
    assert {c[n]["L"] for n in c} >= {1, 2, 64, 65, 301} and {c[n]["r"] for n in c} == {1, 2, 3}
    assert float(sd["d80/s"].abs().max()) == 40.0
    assert math.isnan(c["t1"]["ref64"]["dmel_all"]) and not math.isnan(c["t1"]["ref64"]["mel_o1_m"])
    assert math.isnan(c["zero"]["ref64"]["mel_o1_m"]) and not math.isnan(c["zero"]["ref64"]["dmel_all"])
    one = c["onehot"]
    assert one["ref64"]["w_std"] < 0.05 and one["e_ref"] == abs(one["ref32"]["w_std"] - one["ref64"]["w_std"]) > REL * one["ref64"]["w_std"]
    assert float((sd["onehot/w"].sum(2) - 1).abs().max()) == 0.0


def test_end_to_end_record_from_its_own_tensors():
    """The reference's logged numbers of run_training_step and train_forward follow from the term table on its own y, y_post, s, w:
    the weights and keys task_forward and run_validation_step use."""
    sd, meta = load_golden()
    e = meta["e2e"]
    assert e["T"] >= 24 and not all(e["teacher_forced"]) and len(set(e["x_lengths"])) == 3 and max(e["x_lengths"]) == e["T"]
    _, terms = restate(sd["e2e/y"], sd["e2e/y_post"], sd["e2e/x"], sd["e2e/s"], sd["e2e/w"], sd["e2e/x_lengths"], meta["pos_weight"])
    got = step_numbers(terms)
    for rec, numbers in got.items():
        assert set(numbers) == set(e[rec])
        for k, v in numbers.items():
            assert same(v, e[rec][k], 2e-5), (rec, k, v, e[rec][k])  # (the record is the reference's fp32)
    assert e["keys_run_training_step"] == sorted(list(got["run_training_step"])[:-1] + ["w"])
    assert e["keys_log"] == sorted(k for k in got["train_forward_extra_0"] if k != "loss") and e["keys_img"] == ["w", "y_post"]


def test_fixture_checksum_and_size():
    _, meta = load_golden()
    path = os.path.join(HERE, "golden", "valstep_small.npz")
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == meta["npz_sha256"]
    assert os.path.getsize(path) < 1 << 20


def test_functions_refuse_what_is_not_on_the_path():
    import torch_tts_amd as T

    y, x = torch.zeros(2, 5, 4), torch.zeros(2, 6, 4)
    mask = torch.ones(2, 5, 1)
    for call in (lambda: T.mel_loss_fn(y, x), lambda: T.mel_loss_fn(y, x, mask, 0), lambda: T.alignment_std_loss(torch.rand(2, 3, 4)),
                 lambda: T.alignment_max_loss(torch.rand(2, 3, 4)), lambda: T.stop_loss(torch.zeros(2, 5), torch.tensor([5, 2]))):
        with pytest.raises(RuntimeError, match="no CPU path"):  # a CPU tensor
            call()
    for call in (lambda: T.mel_loss_fn(y.half(), x.half()), lambda: T.mel_loss_fn(y.double(), x.double(), mask.double()),
                 lambda: T.alignment_std_loss(torch.rand(2, 3, 4).double()), lambda: T.stop_loss(torch.zeros(2, 5).half(), torch.tensor([5, 2]))):
        with pytest.raises(NotImplementedError, match="exact fp32"):
            call()
    holes = mask.clone()
    holes[1, 2] = 0  # a hole inside an utterance
    with pytest.raises(ValueError, match="not a prefix mask"):
        T.mel_loss_fn(y, x, holes)
    with pytest.raises(ValueError, match=r"\[B, T, 1\]"):
        T.mel_loss_fn(y, x, torch.ones(2, 5))
    with pytest.raises(ValueError):
        T.mel_loss_fn(y, x, mask, order=3)
    with pytest.raises(ValueError):
        T.mel_loss_fn(y, x[:, :4])  # x shorter than y
    with pytest.raises(ValueError):
        T.stop_loss(torch.zeros(2, 5), torch.tensor([5.0, 2.0]))
    model = torch.nn.Linear(1, 1).train()
    with pytest.raises(RuntimeError, match="inference only"):
        T.validation_terms(model, torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2]), x, torch.tensor([6, 4]))
    with pytest.raises(RuntimeError, match="inference only"):
        T.task_forward(model, (None, torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2]), x, torch.tensor([6, 4])))
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.run_validation_step(model.eval(), (torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2]), x, torch.tensor([6, 4])), "cpu")


def test_torch_op_forms_agree_with_the_restatement():
    """autograd_path's forms - what an operand that requires grad gets, and what tools/time_tacotron_losses.py times against - are
    device-only like the rest of the package; their formulas, evaluated here through the same torch ops on the CPU records."""
    from torch_tts_amd import autograd_path as AP

    sd, meta = load_golden()
    t = case_tensors(sd, "d80")
    T_ = t["y"].shape[1]
    ln = t["lengths"].clamp(0, T_)
    mask = (torch.arange(T_)[None, :] < ln[:, None]).unsqueeze(2).float()
    orig, AP._require_device = AP._require_device, lambda *a: None
    try:
        for order in (0, 1, 2):
            assert same(float(AP.mel_loss_fn(t["y"], t["x"][:, :T_], mask, order)), mel_restated(t["y"], t["x"], ln, order)[1], 1e-5)
            assert same(float(AP.mel_loss_fn(t["y"], t["x"][:, :T_], None, order)), mel_restated(t["y"], t["x"], None, order)[1], 1e-5)
        _, terms = restate(t["y"], t["y_post"], t["x"], t["s"], t["w"], ln, 0.1)
        assert same(float(AP.stop_loss(t["s"], ln, 0.1)), terms[6], 1e-5)
        assert same(float(AP.alignment_std_loss(t["w"])), terms[7], 1e-5) and same(float(AP.alignment_max_loss(t["w"])), terms[8], 1e-5)
    finally:
        AP._require_device = orig
