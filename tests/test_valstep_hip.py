"""GPU tests of the Tacotron validation step's loss terms (csrc/valstep.hip through ttsdec_val_losses / ttsdec_mel_loss and
torch_tts_amd.tacotron): every term and every per-utterance sum against the fp64 restatement of tests/test_valstep_host.py (itself
checked against the reference's fp64 records) at the project's bar of 1e-4 relative, at the smallest shapes at which each mechanism
can break - D without a 16-byte path and beyond one pass of a wave, T on both sides of a frame run, lengths 0 / 1 / T / above T,
T_x > T, operands left out, the divisors that are zero - the bit-level promises (an utterance alone, a call twice, the two load
paths), the workspace's reach, and the end-to-end record of the reference's run_training_step / TacotronTask.train_forward."""
import math

import pytest
import torch

import test_valstep_host as HOST
from test_valstep_host import REL, TERM_RECORDS, case_tensors, mel_restated, restate, same, step_numbers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ("d80", "d3", "d1", "d260", "t1", "zero", "onehot")


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    sd, meta = HOST.load_golden()
    return {"sd": sd, "meta": meta, "cuda": {k: v.to(DEV) for k, v in sd.items()}}


def engine():
    import torch_tts_amd as T

    return T.tacotron._engine(torch.device(DEV))


def on_gpu(G, name):
    t = {k: G["cuda"][f"{name}/{k}"] for k in ("y", "y_post", "x", "s", "w")}
    t["lengths"] = G["cuda"][f"{name}/lengths"].to(torch.int32)
    return t


def call(t, **override):
    a = dict(t, **override)
    shape = None
    if a["y"] is None:  # (B, T, D) then come from the stop logits, or the alignment alone
        shape = (a["s"].shape[0], a["s"].shape[1], 1) if a["s"] is not None else (a["w"].shape[0], 1, 1)
    rows, terms = engine().val_losses(a["y"], a["y_post"], a["x"], a["s"], a["w"], a["lengths"], 0.1, shape=shape)
    return rows.cpu(), terms.cpu()


def assert_rows(rows, want, what, skip=()):
    for k in range(9):
        if k in skip:
            continue
        for b in range(rows.shape[0]):
            assert same(float(rows[b, k]), float(want[b, k]), REL), (what, "rows", b, k, float(rows[b, k]), float(want[b, k]))


def assert_terms(terms, want, what, bars=None):
    assert terms.shape == (16,)
    for i in range(16):
        got, w = float(terms[i]), want[i]
        if bars and i in bars:
            assert abs(got - w) <= max(REL * abs(w), bars[i]), (what, i, got, w)
        else:
            assert same(got, w, REL), (what, "terms", i, got, w)


@pytest.mark.parametrize("name", CASES)
def test_terms_and_rows_against_the_fp64_restatement(G, name):
    c = G["meta"]["cases"][name]
    cpu, t = case_tensors(G["sd"], name), on_gpu(G, name)
    rows, terms = call(t)
    want_rows, want = restate(cpu["y"], cpu["y_post"], cpu["x"], cpu["s"], cpu["w"], cpu["lengths"], 0.1)
    # the near-zero variance: the bar is the reference's own fp32 error there (of w_std; its square, the row sum of variances, likewise)
    near0 = name == "onehot"
    assert_rows(rows, want_rows, name, skip=(7,) if near0 else ())
    assert_terms(terms, want, name, bars={7: c["e_ref"]} if near0 else None)
    if near0:
        assert abs(float(terms[7]) - want[7]) < 0.1 * c["e_ref"]  # (the form without the cancellation is far inside it)
    for i, rec in enumerate(TERM_RECORDS):  # and the reference's fp64 records directly
        r = c["ref64"][rec]
        assert math.isnan(float(terms[i])) if math.isnan(r) else abs(float(terms[i]) - r) <= max(REL * abs(r), c.get("e_ref", 0.0) if i == 7 else 0.0)
    # the divisors that are zero give NaN in their own terms only
    nan = {i for i in range(16) if math.isnan(float(terms[i]))}
    assert nan == {"t1": {2, 3}, "zero": {0, 1, 4, 5}}.get(name, set()) | ({4, 5} if name == "t1" else set()), (name, nan)
    # a call repeats bit for bit
    rows2, terms2 = call(t)
    assert torch.equal(rows, rows2) and torch.equal(terms.view(torch.int32), terms2.view(torch.int32))


@pytest.mark.parametrize("name", ("d80", "d3"))
def test_an_utterance_alone_gets_the_same_bits(G, name):
    t = on_gpu(G, name)
    rows, _ = call(t)
    for b in range(t["y"].shape[0]):
        one = {k: v[b:b + 1].contiguous() for k, v in t.items()}
        rows1, terms1 = call(one)
        assert torch.equal(rows1[0].view(torch.int32), rows[b].view(torch.int32)), (name, b)
        cpu = {k: v[b:b + 1] for k, v in case_tensors(G["sd"], name).items()}
        _, want = restate(cpu["y"], cpu["y_post"], cpu["x"], cpu["s"], cpu["w"], cpu["lengths"], 0.1)
        assert_terms(terms1, want, (name, b))  # B = 1, with lengths 0, 1, T and above T among them


def test_operands_left_out(G):
    """y_post NULL, w NULL, s NULL, the frame operands NULL, lengths NULL: the entries of what is there keep their bits, the others are zero."""
    t, cpu = on_gpu(G, "d80"), case_tensors(G["sd"], "d80")
    rows, terms = call(t)
    for left_out, zero_rows, zero_terms in (({"y_post": None}, (1, 3, 5), (1, 3, 5)), ({"w": None}, (7, 8), (7, 8)), ({"s": None}, (6,), (6,)),
                                            ({"y": None, "y_post": None, "x": None}, (0, 1, 2, 3, 4, 5), (0, 1, 2, 3, 4, 5)),
                                            ({"y": None, "y_post": None, "x": None, "s": None}, (0, 1, 2, 3, 4, 5, 6), (0, 1, 2, 3, 4, 5, 6))):
        r, tm = call(t, **left_out)
        for k in range(9):
            assert torch.equal(r[:, k], torch.zeros(3) if k in zero_rows else rows[:, k]), (left_out, k)
        for i in range(16):
            if "s" in left_out and "y" in left_out and i in (9, 10):
                continue  # (T is not known without y and s: the alignment terms do not read it)
            assert float(tm[i]) == (0.0 if i in zero_terms else float(terms[i])), (left_out, i)
    r, tm = call(t, lengths=None)
    want_rows, want = restate(cpu["y"], cpu["y_post"], cpu["x"], cpu["s"], cpu["w"], None, 0.1)
    assert_rows(r, want_rows, "no lengths")
    assert_terms(tm, want, "no lengths")


def test_both_load_paths_give_the_same_bits(G):
    """D = 80 from bases that are 4 bytes off a 16-byte boundary takes the 4-byte loads: the lane-to-channel map is the same, so
    are the sums."""
    t = on_gpu(G, "d80")
    rows, terms = call(t)

    def shifted(v):
        buf = torch.empty(v.numel() + 1, device=DEV)
        buf[1:].copy_(v.reshape(-1))
        return buf[1:].view(v.shape)

    off = {k: shifted(t[k]) for k in ("y", "y_post", "x")}
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in off.values())
    rows_s, terms_s = call(t, **off)
    assert torch.equal(rows_s.view(torch.int32), rows.view(torch.int32)) and torch.equal(terms_s.view(torch.int32), terms.view(torch.int32))


def test_workspace_tail_is_untouched(G):
    from torch_tts_amd import _lib

    lib, eng = _lib.load(), engine()
    for name in ("d80", "d260"):
        t = on_gpu(G, name)
        B, T, D = t["y"].shape
        S, L = t["w"].shape[1:]
        need = int(lib.ttsdec_val_losses_workspace_bytes(eng._h, B, T, S))
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        rows, terms = torch.empty(B, 9, device=DEV), torch.empty(16, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.ttsdec_val_losses(eng._h, t["y"].data_ptr(), t["y_post"].data_ptr(), t["x"].data_ptr(), t["x"].shape[1], t["s"].data_ptr(),
                                   t["w"].data_ptr(), t["lengths"].data_ptr(), B, T, D, S, L, 0.1, rows.data_ptr(), terms.data_ptr(), ws.data_ptr(),
                                   need, stream)
        assert rc == _lib.OK
        assert bool((ws[need:] == 0xA5).all()), name
        r0, t0 = call(t)
        assert torch.equal(rows.cpu(), r0) and torch.equal(terms.cpu().view(torch.int32), t0.view(torch.int32))
        assert lib.ttsdec_val_losses(eng._h, t["y"].data_ptr(), t["y_post"].data_ptr(), t["x"].data_ptr(), t["x"].shape[1], t["s"].data_ptr(),
                                     t["w"].data_ptr(), t["lengths"].data_ptr(), B, T, D, S, L, 0.1, rows.data_ptr(), terms.data_ptr(), ws.data_ptr(),
                                     need - 1, stream) == _lib.ERR_WORKSPACE
        need_m = int(lib.ttsdec_val_losses_workspace_bytes(eng._h, B, T, 0))
        ws.fill_(0xA5)
        out, rows1 = torch.empty(1, device=DEV), torch.empty(B, device=DEV)
        assert lib.ttsdec_mel_loss(eng._h, t["y"].data_ptr(), t["x"].data_ptr(), t["x"].shape[1], t["lengths"].data_ptr(), B, T, D, 2, rows1.data_ptr(),
                                   out.data_ptr(), ws.data_ptr(), need_m, stream) == _lib.OK
        assert bool((ws[need_m:] == 0xA5).all()), name


@pytest.mark.parametrize("name", CASES)
def test_mel_loss_fn_against_the_records(G, name):
    import torch_tts_amd as T

    c, t, cpu = G["meta"]["cases"][name], on_gpu(G, name), case_tensors(G["sd"], name)
    Tn = t["y"].shape[1]
    mask = (torch.arange(Tn, device=DEV)[None, :] < t["lengths"][:, None]).unsqueeze(2)
    for order in (0, 1, 2):
        for rec, kw in ((f"mel_o{order}", {}), (f"mel_o{order}_m", {"mask": mask.float()}), (f"mel_o{order}_m", {"mask": mask}),
                        (f"mel_o{order}_m", {"lengths": t["lengths"]})):
            got = T.mel_loss_fn(t["y"], t["x"], order=order, **kw)
            assert got.shape == () and got.device.type == "cuda"
            assert same(float(got), c["ref64"][rec], REL), (name, rec, list(kw), float(got), c["ref64"][rec])
        want_rows, want = mel_restated(cpu["y"], cpu["x"], cpu["lengths"], order)
        rows, out = engine().mel_loss(t["y"], t["x"], t["lengths"], order)
        assert same(float(out[0]), want, REL) and all(same(float(a), float(b), REL) for a, b in zip(rows.cpu(), want_rows))
    # order 1 is the frame pass of the fused call: the same bits
    assert torch.equal(engine().mel_loss(t["y"], t["x"], t["lengths"], 1)[0].cpu(), call(t)[0][:, 0])
    # the reference's own call shape: x cut to T frames (a view with its own batch stride is copied, a contiguous one is not)
    assert same(float(T.mel_loss_fn(t["y_post"], t["x"][:, :Tn], mask, 1)), c["ref64"]["melp_o1_m"], REL)


@pytest.mark.parametrize("name", CASES)
def test_alignment_and_stop_losses_against_the_records(G, name):
    import torch_tts_amd as T

    c, t = G["meta"]["cases"][name], on_gpu(G, name)
    r = c["ref64"]
    assert abs(float(T.alignment_std_loss(t["w"])) - r["w_std"]) <= max(REL * abs(r["w_std"]), c.get("e_ref", 0.0))
    assert same(float(T.alignment_max_loss(t["w"])), r["w_max"], REL)
    for s in (t["s"], t["s"].unsqueeze(2)):
        assert same(float(T.stop_loss(s, t["lengths"])), r["stop"], REL)
    assert same(float(T.stop_loss(t["s"], G["sd"][f"{name}/lengths"])), r["stop"], REL)  # int64 lengths on the host


def test_stop_loss_is_stable_at_large_logits():
    import torch_tts_amd as T

    s = torch.tensor([[40.0, -40.0, 88.0, -88.0, 0.0, 1e-8]], device=DEV)
    for ln in (0, 3, 6):
        got = float(T.stop_loss(s, torch.tensor([ln])))
        _, want = restate(None, None, None, s.cpu(), None, torch.tensor([ln]), 0.1)
        assert math.isfinite(got) and same(got, want[6], REL), (ln, got, want[6])


def test_an_operand_with_grad_takes_the_torch_ops(G):
    import torch_tts_amd as T

    t, c = on_gpu(G, "d80"), G["meta"]["cases"]["d80"]
    Tn = t["y"].shape[1]
    mask = (torch.arange(Tn, device=DEV)[None, :] < t["lengths"][:, None]).unsqueeze(2).float()
    y = t["y"].clone().requires_grad_(True)
    loss = T.mel_loss_fn(y, t["x"], mask, 1)
    assert loss.requires_grad and same(float(loss), c["ref64"]["mel_o1_m"], REL)
    loss.backward()
    assert y.grad is not None and float(y.grad[1, 20:].abs().max()) == 0.0  # (utterance 1 has 17 frames)
    w = t["w"].clone().requires_grad_(True)
    assert T.alignment_std_loss(w).requires_grad and same(float(T.alignment_max_loss(w)), c["ref64"]["w_max"], REL)
    s = t["s"].clone().requires_grad_(True)
    assert T.stop_loss(s, t["lengths"]).requires_grad and same(float(T.stop_loss(s, t["lengths"])), c["ref64"]["stop"], REL)
    with torch.no_grad():  # grad mode off: the HIP path, whatever the flag
        assert not T.mel_loss_fn(y, t["x"], mask, 1).requires_grad


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: the reference's own run of run_training_step / TacotronTask.train_forward
# ---------------------------------------------------------------------------------------------------------------------------
def small_tacotron(golden, refencoder=None):
    import hip_helpers as H
    import torch_tts_amd as T
    from oracle import tacotron_oracle as O

    d = golden["meta"]["small_dims"]
    dims = O.DecoderDims(d_mel=d["d_mel"], r=d["r"], d_pre=d["d_pre"], d_ctx=d["d_ctx"], h_att=d["h_att"], h_dec=d["h_dec"])
    enc = T.Encoder2(golden["enc"]["emb.weight"].shape[0], dim_out=d["d_ctx"], dim_emb=golden["enc"]["emb.weight"].shape[1])
    dec = H.make_decoder(dims, golden["dec"], device="cpu")
    pn = T.MelPostnet(d["d_mel"], dim_hidden=d["postnet_hidden"], kernel_size=5, num_layers=d["postnet_layers"])
    if refencoder is not None:
        torch.manual_seed(5)
    model = T.Tacotron(enc, dec, pn, refencoder)  # (its constructor re-initialises: load the fixture's weights afterwards)
    sd = {"encoder." + k: v for k, v in golden["enc"].items()}
    sd.update({"decoder." + k: v for k, v in golden["dec"].items()})
    sd.update({"postnet." + k: v for k, v in golden["post"].items()})
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") or k.endswith("attention_module.bias") or k.startswith("refencoder.")
                                  for k in missing), (missing, unexpected)
    return model.to(DEV).eval()


def test_end_to_end_against_the_reference_record(G, golden):
    import torch_tts_amd as T

    e, sd = G["meta"]["e2e"], G["sd"]
    model = small_tacotron(golden)
    assert model.decoder.dropout_source == "reference_rng"
    c, c_lengths, x, x_lengths = golden["ids"], golden["lengths"], sd["e2e/x"], sd["e2e/x_lengths"]
    torch.manual_seed(e["seed"])
    loss, logs = T.run_validation_step(model, (c, c_lengths, x, x_lengths), DEV)
    assert sorted(logs) == e["keys_run_training_step"] and loss.shape == () and loss.device.type == "cuda" and not loss.requires_grad
    want = dict(e["run_training_step"])
    assert same(float(loss), want.pop("loss"), REL)
    for k, v in want.items():
        assert isinstance(logs[k], float) and same(logs[k], v, REL), (k, logs[k], v)
    assert logs["w"].device.type == "cpu" and float((logs["w"] - sd["e2e/w"]).abs().max()) <= 1e-4
    for extra in (False, True):
        torch.manual_seed(e["seed"])
        loss, log, img = T.task_forward(model, (None, c.to(DEV), c_lengths.to(DEV), x.to(DEV), x_lengths.to(DEV)), extra_loss=extra)
        want = dict(e[f"train_forward_extra_{int(extra)}"])
        assert sorted(log) == e["keys_log"] and sorted(img) == e["keys_img"]
        assert same(float(loss), want.pop("loss"), REL) and float(loss) == pytest.approx(log["total"], rel=1e-6)
        for k, v in want.items():
            assert isinstance(log[k], float) and same(log[k], v, REL), (extra, k, log[k], v)
        torch.manual_seed(e["seed"])
        terms, y, y_post, s, out = T.validation_terms(model, c.to(DEV), c_lengths.to(DEV), x.to(DEV), x_lengths.to(DEV), xref=x.to(DEV),
                                                      xref_lengths=x_lengths.to(DEV))
        assert torch.equal(img["w"], out["w"].cpu()) and torch.equal(img["y_post"], y_post.cpu())  # the forward's own, under the same seed
        assert float((img["y_post"] - sd["e2e/y_post"]).abs().max()) <= 1e-4 + 1e-4 * float(sd["e2e/y_post"].abs().max())
    # the terms are those of the restatement on the forward's own outputs, and the logged numbers follow from them
    _, want_terms = restate(y.cpu(), y_post.cpu(), x, s.cpu(), out["w"].cpu(), x_lengths, 0.1)
    assert_terms(terms.cpu(), want_terms, "e2e")
    got = step_numbers([float(v) for v in terms.cpu()])
    assert same(log["total"], got["train_forward_extra_1"]["total"], 1e-6)


def test_training_mode_and_the_kl_of_a_style_encoder(G, golden):
    """With a VAE as refencoder and xref = x the step's loss_kl is the forward's kl_loss under the same seed, and enters the total with
    the reference's weight."""
    import torch_tts_amd as T

    e, sd = G["meta"]["e2e"], G["sd"]
    d = golden["meta"]["small_dims"]
    model = small_tacotron(golden, T.VAE(num_mels=d["d_mel"], dim_emb=d["d_ctx"], dim_enc=16, dim_vae=8))
    c, c_lengths, x, x_lengths = golden["ids"].to(DEV), golden["lengths"].to(DEV), sd["e2e/x"].to(DEV), sd["e2e/x_lengths"].to(DEV)
    with torch.no_grad():
        torch.manual_seed(e["seed"])
        _, _, _, out = model(c, c_lengths, x, x_lengths, xref=x, xref_lengths=x_lengths)
    kl = float(out["kl_loss"])
    assert kl > 0.0
    torch.manual_seed(e["seed"])
    loss, logs = T.run_validation_step(model, (c, c_lengths, x, x_lengths), DEV)
    assert logs["loss_kl"] == kl
    want = 0.8 * logs["loss_mel_db"] / 100 + 0.2 * logs["loss_mel_post_db"] / 100 + 0.1 * logs["loss_stop"] + 0.0002 * kl + 0.0001 * logs["loss_w"]
    assert same(float(loss), want, 1e-5)
    torch.manual_seed(e["seed"])
    _, log, _ = T.task_forward(model, (None, c, c_lengths, x, x_lengths))
    assert log["kl"] == kl
    model.train()
    with pytest.raises(RuntimeError, match="inference only"):
        T.run_validation_step(model, (c, c_lengths, x, x_lengths), DEV)
