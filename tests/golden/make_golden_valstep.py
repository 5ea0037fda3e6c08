#!/usr/bin/env python3
"""Golden records for the Tacotron validation step (csrc/valstep.hip, torch_tts_amd.tacotron.validation_terms and its callers),
produced by the reference's own tacotron.py and tacotron_lightning.py on the CPU.

    TTS_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_valstep.py

``lightning``, which tacotron_lightning.py imports for its base class and which is not installed here, is a stub module whose
LightningModule is torch.nn.Module: TacotronTask.train_forward uses nothing else of it.  No reference text is written.

Writes tests/golden/valstep_small.npz + valstep_meta.json:

(a) loss-function records, one per entry of CASES: fixed random y, y_post [B, T, D], x [B, T_x >= T, D], s [B, T] (logits up to
    |40|), w [B, S, L], lengths [B] under ``<case>/``, and in the meta the reference's values on them, in fp32 (``ref32``) and after
    .double() (``ref64``):
      mel_o{0,1,2} / mel_o{0,1,2}_m   mel_loss_fn(y, x[:, :T], None / xmask, order)
      melp_o1_m                       mel_loss_fn(y_post, x[:, :T], xmask, 1)
      dmel_all / dmelp_all            mel_loss_fn(y.diff(1), x.diff(1), order=1)                  (run_training_step)
      dmel_m / dmelp_m                mel_loss_fn(y.diff(1), x.diff(1), xmask[:, 1:], order=1)    (TacotronTask.train_forward)
      stop                            binary_cross_entropy_with_logits(s, xmask.float(), pos_weight=0.1)
      w_std / w_max                   alignment_std_loss(w) / alignment_max_loss(w)
    with xmask = (arange(T) < lengths)[:, :, None], the reference's lengths_to_mask cut to T frames.  A value the reference
    itself leaves undefined (0 / 0: every length 0, or T = 1 for the difference terms) is stored as NaN.  ``rel_err`` is
    |ref32 - ref64| / |ref64| of each defined value; the script asserts it is <= 1e-5 for every stored value, so the GPU tests' bar
    of 1e-4 against an fp64 restatement is at least ten times the reference's own fp32 error.  The case ``onehot`` has alignment
    rows that are near one-hot and sum to 1: the variance is near 0, where a relative error says nothing, and the meta records the
    reference's absolute fp32-against-fp64 error ``e_ref`` of w_std instead.
(b) one end-to-end record, ``e2e/``: the reference's Tacotron at the dims and weights of small_model.npz (Encoder2, the
    Taco2ProdDecoderCell decoder, MelPostnet, no style encoder) in eval mode, teacher input x [3, 26, 20] with x_lengths 26 / 19 / 9,
    under torch.manual_seed(seed) before each call (the first seed from SEED on
    whose replayed coin flips of decoder.py:65 leave a step not teacher-forced; recorded): what run_training_step(model, (c, c_lengths, x, x_lengths), "cpu") and
    TacotronTask(model, lr, extra_loss).train_forward((None, c, c_lengths, x, x_lengths)) return for both extra_loss settings -
    the floats in the meta, w and y_post in the npz."""
import copy
import hashlib
import json
import math
import os
import sys
import types

import numpy as np
import torch
import yaml

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("TTS_REFERENCE")
if not REF:
    sys.exit("set TTS_REFERENCE to a checkout of the reference project")
sys.path.insert(0, os.path.join(REF, "tacotron"))
sys.path.insert(0, ROOT)
stub = types.ModuleType("lightning")
stub.LightningModule = torch.nn.Module
sys.modules["lightning"] = stub
import tacotron as ref  # noqa: E402
import tacotron_lightning as ref_task  # noqa: E402
from oracle import tacotron_oracle as O  # noqa: E402

torch.set_num_threads(4)
SEED = 31
POS_WEIGHT = 0.1
# name: B, T, T_x, D, r, L, lengths, how the rows of w are drawn
CASES = {
    "d80": dict(B=3, T=33, T_x=36, D=80, r=3, L=65, lengths=[40, 17, 1], w="softmax"),     # a run boundary and its halo inside an utterance
    "d3": dict(B=3, T=5, T_x=5, D=3, r=1, L=2, lengths=[5, 0, 3], w="rand"),               # no 16-byte path; rows of w that do not sum to 1
    "d1": dict(B=1, T=2, T_x=4, D=1, r=2, L=1, lengths=[2], w="rand"),
    "d260": dict(B=1, T=5, T_x=6, D=260, r=1, L=301, lengths=[4], w="softmax"),            # more than one pass of a wave
    "t1": dict(B=3, T=1, T_x=2, D=3, r=1, L=64, lengths=[1, 0, 1], w="softmax"),           # no difference terms
    "zero": dict(B=3, T=5, T_x=5, D=3, r=1, L=64, lengths=[0, 0, 0], w="softmax"),         # no masked terms
    "onehot": dict(B=1, T=6, T_x=6, D=4, r=1, L=120, lengths=[6], w="onehot"),             # variance near 0
}


def draw_case(name, c):
    g = torch.Generator().manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    B, T, S = c["B"], c["T"], c["T"] // c["r"]
    x = torch.randn(B, c["T_x"], c["D"], generator=g) * 0.5 + 0.2
    y = x[:, :T] + 0.3 * torch.randn(B, T, c["D"], generator=g)
    y_post = x[:, :T] + 0.2 * torch.randn(B, T, c["D"], generator=g)
    s = (15.0 * torch.randn(B, T, generator=g)).clamp(-40.0, 40.0)
    s.view(-1)[0] = 40.0
    s.view(-1)[-1] = -40.0
    if c["w"] == "softmax":
        w = torch.softmax(2.0 * torch.randn(B, S, c["L"], generator=g), dim=2)
    elif c["w"] == "rand":
        w = torch.rand(B, S, c["L"], generator=g)
    else:  # near one-hot rows that sum to 1: a little weight beside the peak
        w = torch.zeros(B, S, c["L"])
        for i in range(S):
            k = 5 + 19 * i
            w[:, i, k], w[:, i, k + 1] = 1.0 - 2.0 ** -(10 + i), 2.0 ** -(10 + i)
    return dict(y=y, y_post=y_post, x=x, s=s, w=w, lengths=torch.tensor(c["lengths"], dtype=torch.int64))


def reference_values(t, dtype):
    y, y_post, x, s, w = (t[k].to(dtype) for k in ("y", "y_post", "x", "s", "w"))
    T = y.shape[1]
    x = x[:, :T]
    xmask = (torch.arange(T)[None, :] < t["lengths"][:, None]).unsqueeze(2)
    out = {}
    for order in (0, 1, 2):
        out[f"mel_o{order}"] = ref.mel_loss_fn(y, x, None, order)
        out[f"mel_o{order}_m"] = ref.mel_loss_fn(y, x, xmask, order)
    out["melp_o1_m"] = ref.mel_loss_fn(y_post, x, xmask, 1)
    out["dmel_all"] = ref.mel_loss_fn(y.diff(dim=1), x.diff(dim=1), order=1)
    out["dmelp_all"] = ref.mel_loss_fn(y_post.diff(dim=1), x.diff(dim=1), order=1)
    out["dmel_m"] = ref.mel_loss_fn(y.diff(dim=1), x.diff(dim=1), xmask[:, 1:], order=1)
    out["dmelp_m"] = ref.mel_loss_fn(y_post.diff(dim=1), x.diff(dim=1), xmask[:, 1:], order=1)
    pw = torch.tensor([POS_WEIGHT], dtype=dtype)
    out["stop"] = torch.nn.functional.binary_cross_entropy_with_logits(s.unsqueeze(2), xmask.to(dtype), pos_weight=pw)
    out["w_std"] = ref.alignment_std_loss(w)
    out["w_max"] = ref.alignment_max_loss(w)
    return {k: float(v) for k, v in out.items()}


def small_config():  # make_golden.py's
    cfg = copy.deepcopy(yaml.safe_load(open(os.path.join(REF, "configs/config-ljspeech.yaml"))))
    cfg["audio"]["num_mels"] = 20
    cfg["model"]["encoder"]["dim_emb"], cfg["model"]["encoder"]["dim_out"] = 24, 40
    cfg["model"]["decoder"]["dim_pre"], cfg["model"]["decoder"]["dim_att"], cfg["model"]["decoder"]["dim_rnn"] = 36, 72, [72, 88]
    cfg["model"]["postnet"]["dim_hidden"], cfg["model"]["postnet"]["num_layers"] = 64, 3
    return cfg


def small_model():
    z = np.load(os.path.join(HERE, "small_model.npz"))
    model = ref.build_tacotron(small_config()).eval()
    sd = {}
    for k in z.files:
        for short, full in (("enc/", "encoder."), ("dec/", "decoder."), ("post/", "postnet.")):
            if k.startswith(short):
                sd[full + k[len(short):]] = torch.from_numpy(z[k])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    assert model.refencoder is None and model.postnet is not None
    return model, torch.from_numpy(z["ids"]), torch.from_numpy(z["lengths"])


def floats(d):
    return {k: v for k, v in d.items() if isinstance(v, float)}


def main():
    meta = {"reference": "kgoba/torch-tts @ 2024_10_08", "torch": torch.__version__, "pos_weight": POS_WEIGHT, "cases": {}}
    npz = {}
    for name, c in CASES.items():
        t = draw_case(name, c)
        r32, r64 = reference_values(t, torch.float32), reference_values(t, torch.float64)
        err = {}
        for k in r64:
            if math.isnan(r64[k]):
                assert math.isnan(r32[k]), (name, k)
                continue
            if name == "onehot" and k == "w_std":
                continue
            if r64[k] == 0.0:  # (an exact zero: one attention position has no variance)
                assert r32[k] == 0.0, (name, k, r32[k])
                err[k] = 0.0
                continue
            err[k] = abs(r32[k] - r64[k]) / abs(r64[k])
            assert err[k] <= 1e-5, (name, k, r32[k], r64[k])
        rec = dict(c, S=c["T"] // c["r"], ref32=r32, ref64=r64, rel_err=err)
        if name == "onehot":
            rec["e_ref"] = abs(r32["w_std"] - r64["w_std"])
            assert r64["w_std"] < 0.05, r64["w_std"]
        meta["cases"][name] = rec
        for k, v in t.items():
            npz[f"{name}/{k}"] = v.numpy()
    nan_terms = {n: sorted(k for k, v in meta["cases"][n]["ref64"].items() if math.isnan(v)) for n in ("t1", "zero")}
    assert nan_terms["t1"] == ["dmel_all", "dmel_m", "dmelp_all", "dmelp_m"], nan_terms
    assert nan_terms["zero"] == ["dmel_m", "dmelp_m", "mel_o0_m", "mel_o1_m", "mel_o2_m", "melp_o1_m"], nan_terms

    # ---- (b) the end-to-end record ----
    model, ids, c_lengths = small_model()
    B, T_x, d_mel = ids.shape[0], 26, 20
    x = 0.5 * torch.randn(B, T_x, d_mel, generator=torch.Generator().manual_seed(77))
    x_lengths = torch.tensor([26, 19, 9])
    # the coin flips of decoder.py:65, replayed: per step two PreNet masks, then (but after the last step) one torch.rand(1)
    seed = SEED - 1
    forced = [True]
    while all(forced):  # the first seed from SEED on that leaves a step unforced
        seed += 1
        torch.manual_seed(seed)
        forced = []
        for t in range(T_x):
            O.draw_prenet_masks(B, 36, 36)
            if t < T_x - 1:
                forced.append(bool(torch.rand(1) > 0.1))
    assert not all(forced) and any(forced), forced
    with torch.no_grad():
        torch.manual_seed(seed)
        y, y_post, s, out = model(ids, c_lengths, x, x_lengths, xref=x, xref_lengths=x_lengths)
        torch.manual_seed(seed)
        loss, logs = ref.run_training_step(model, (ids, c_lengths, x, x_lengths), "cpu")
        e2e = {"seed": seed, "teacher_forced": forced, "x_lengths": x_lengths.tolist(), "T": int(y.shape[1]),
               "run_training_step": dict(floats(logs), loss=float(loss)), "keys_run_training_step": sorted(logs)}
        assert torch.equal(logs["w"], out["w"]) and y.shape[1] == T_x >= 24
        for extra in (False, True):
            task = ref_task.TacotronTask(model, 1e-3, extra_loss=extra)
            torch.manual_seed(seed)
            loss_t, log_t, img_t = task.train_forward((None, ids, c_lengths, x, x_lengths))
            assert torch.equal(img_t["w"], out["w"]) and torch.equal(img_t["y_post"], y_post)
            e2e[f"train_forward_extra_{int(extra)}"] = dict(floats(log_t), loss=float(loss_t))
            e2e["keys_log"], e2e["keys_img"] = sorted(log_t), sorted(img_t)
    meta["e2e"] = e2e
    npz.update({"e2e/x": x.numpy(), "e2e/x_lengths": x_lengths.numpy(), "e2e/y": y.numpy(), "e2e/y_post": y_post.numpy(), "e2e/s": s.numpy(),
                "e2e/w": out["w"].numpy()})
    path = os.path.join(HERE, "valstep_small.npz")
    np.savez_compressed(path, **npz)
    meta["npz_sha256"] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    with open(os.path.join(HERE, "valstep_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps({n: max(r["rel_err"].values()) for n, r in meta["cases"].items()}, indent=1))
    print("e_ref", meta["cases"]["onehot"]["e_ref"], "w_std64", meta["cases"]["onehot"]["ref64"]["w_std"])
    print(json.dumps(e2e, indent=1)[:2000])
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
