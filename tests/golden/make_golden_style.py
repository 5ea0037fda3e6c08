#!/usr/bin/env python3
"""Golden vectors for the style encoders - ReferenceEncoder, GST, GST_VAE, VAE - produced by running the REFERENCE on the CPU.

    TTS_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_style.py
Writes tests/golden/style_small.npz + style_meta.json:
  enc/     ReferenceEncoder(num_mels=20, dim_out=16, ref_enc_filters=[4, 4, 8, 8, 16, 16]) alone, with ragged lengths and without
  gst/     the reference's GST with that encoder and STL(dim_query=16, num_tokens=5, dim_emb=32, num_heads=4) put in its place
  gstvae/  the reference's GST_VAE likewise, dim_vae=8
  vae/     VAE(num_mels=80, dim_vae=16) at the reference's fixed filter widths; its 0.49 M weights and its input are drawn on the
           fp16 grid (the large tensors on multiples of 2^-10) and stored as float16: they load to fp32 exactly
BatchNorm statistics, biases and the token embeddings are perturbed (fresh modules have zeros / ones there); the mean / logvar
biases are moved far enough that kl does not sit near zero.  eps: torch.randn_like is replaced while the module runs."""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TTS_REFERENCE")
if not REF:
    sys.exit("set TTS_REFERENCE to a checkout of the reference project")
sys.path.insert(0, os.path.join(REF, "tacotron"))
from modules import style as ref_style  # noqa: E402

torch.set_num_threads(4)
SMALL = dict(num_mels=20, dim_out=16, ref_enc_filters=[4, 4, 8, 8, 16, 16])
DIM_EMB, TOKENS, HEADS, DIM_VAE = 32, 5, 4, 8


def perturb(m, g, fp16_grid=False):
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith("running_mean"):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
        elif ".bns." in k and k.endswith(".weight"):
            v.copy_(1.5 + 0.5 * torch.rand(v.shape, generator=g))  # (gain > 1: six stride-2 stages would otherwise fade the signal)
        elif k.endswith("logvar_linear.bias"):
            v.copy_(-1.0 + 0.5 * torch.randn(v.shape, generator=g))
        elif k.endswith("mean_linear.bias"):
            v.copy_(0.5 * torch.randn(v.shape, generator=g) + 0.7)
        elif k.endswith(".bias") or k.endswith("bias_ih_l0") or k.endswith("bias_hh_l0"):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
        elif k.endswith("embed"):
            v.copy_(0.5 * torch.randn(v.shape, generator=g))
        elif k.endswith("convs.0.weight"):
            v.mul_(3.0)
        if fp16_grid:  # (the large tensors on multiples of 2^-10, which fp16 holds exactly below 2: they compress to a byte each)
            v.copy_((torch.round(v * 1024) / 1024 if v.numel() > 1000 else v).half().float())
    m.load_state_dict(sd)
    return m.eval()


def run(m, x, lengths, eps=None):
    orig = torch.randn_like
    if eps is not None:
        torch.randn_like = lambda t: eps.view_as(t).clone()
    try:
        with torch.no_grad():
            out = m(x, lengths) if lengths is not None else m(x)
    finally:
        torch.randn_like = orig
    return out


def weights(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}


def main():
    g = torch.Generator().manual_seed(23)
    torch.manual_seed(23)
    npz, meta = {}, {"small": {**SMALL, "dim_emb": DIM_EMB, "num_tokens": TOKENS, "num_heads": HEADS, "dim_vae": DIM_VAE}, "keys": {}}

    def small_encoder():
        return ref_style.ReferenceEncoder(**SMALL)

    def small_stl():
        return ref_style.STL(dim_query=SMALL["dim_out"], num_tokens=TOKENS, dim_emb=DIM_EMB, num_heads=HEADS)

    # ragged lengths: the padded length itself, one that is no multiple of 64, 64, one below 64 (clipped to one step), 1
    B, T = 5, 200
    lengths = torch.tensor([200, 130, 64, 63, 1])
    x = torch.randn(B, T, SMALL["num_mels"], generator=g)
    for b in range(B):
        x[b, lengths[b]:] = 0
    npz["x"], npz["lengths"] = x.numpy(), lengths.numpy()

    enc = perturb(small_encoder(), g)
    npz["enc/enc_out"] = run(enc, x, lengths).numpy()
    npz["enc/enc_out_nolen"] = run(enc, x, None).numpy()
    for k, v in weights(enc).items():
        npz["enc/w/" + k] = v.numpy()
    meta["keys"]["enc"] = {k: list(v.shape) for k, v in weights(enc).items()}

    gst = ref_style.GST(num_mels=SMALL["num_mels"], dim_emb=DIM_EMB, dim_enc=SMALL["dim_out"], num_tokens=TOKENS, num_heads=HEADS)
    gst.encoder, gst.stl = small_encoder(), small_stl()
    gst = perturb(gst, g)
    xo, extra = run(gst, x, lengths)
    assert extra == {} and xo.shape == (B, 1, DIM_EMB)
    npz["gst/x"], npz["gst/enc_out"] = xo.numpy(), run(gst.encoder, x, lengths).numpy()
    for k, v in weights(gst).items():
        npz["gst/w/" + k] = v.numpy()
    meta["keys"]["gst"] = {k: list(v.shape) for k, v in weights(gst).items()}

    gv = ref_style.GST_VAE(num_mels=SMALL["num_mels"], dim_emb=DIM_EMB, dim_enc=SMALL["dim_out"], num_tokens=TOKENS, num_heads=HEADS, dim_vae=DIM_VAE)
    gv.encoder, gv.stl = small_encoder(), small_stl()
    gv = perturb(gv, g)
    eps = torch.randn(B, 1, DIM_VAE, generator=g)
    xo, extra = run(gv, x, lengths, eps)
    assert xo.shape == (B, 1, DIM_EMB) and extra["kl"].shape == (B, 1, DIM_VAE)
    npz["gstvae/x"], npz["gstvae/kl"], npz["gstvae/eps"] = xo.numpy(), extra["kl"].numpy(), eps.numpy()
    npz["gstvae/enc_out"] = run(gv.encoder, x, lengths).numpy()
    for k, v in weights(gv).items():
        npz["gstvae/w/" + k] = v.numpy()
    meta["keys"]["gstvae"] = {k: list(v.shape) for k, v in weights(gv).items()}

    # the full-width VAE: weights and input on the fp16 grid
    vae = perturb(ref_style.VAE(num_mels=80, dim_vae=16), g, fp16_grid=True)
    Bv, Tv = 2, 130
    vlen = torch.tensor([130, 70])
    xv = torch.randn(Bv, Tv, 80, generator=g).half().float()
    xv[1, 70:] = 0
    veps = torch.randn(Bv, 16, generator=g)
    xo, extra = run(vae, xv, vlen, veps)
    assert xo.shape == (Bv, 1, 256) and extra["kl"].shape == (Bv, 16)
    # z re-derived from the recorded eps reproduces the module's output: the patched draw is the one it used
    enc_out = run(vae.encoder, xv, vlen)
    with torch.no_grad():
        z = veps * torch.exp(0.5 * vae.logvar_linear(enc_out)) + vae.mean_linear(enc_out)
        assert torch.equal(torch.tanh(vae.fc_out(z).unsqueeze(1)), xo)
    npz["vae/x_in"], npz["vae/lengths"], npz["vae/eps"] = xv.half().numpy(), vlen.numpy(), veps.numpy()
    npz["vae/x"], npz["vae/kl"], npz["vae/enc_out"] = xo.numpy(), extra["kl"].numpy(), enc_out.numpy()
    n_w = 0
    for k, v in weights(vae).items():
        assert torch.equal(v.half().float(), v), k
        npz["vae/w/" + k] = v.half().numpy()
        n_w += v.numel()
    meta["keys"]["vae"] = {k: list(v.shape) for k, v in weights(vae).items()}
    meta["vae_weights"] = n_w
    meta["abs_mean"] = {k: float(np.abs(npz[k]).mean()) for k in ("enc/enc_out", "gst/x", "gstvae/x", "gstvae/kl", "vae/x", "vae/kl", "vae/enc_out")}
    meta["kl_min_abs"] = {k: float(np.abs(npz[k]).min()) for k in ("gstvae/kl", "vae/kl")}

    out = os.path.join(HERE, "style_small.npz")
    np.savez_compressed(out, **npz)
    json.dump(meta, open(os.path.join(HERE, "style_meta.json"), "w"), indent=1)
    print(json.dumps(meta["abs_mean"]), meta["kl_min_abs"], n_w, os.path.getsize(out))


if __name__ == "__main__":
    main()
