#!/usr/bin/env python3
"""Golden vectors for the VITS2 waveform discriminators (vits2/models.py:977-1110) and the three GAN terms of vits2/losses.py:7-34,
produced by the reference's own models.MultiPeriodDiscriminator on CPU.  models.py imports monotonic_align at module level, which
the discriminators never use: a stub module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_disc.py

The widths are hard-coded in the reference (46 747 132 parameters), so the weights are never stored: both sides fill them with
tests/recipes.py fill_by_key(module, SEED, gain=1.2).  Writes tests/golden/disc_small.npz + disc_meta.json:
  y/T<T>, y_hat/T<T>                  the inputs [B, 1, T]
  score_r/T<T>/<d>, score_g/T<T>/<d>  every score of discriminator d, in full
  fmap_r/T<T>/<d>/<l>, fmap_g/...     feature map l of discriminator d: the elements at STRIDE of the flattened tensor
and in the meta JSON each feature map's shape and fp64 mean absolute value, the three loss values, and the state-dict key / shape
record of models.MultiPeriodDiscriminator."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/vits2"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.modules.setdefault("monotonic_align", types.ModuleType("monotonic_align"))  # (imported by models.py, unused here)
import losses  # noqa: E402
import models  # noqa: E402
import recipes  # noqa: E402

SEED, GAIN = 31, 1.2
STRIDE = 13  # coprime to 2 * 3 * 5 * 7 * 11: the samples walk every period's columns and every channel
CASES = {2310: 1, 97: 2}  # T -> B (one row at 2310 keeps the file below the 1 MiB a committed fixture may take)


def main():
    mpd = models.MultiPeriodDiscriminator().eval()
    recipes.fill_by_key(mpd, SEED, gain=GAIN)
    out = {}
    meta = {"seed": SEED, "gain": GAIN, "stride": STRIDE, "cases": {},
            "n_params": sum(p.numel() for p in mpd.parameters()),
            "state_dict": [[k, list(v.shape)] for k, v in mpd.state_dict().items()]}
    for T, B in CASES.items():
        y, y_hat = recipes.seeded_randn(1000 + T, B, 1, T), recipes.seeded_randn(2000 + T, B, 1, T)
        with torch.no_grad():
            s_r, s_g, f_r, f_g = mpd(y, y_hat)
            loss_fm = losses.feature_loss(f_r, f_g)
            loss_dr, loss_dg = losses.discriminator_loss(s_r, s_g)
            loss_gen = losses.generator_loss(s_g)
        out[f"y/T{T}"], out[f"y_hat/T{T}"] = y.numpy(), y_hat.numpy()
        case = {"B": B, "fmaps": {}, "feature_loss": float(loss_fm), "discriminator_loss": [loss_dr.tolist(), loss_dg.tolist()],
                "generator_loss": loss_gen.tolist()}
        for side, scores, fmaps in (("r", s_r, f_r), ("g", s_g, f_g)):
            for d, (s, fm) in enumerate(zip(scores, fmaps)):
                out[f"score_{side}/T{T}/{d}"] = s.numpy()
                for l, f in enumerate(fm):
                    out[f"fmap_{side}/T{T}/{d}/{l}"] = f.reshape(-1)[::STRIDE].numpy().copy()
                    case["fmaps"][f"{side}/{d}/{l}"] = {"shape": list(f.shape), "mean_abs": float(f.double().abs().mean())}
        meta["cases"][f"T{T}"] = case
    np.savez_compressed(os.path.join(HERE, "disc_small.npz"), **out)
    with open(os.path.join(HERE, "disc_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(meta["n_params"], os.path.getsize(os.path.join(HERE, "disc_small.npz")), "bytes")


if __name__ == "__main__":
    main()
