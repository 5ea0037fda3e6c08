#!/usr/bin/env python3
"""Golden vectors for the VITS2 duration discriminators (vits2/models.py:183-329), produced by the reference's own
models.DurationDiscriminatorV1 / DurationDiscriminatorV2 on CPU, with the GAN terms of vits2/losses.py:16-34 on their outputs as
train.py:394 / 424 takes them.  models.py imports monotonic_align at module level, which the discriminators never use: a stub
module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_durdisc.py

The weights are never stored: both sides fill them with tests/recipes.py fill_by_key(module, SEED, gain=GAIN).  GAIN was chosen on
the CPU so that the reference's pre-sigmoid logits stay within about +-8 (a saturated sigmoid would hide errors); the observed
range goes into the meta file.  Writes tests/golden/durdisc_small.npz + durdisc_meta.json, per case <c> and version <v>:
  x/<c>, dur_r/<c>, dur_hat/<c>       the inputs [B, C, T] / [B, 1, T] (shared by the versions); the lengths are in the meta file
  trunk/<c>/v<v>                      forward's x in front of its loop over the durations [B, F, T] (elements at the case's
                                      stride of the flattened tensor; stride 1 = in full)
  prob_r, prob_hat, logit_r, logit_hat /<c>/v<v>   both outputs [B, T, 1] and the inputs of the Sigmoid (forward hook on
                                      output_layer[0])
and in the meta JSON the loss values and each class's state-dict key / shape record."""
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

SEED, GAIN = 47, 1.2
# name -> in_channels, filter_channels, T, lengths, stride of the stored trunk samples
CASES = {"c24f40": (24, 40, 9, [9, 4], 1), "c192": (192, 192, 37, [37, 20, 1], 7)}


def inputs(name, C, T, lengths):
    """x ~ N(0, 1); dur_r = log(integer durations 1 .. 7) as logw_ is; dur_hat ~ N(0.8, 0.7) as a predictor's logw might be."""
    B, s = len(lengths), sum(ord(c) for c in name)
    x = recipes.seeded_randn(3000 + s, B, C, T)
    dur_r = torch.log(recipes.seeded_ids(4000 + s, 8, B, 1, T, low=1).float())
    dur_hat = 0.8 + 0.7 * recipes.seeded_randn(5000 + s, B, 1, T)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).unsqueeze(1).float()
    return x, mask, dur_r * mask, dur_hat


def main():
    out, meta = {}, {"seed": SEED, "gain": GAIN, "cases": {}, "state_dict": {}}
    lo, hi = 0.0, 0.0
    for name, (C, F, T, lengths, stride) in CASES.items():
        x, mask, dur_r, dur_hat = inputs(name, C, T, lengths)
        out[f"x/{name}"], out[f"dur_r/{name}"], out[f"dur_hat/{name}"] = x.numpy(), dur_r.numpy(), dur_hat.numpy()
        case = {"in_channels": C, "filter_channels": F, "T": T, "lengths": lengths, "trunk_stride": stride}
        for v, cls in ((1, models.DurationDiscriminatorV1), (2, models.DurationDiscriminatorV2)):
            net = cls(C, F, 3, 0.1, gin_channels=0).eval()
            recipes.fill_by_key(net, SEED, gain=GAIN)
            meta["state_dict"][f"v{v}/{name}"] = [[k, list(t.shape)] for k, t in net.state_dict().items()]
            logits, trunk = [], []
            h1 = net.output_layer[0].register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
            h2 = net.pre_out_conv_1.register_forward_hook(lambda m, i, o: trunk.append(i[0].detach().clone()))
            with torch.no_grad():
                res = net(x, mask, dur_r, dur_hat)
                loss_r, loss_g = losses.discriminator_loss(res[0], res[1])
                loss_gen = losses.generator_loss(res[1])
            h1.remove()
            h2.remove()
            p_r, p_hat = (res[0], res[1]) if v == 1 else (res[0][0], res[1][0])
            # pre_out_conv_1 reads cat([h, dur_proj(dur)]) * mask: its first F channels at UNMASKED tokens are h; h itself is not
            # an output of the reference's forward, so it is rebuilt here from the module's own layers
            with torch.no_grad():
                h = net.conv_1(x * mask)
                if v == 2:
                    h = net.norm_1(torch.relu(h))
                h = net.conv_2(h * mask)
                if v == 2:
                    h = net.norm_2(torch.relu(h))
            assert torch.equal(trunk[0][:, :F] * mask, h * mask)
            out[f"trunk/{name}/v{v}"] = h.reshape(-1)[::stride].numpy().copy()
            for key, t in (("prob_r", p_r), ("prob_hat", p_hat), ("logit_r", logits[0]), ("logit_hat", logits[1])):
                assert tuple(t.shape) == (len(lengths), T, 1)
                out[f"{key}/{name}/v{v}"] = t.numpy()
            lo, hi = min(lo, float(min(l.min() for l in logits))), max(hi, float(max(l.max() for l in logits)))
            case[f"v{v}"] = {"discriminator_loss": [loss_r.tolist(), loss_g.tolist()], "generator_loss": loss_gen.tolist(),
                             "n_params": sum(p.numel() for p in net.parameters())}
        meta["cases"][name] = case
    meta["logit_range"] = [lo, hi]
    np.savez_compressed(os.path.join(HERE, "durdisc_small.npz"), **out)
    with open(os.path.join(HERE, "durdisc_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("logit range", lo, hi, os.path.getsize(os.path.join(HERE, "durdisc_small.npz")), "bytes")


if __name__ == "__main__":
    main()
