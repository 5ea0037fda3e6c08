#!/usr/bin/env python3
"""Golden vectors for the VITS2 HiFi-GAN generator (vits2/models.py:900-974 with modules.ResBlock1, modules.py:221-315), produced
by the reference's own models.Generator on CPU.  models.py imports monotonic_align at module level, which Generator never uses:
a stub module stands in for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_generator.py

Writes tests/golden/generator_small.npz + generator_meta.json (reduced dims, weight norm still on, no reference source):
  w{0,4}/<state-dict key>     weights of the generator without / with gin_channels = 4
  x{0,4}/T<T>, g4/T<T>, y{0,4}/T<T>   inputs z [3, C, T] (utterance 1 has zeroed tail frames), speaker rows g [3, 4, 1] and the
                                      reference's waveform [3, 1, T * prod(u)] for T in 1, 2, 9
and in the meta JSON the state-dict key / shape record of models.Generator at the ModelConfig dims (vits2/cli.py:159-180)."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference/vits2"
sys.path.insert(0, REF)
sys.modules.setdefault("monotonic_align", types.ModuleType("monotonic_align"))  # (imported by models.py, unused by Generator)
import models  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = dict(initial_channel=8, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
             upsample_rates=[4, 2], upsample_initial_channel=32, upsample_kernel_sizes=[8, 4])
FULL = dict(initial_channel=192, resblock="1", resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3,
            upsample_rates=[8, 8, 2, 2], upsample_initial_channel=512, upsample_kernel_sizes=[16, 16, 4, 4])


def randomize(gen, seed):
    """Weights that keep every stage's activations O(1) (the reference's init_weights std 0.01 shrinks the signal until any
    layer error hides below the tests' atol): weight_norm gains near 1, plain convs at 1/sqrt(fan_in), biases 0.1 N(0, 1)."""
    gsd = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in gen.named_parameters():
            if n.endswith("weight_g"):
                p.copy_(0.6 + 0.4 * torch.rand(p.shape, generator=gsd))
            elif n.endswith("weight_v") or n.endswith("weight"):
                fan_in = p[0].numel() if not n.startswith("ups") else p.shape[0] * p.shape[2]
                p.copy_(torch.randn(p.shape, generator=gsd) / fan_in**0.5)
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=gsd))


def main():
    out, meta = {}, {"dims": SMALL, "T": [1, 2, 9], "B": 3, "cases": {}}
    for gin in (0, 4):
        torch.manual_seed(11 + gin)
        gen = models.Generator(**SMALL, gin_channels=gin).eval()
        randomize(gen, 100 + gin)
        for k, v in gen.state_dict().items():
            out[f"w{gin}/{k}"] = v.numpy().copy()
        for T in meta["T"]:
            x = torch.randn(3, SMALL["initial_channel"], T)
            if T > 1:
                x[1, :, T // 2 + 1 :] = 0.0  # one utterance with zeroed tail frames
            g = torch.randn(3, gin, 1) if gin else None
            with torch.no_grad():
                y = gen(x, g)
            out[f"x{gin}/T{T}"] = x.numpy()
            if gin:
                out[f"g{gin}/T{T}"] = g.numpy()
            out[f"y{gin}/T{T}"] = y.numpy()
            meta["cases"][f"gin{gin}/T{T}"] = {"sat_frac": float((y.abs() > 0.99).float().mean()), "y_rms": float(y.pow(2).mean().sqrt())}
    full = models.Generator(**FULL, gin_channels=0)
    meta["fulldims"] = FULL
    meta["fulldims_state_dict"] = [[k, list(v.shape)] for k, v in full.state_dict().items()]
    np.savez_compressed(os.path.join(HERE, "generator_small.npz"), **out)
    with open(os.path.join(HERE, "generator_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(json.dumps(meta["cases"]), os.path.getsize(os.path.join(HERE, "generator_small.npz")), "bytes")


if __name__ == "__main__":
    main()
