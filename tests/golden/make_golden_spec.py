#!/usr/bin/env python3
"""Golden vectors for the VITS2 spectrogram front-end: vits2/mel_processing.py:58-187 run by the reference's own code on CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_spec.py <path to the reference's vits2 directory>

The reference's module imports librosa, which is not installed here: stub modules stand in for it, and its ``filters.mel`` returns
the basis this repository uses by default (torch_tts_amd.audio.melscale_fbanks transposed: Slaney scale, area-normalised), so that
the reference's own spec_to_mel_torch / mel_spectrogram_torch lines run on a recorded basis.  No reference text is written here.

Writes tests/golden/spec_small.npz + spec_meta.json:
  basis/<n_fft>                      the mel basis [80, n_fft / 2 + 1] fp32
  c<i>/u<j>/wav                      utterance j of configuration i (n_fft, hop, win in the meta JSON), fp32; three signals: uniform
                                     noise at 0.9 full scale, a 440 Hz sine plus 1 % noise, noise under a t^4 ramp scaled to 0.05
                                     (the 1e-6 floor and the quiet end of the log); ragged lengths that are no multiples of the hop
  c<i>/u<j>/{spec32, mel32}          spectrogram_torch / mel_spectrogram_torch of that utterance ALONE, fp32
  c<i>/u<j>/{spec64, mel64}          the same lines on y.double()
and in the meta JSON per configuration the reference's own fp32-against-fp64 error: ``spec_frame_err`` = max over frames of
max_bins |s32 - s64| / max_bins s64, ``mel_abs_err`` = max |m32 - m64| and ``mel_tol_ratio`` = max |m32 - m64| / (1e-5 + 1e-4 |m64|).
The GPU test's bar for the linear spectrogram is 4 x spec_frame_err."""
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from torch_tts_amd.audio import melscale_fbanks  # noqa: E402

SR, N_MELS, FMIN, FMAX = 22050, 80, 0.0, None
CONFIGS = [dict(n_fft=1024, hop=256, win=1024, lengths=[3700, 2900, 3333]),
           dict(n_fft=256, hop=64, win=256, lengths=[1250, 833, 1001]),
           dict(n_fft=1024, hop=256, win=800, lengths=[3001, 3650, 2777])]


def basis_of(n_fft):
    return melscale_fbanks(n_fft // 2 + 1, FMIN, SR / 2.0, N_MELS, SR).t().contiguous().numpy()


def librosa_mel(sr, n_fft, n_mels, fmin, fmax):
    assert (sr, n_mels, fmin, fmax) == (SR, N_MELS, FMIN, FMAX)
    return basis_of(n_fft)


lib = types.ModuleType("librosa")
lib.util = types.ModuleType("librosa.util")
lib.filters = types.ModuleType("librosa.filters")
lib.filters.mel = librosa_mel
for n in ("normalize", "pad_center", "tiny"):
    setattr(lib.util, n, None)
sys.modules.update({"librosa": lib, "librosa.util": lib.util, "librosa.filters": lib.filters})
spec_ = importlib.util.spec_from_file_location("ref_mel_processing", os.path.join(REF, "mel_processing.py"))
ref = importlib.util.module_from_spec(spec_)
spec_.loader.exec_module(ref)


def signal(kind, n, gen):
    t = torch.arange(n, dtype=torch.float64)
    noise = torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1
    if kind == 0:
        y = 0.9 * noise
    elif kind == 1:
        y = 0.5 * torch.sin(2 * math.pi * 440.0 * t / SR) + 0.01 * noise
    else:
        y = 0.05 * noise * (t / n) ** 4
    return y.to(torch.float32)


out, meta = {}, dict(sampling_rate=SR, n_mels=N_MELS, fmin=FMIN, fmax=FMAX, configs=[])
gen = torch.Generator().manual_seed(20)
for ci, c in enumerate(CONFIGS):
    out[f"basis/{c['n_fft']}"] = basis_of(c["n_fft"])
    e_spec = e_abs = e_tol = 0.0
    for ui, n in enumerate(c["lengths"]):
        y = signal(ui, n, gen)[None]
        res = {}
        for tag, yy in (("32", y), ("64", y.double())):
            ref.mel_basis.clear()  # (the reference keys its caches by fmax / win_size and dtype, not by n_fft)
            ref.hann_window.clear()
            res["spec" + tag] = ref.spectrogram_torch(yy, c["n_fft"], SR, c["hop"], c["win"], center=False)[0]
            res["mel" + tag] = ref.mel_spectrogram_torch(yy, c["n_fft"], N_MELS, SR, c["hop"], c["win"], FMIN, FMAX, center=False)[0]
            m2 = ref.spec_to_mel_torch(res["spec" + tag][None], c["n_fft"], N_MELS, SR, FMIN, FMAX)[0]
            assert torch.equal(m2, res["mel" + tag])
        s32, s64, m32, m64 = res["spec32"].double(), res["spec64"], res["mel32"].double(), res["mel64"]
        e_spec = max(e_spec, float(((s32 - s64).abs().amax(0) / s64.amax(0)).max()))
        e_abs = max(e_abs, float((m32 - m64).abs().max()))
        e_tol = max(e_tol, float(((m32 - m64).abs() / (1e-5 + 1e-4 * m64.abs())).max()))
        out[f"c{ci}/u{ui}/wav"] = y[0].numpy()
        for k, v in res.items():
            out[f"c{ci}/u{ui}/{k}"] = v.numpy()
    meta["configs"].append(dict(n_fft=c["n_fft"], hop=c["hop"], win=c["win"], lengths=c["lengths"], spec_frame_err=e_spec, mel_abs_err=e_abs,
                                mel_tol_ratio=e_tol))
np.savez_compressed(os.path.join(HERE, "spec_small.npz"), **out)
with open(os.path.join(HERE, "spec_meta.json"), "w") as f:
    json.dump(meta, f, indent=1)
print(json.dumps(meta["configs"], indent=1), os.path.getsize(os.path.join(HERE, "spec_small.npz")))
