#!/usr/bin/env python3
"""Golden vectors for the VITS2 validation step: SynthesizerTrn.forward as a whole (vits2/models.py:1214-1286) and the loss terms of
train.py:357-418 (loss_mel, loss_kl, loss_dur), produced by the reference's own models.py, losses.py, commons.py and
mel_processing.py on CPU in eval mode.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_evalstep.py <path to the reference's vits2 directory>

monotonic_align is the reference's core.pyx compiled by pyximport in a temporary directory, as make_golden_align.py does; librosa,
which the reference's mel_processing imports and which is not installed here, is the stub of make_golden_spec.py: its
``filters.mel`` returns the recorded basis (torch_tts_amd.audio.melscale_fbanks transposed).  Nothing compiled and no reference
text is written here.

The model is durnll_meta.json's ``net`` at sizes at which the mel of a generated segment exists: the generator's hop is 8
(upsample_rates [4, 2]); with n_fft = win = 256 the reflection pad is 124 samples, so segment_size = 128 samples = 16 frames is the
smallest multiple of the hop above it.  n_mels = 16.  Four utterances of 40 / 16 / 33 / 25 frames (one exactly a segment, one the
full width) of 9 / 6 / 3 / 1 tokens; each utterance's waveform is 8 samples per frame, uniform noise at half scale, zeros past its
length, and its spectrogram is the reference's of that utterance alone.

Writes tests/golden/evalstep_small.npz + evalstep_meta.json:
  basis                                   the mel basis [16, 129] fp32
  <model>/{x, x_lengths, spec, y_lengths, sid, wav}   the inputs of model_mel (spec_channels 16: a mel posterior encoder, SDP, no
                                          speakers) and model_lin (spec_channels 129: the linear spectrogram, a plain duration
                                          predictor, 3 speakers)
  <model>/{e_post, e_q, e_w, u}           every draw: the posterior's randn_like, the SDP's two torch.randn(B, 2, T_x) (model_mel), and
                                          the torch.rand([B]) of rand_slice_segments
  <model>/{o, l_length, attn, ids_slice, x_mask, y_mask, z, z_p, m_p, logs_p, m_q, logs_q, hidden_x, logw, logw_}
                                          the eight results of net_g(x, x_lengths, spec, y_lengths, sid=sid); attn as int8
  <model>/{y_mel, y_hat_mel, loss_mel, loss_kl, loss_dur}   train.py:357-369 and F.l1_loss(y_mel, y_hat_mel), losses.kl_loss(z_p, logs_q,
                                          m_p, logs_p, z_mask), l_length.sum() - without c_mel / c_kl
  <model>/{loss_mel64, loss_kl64, loss_dur64}   the same from the same modules after .double() on the same draws, and what the tests'
                                          fp64 restatement starts from: {z_p64, logs_q64, m_pu64, logs_pu64 (the text encoder's
                                          unexpanded prior), m_p64, logs_p64 (expanded), mel64, y_hat_mel64}
and in the meta JSON the seeds and checksums of every weight and the yardstick of the GPU tests' bar: each loss's fp32-against-fp64
error |a - b| / (0.1 + |b|).  The weights are redrawn (next seed; every seed tried is recorded with its figures) until each is
<= 2.5e-5 - the GPU bar of 1e-4 is then at least 4 x the reference's own error, the convention of align_meta.json and
durnll_meta.json - until the reference's own fp32 z, z_p, m_p, logs_p, m_q, logs_q and o lie within a quarter of the tests' bar on
those tensors, max |a - b| / (1e-5 + 1e-4 |b|) <= 0.25 (durnll_meta.json's c192_t150_g4: an element the reference's own fp32 cannot
hold says nothing about a kernel), and until the fp64 model's own search finds the fp32 model's path (a path that holds in both has
no near-tie a third evaluation order could fall the other side of: the tests compare attn for equality).
The posterior encoder's last conv, enc_q.proj, is scaled by 0.25 after make_golden_duration.randomize, weight and bias (recorded as
``enc_q_proj_scale``; the checksums are those of the scaled weights, and tests/test_evalstep_host.eval_net scales the same way):
randomize's unit-variance proj on a real spectrogram's values gives logs_q up to +-6 and z = m_q + e exp(logs_q) up to 1000, where
the flow's z_p is a small difference of large numbers: the reference's own fp32 z_p was then at 0.23 - 1.6 of the bar against its
fp64 self over the first eight seeds of model_lin (1.56 at model_mel's first), and none of 50 seeds had every tensor within a
quarter; scaled, logs_q stays within +-1.5 as a trained posterior's does, and the reference is at 0.13 of the bar."""
import copy
import hashlib
import importlib.util
import json
import os
import shutil
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_align as A  # noqa: E402  (the monotonic_align stand-in, NET; imports the reference's models)
from make_golden_duration import checksum, randomize  # noqa: E402
from torch_tts_amd.audio import melscale_fbanks  # noqa: E402

models = A.models
import commons  # noqa: E402  (the reference's, from the path make_golden_align put first)
import losses  # noqa: E402

N_FFT, HOP, WIN, SR, N_MELS, FMIN, FMAX = 256, 8, 256, 22050, 16, 0.0, None
SEG_FRAMES = 16
AUDIO = dict(n_fft=N_FFT, hop_size=HOP, win_size=WIN, sampling_rate=SR, n_mels=N_MELS, fmin=FMIN, fmax=FMAX, segment_size=SEG_FRAMES * HOP)
BASIS = melscale_fbanks(N_FFT // 2 + 1, FMIN, SR / 2.0, N_MELS, SR).t().contiguous().numpy()

lib = types.ModuleType("librosa")
lib.util = types.ModuleType("librosa.util")
lib.filters = types.ModuleType("librosa.filters")
lib.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: BASIS
for n in ("normalize", "pad_center", "tiny"):
    setattr(lib.util, n, None)
sys.modules.update({"librosa": lib, "librosa.util": lib.util, "librosa.filters": lib.filters})
spec_ = importlib.util.spec_from_file_location("ref_mel_processing", os.path.join(A.REF, "mel_processing.py"))
mp = importlib.util.module_from_spec(spec_)
spec_.loader.exec_module(mp)

YARD_MAX = 2.5e-5
RATIO_MAX = 0.25
ENC_Q_PROJ_SCALE = 0.25  # on enc_q.proj after randomize (see the module's docstring)
TENSORS = ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q", "o")  # what the GPU tests compare at rtol 1e-4 / atol 1e-5
PARTS = ("enc_p", "enc_q", "flow", "dp", "dec", "emb_g")
B, T_X, T_Y = 4, 9, 40
X_LENGTHS, Y_LENGTHS = [9, 6, 3, 1], [40, 16, 33, 25]
out = {}


def tol_ratio(a, b):
    """The reference's own fp32 tensor against the same module in fp64, as a fraction of the GPU tests' bar on the tensors:
    max |a - b| / (ATOL + RTOL |b|) with RTOL, ATOL = 1e-4, 1e-5."""
    return float(((a.double() - b).abs() / (1e-5 + 1e-4 * b.abs())).max())


def rel(a, b):
    return float(((a.double() - b.double()).abs() / (0.1 + b.double().abs())).max())


class Draws:
    """Records what torch.randn / randn_like / rand return inside the reference's code, or replays a recorded list in the dtype
    asked for."""

    def __init__(self, replay=None):
        self.draws, self.replay = [], None if replay is None else list(replay)

    def _wrap(self, real, like):
        def fn(*a, **k):
            if self.replay is not None:
                r = self.replay.pop(0)
                r = r.to(a[0].dtype) if like else r
                assert tuple(r.shape) == tuple(a[0].shape if like else real(*a, **k).shape)
                return r.clone()
            r = real(*a, **k)
            self.draws.append(r.clone())
            return r
        return fn

    def __enter__(self):
        self._real = (torch.randn, torch.randn_like, torch.rand)
        torch.randn, torch.randn_like, torch.rand = self._wrap(torch.randn, False), self._wrap(torch.randn_like, True), self._wrap(torch.rand, False)
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like, torch.rand = self._real


def step(net, x, x_lengths, spec, y_lengths, sid, wav, mel_posterior, draws=None):
    """train.py:341-369 and 416-418 without the coefficients -> (a dict of everything computed, the draws)."""
    got = {}
    hook = net.enc_p.register_forward_hook(lambda m, i, o: got.update(m_pu=o[1], logs_pu=o[2]))
    try:
        with torch.no_grad(), Draws(draws) as rec:
            (o, l_length, attn, ids_slice, x_mask, z_mask, (z, z_p, m_p, logs_p, m_q, logs_q), (hidden_x, logw, logw_)) = net(
                x, x_lengths, spec, y_lengths, sid=sid)
    finally:
        hook.remove()
    with torch.no_grad():
        mel = spec if mel_posterior else mp.spec_to_mel_torch(spec, N_FFT, N_MELS, SR, FMIN, FMAX)
        y_mel = commons.slice_segments(mel, ids_slice, SEG_FRAMES)
        y_hat_mel = mp.mel_spectrogram_torch(o.squeeze(1), N_FFT, N_MELS, SR, HOP, WIN, FMIN, FMAX)
        y = commons.slice_segments(wav, ids_slice * HOP, SEG_FRAMES * HOP)
        got.update(o=o, l_length=l_length, attn=attn, ids_slice=ids_slice, x_mask=x_mask, y_mask=z_mask, z=z, z_p=z_p, m_p=m_p, logs_p=logs_p,
                   m_q=m_q, logs_q=logs_q, hidden_x=hidden_x, logw=logw, logw_=logw_, mel=mel, y_mel=y_mel, y_hat_mel=y_hat_mel, y=y,
                   loss_dur=torch.sum(l_length.float() if l_length.dtype == torch.float32 else l_length),
                   loss_mel=F.l1_loss(y_mel, y_hat_mel), loss_kl=losses.kl_loss(z_p, logs_q, m_p, logs_p, z_mask))
    return got, rec.draws


def inputs(name, spec_channels, n_speakers, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, A.NET["n_vocab"], (B, T_X), generator=gen)
    wav = torch.zeros(B, 1, T_Y * HOP)
    spec = torch.zeros(B, spec_channels, T_Y)
    for b, t in enumerate(Y_LENGTHS):
        wav[b, 0, :t * HOP] = 0.5 * (2 * torch.rand(t * HOP, generator=gen) - 1)
        own = wav[b, :, :t * HOP]
        s = (mp.mel_spectrogram_torch(own, N_FFT, N_MELS, SR, HOP, WIN, FMIN, FMAX) if spec_channels == N_MELS else
             mp.spectrogram_torch(own, N_FFT, SR, HOP, WIN))
        assert s.shape == (1, spec_channels, t)
        spec[b, :, :t] = s[0]
    sid = torch.tensor([0, 2, 1, 1]) if n_speakers else None
    return x, torch.tensor(X_LENGTHS), spec, torch.tensor(Y_LENGTHS), sid, wav


def model_case(meta, name, use_sdp, n_speakers, spec_channels, seed0):
    gin = 4 if n_speakers else 0
    net_dims = dict(A.NET, spec_channels=spec_channels, segment_size=SEG_FRAMES)
    x, x_lengths, spec, y_lengths, sid, wav = inputs(name, spec_channels, n_speakers, seed0)
    mel_posterior = spec_channels == N_MELS
    tried = {}
    for seed in range(seed0, seed0 + 5000, 100):
        torch.manual_seed(seed)
        net = models.SynthesizerTrn(**net_dims, n_speakers=n_speakers, gin_channels=gin, use_sdp=use_sdp).eval()
        seeds = {part: 1000 * seed + len(part) for part in PARTS if hasattr(net, part)}
        for part, s in seeds.items():
            randomize(getattr(net, part), s)
        with torch.no_grad():
            net.enc_q.proj.weight.mul_(ENC_Q_PROJ_SCALE)
            net.enc_q.proj.bias.mul_(ENC_Q_PROJ_SCALE)
        torch.manual_seed(seed + 1)
        r32, draws = step(net, x, x_lengths, spec, y_lengths, sid, wav, mel_posterior)
        r64, _ = step(copy.deepcopy(net).double(), x, x_lengths, spec.double(), y_lengths, sid, wav.double(), mel_posterior, draws)
        errs = {k: rel(r32[k], r64[k]) for k in ("loss_mel", "loss_kl", "loss_dur")}
        same_path = bool(torch.equal(r32["attn"].double(), r64["attn"]))
        ratios = {k: tol_ratio(r32[k], r64[k]) for k in TENSORS}
        tried[str(seed)] = [errs["loss_mel"], errs["loss_kl"], errs["loss_dur"], same_path, max(ratios.values())]
        if max(errs.values()) <= YARD_MAX and same_path and max(ratios.values()) <= RATIO_MAX:
            break
    else:
        raise RuntimeError("no weights within the yardstick")
    assert torch.equal(r32["ids_slice"], r64["ids_slice"])
    # the posterior's randn_like, then (SDP) the likelihood's and the reverse pass's torch.randn(B, 2, T_x), then the slice's torch.rand([B])
    assert len(draws) == (4 if use_sdp else 2) and draws[0].shape == (B, A.NET["inter_channels"], T_Y) and draws[-1].shape == (B,)
    rec = dict(x=x, x_lengths=x_lengths, spec=spec, y_lengths=y_lengths, wav=wav, e_post=draws[0], u=draws[-1])
    if use_sdp:
        rec["e_q"], rec["e_w"] = draws[1], draws[2]
    if sid is not None:
        rec["sid"] = sid
    for k in ("o", "l_length", "ids_slice", "x_mask", "y_mask", "z", "z_p", "m_p", "logs_p", "m_q", "logs_q", "hidden_x", "logw", "logw_", "y_mel",
              "y_hat_mel", "loss_mel", "loss_kl", "loss_dur"):
        rec[k] = r32[k]
    rec["attn"] = r32["attn"].to(torch.int8)
    for k in ("loss_mel", "loss_kl", "loss_dur", "z_p", "logs_q", "m_pu", "logs_pu", "m_p", "logs_p", "mel", "y_hat_mel"):
        rec[k + "64"] = r64[k]
    for k, v in rec.items():
        out[f"{name}/{k}"] = v.numpy()
    assert r32["ids_slice"].tolist() == (draws[-1] * (y_lengths - SEG_FRAMES + 1)).long().tolist()
    assert r32["o"].shape == (B, 1, SEG_FRAMES * HOP) and r32["y_hat_mel"].shape == r32["y_mel"].shape == (B, N_MELS, SEG_FRAMES)
    meta["models"][name] = dict(use_sdp=use_sdp, n_speakers=n_speakers, gin_channels=gin, spec_channels=spec_channels, input_seed=seed0, seeds=seeds,
                                checksums={part: checksum(getattr(net, part)) for part in seeds}, cpu_f32_err=errs, cpu_f32_tol_ratio=ratios,
                                tol_ratio_max=RATIO_MAX, tried=tried,
                                ids_slice=r32["ids_slice"].tolist(),
                                losses={k: float(r32[k]) for k in ("loss_mel", "loss_kl", "loss_dur")},
                                losses64={k: float(r64[k]) for k in ("loss_mel", "loss_kl", "loss_dur")})


def main():
    meta = {"net": dict(A.NET, segment_size=SEG_FRAMES), "audio": AUDIO, "yardstick_max": YARD_MAX, "enc_q_proj_scale": ENC_Q_PROJ_SCALE, "x_lengths": X_LENGTHS, "y_lengths": Y_LENGTHS,
            "torch": torch.__version__, "threads": torch.get_num_threads(), "models": {}}
    out["basis"] = BASIS
    model_case(meta, "model_mel", True, 0, N_MELS, 210)
    model_case(meta, "model_lin", False, 3, N_FFT // 2 + 1, 220)
    path = os.path.join(HERE, "evalstep_small.npz")
    np.savez_compressed(path, **out)
    meta["npz_sha256"] = hashlib.sha256(open(path, "rb").read()).hexdigest()
    with open(os.path.join(HERE, "evalstep_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(os.path.getsize(path), "bytes", json.dumps({n: (m["cpu_f32_err"], len(m["tried"])) for n, m in meta["models"].items()}))
    shutil.rmtree(A.TMP, ignore_errors=True)


if __name__ == "__main__":
    main()
