"""The reference's vits2/mel_processing.py:58-187 on the device: waveforms to the linear or log-mel spectrograms the VITS2
posterior encoder reads, through ``ttsvits_spectrogram`` / ``ttsvits_spec_to_mel`` / ``ttsvits_mel_spectrogram``
(include/ttsdec.h, csrc/spec.hip).

* ``spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center=False)``        -> [B, n_fft / 2 + 1, T]
* ``spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax)``                 -> [B, num_mels, T]
* ``mel_spectrogram_torch(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)``

Same names, positional signatures, layouts and dtype as the reference's.  Keyword-only additions: ``lengths`` ([B], samples per
utterance for the waveform forms, frames for ``spec_to_mel_torch``) - the reference makes every utterance's spectrogram alone
(data_utils.py:86-135), so its reflect padding mirrors at that utterance's own end; with ``lengths`` a padded batch gives the same,
frames past an utterance's count are exact zeros and the functions return ``(spec, spec_lengths)``; and ``mel_basis``
([num_mels, n_fft / 2 + 1]) in place of the default, which is ``audio.melscale_fbanks`` (Slaney scale, area-normalised: what
``librosa.filters.mel`` computes by default - that equality is not pinned here).

fp32 on a ROCm device only; ``center=True``, other dtypes, CPU tensors and an ``n_fft`` outside 256 / 512 / 1024 / 2048 raise
NotImplementedError (there is no fallback); an utterance no longer than the padding, or one too short for a frame, raises
ValueError - found on the host when ``lengths`` is absent or lives there, else through the call's status word (one host read)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .audio import melscale_fbanks

N_FFTS = (256, 512, 1024, 2048)  # what csrc/spec.hip has radix plans for

_windows: Dict[Tuple, torch.Tensor] = {}
_bases: Dict[Tuple, torch.Tensor] = {}


def pad_of(n_fft: int, hop_size: int) -> int:
    """int((n_fft - hop_size) / 2), mel_processing.py:74."""
    return int((n_fft - hop_size) / 2)


def frame_count(n_samples: int, n_fft: int, hop_size: int) -> int:
    """Frames of one utterance: torch.stft(center=False) on the reflect-padded waveform; 0 where the reference raises (the
    reflection needs more samples than the padding, a frame needs n_fft padded samples)."""
    pad = pad_of(n_fft, hop_size)
    if n_samples <= pad or n_samples + 2 * pad < n_fft:
        return 0
    return 1 + (n_samples + 2 * pad - n_fft) // hop_size


def hann(win_size: int, device: torch.device) -> torch.Tensor:
    key = (win_size, str(device))
    if key not in _windows:
        _windows[key] = torch.hann_window(win_size).to(dtype=torch.float32, device=device)  # mel_processing.py:68
    return _windows[key]


def default_mel_basis(n_fft: int, num_mels: int, sampling_rate: int, fmin: float, fmax: Optional[float], device: torch.device) -> torch.Tensor:
    key = (n_fft, num_mels, sampling_rate, fmin, fmax, str(device))
    if key not in _bases:
        fb = melscale_fbanks(n_fft // 2 + 1, float(fmin), float(fmax) if fmax else sampling_rate / 2.0, num_mels, sampling_rate)
        _bases[key] = fb.t().contiguous().to(device)
    return _bases[key]


def _check_wave(y: torch.Tensor, n_fft: int, hop_size: int, win_size: int, center: bool, who: str) -> None:
    if center:
        raise NotImplementedError(f"{who}: center=True is outside the HIP path (no caller in the reference uses it)")
    if not y.is_cuda:
        raise NotImplementedError(f"{who} runs on a ROCm device only: there is no CPU fallback")
    if y.dtype != torch.float32:
        raise NotImplementedError(f"{who} is exact fp32: got {y.dtype}")
    if n_fft not in N_FFTS:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"n_fft = {n_fft}: built for {N_FFTS}")
    if y.dim() != 2:
        raise ValueError(f"{who}: y must be [B, samples], got {tuple(y.shape)}")
    if hop_size < 1 or not 1 <= win_size <= n_fft:
        raise ValueError(f"{who}: hop_size >= 1 and 1 <= win_size <= n_fft expected, got hop_size = {hop_size}, win_size = {win_size}")


def _short(n_fft: int, hop_size: int) -> str:
    return (f"an utterance is no longer than the reflect padding ({pad_of(n_fft, hop_size)} samples) or too short for one frame of "
            f"n_fft = {n_fft}: its spectrogram is undefined")


def _basis(mel_basis, n_fft, num_mels, sampling_rate, fmin, fmax, device) -> torch.Tensor:
    if mel_basis is None:
        return default_mel_basis(n_fft, num_mels, sampling_rate, fmin, fmax, device)
    mb = torch.as_tensor(mel_basis).to(device=device, dtype=torch.float32).contiguous()
    if tuple(mb.shape) != (num_mels, n_fft // 2 + 1):
        raise ValueError(f"mel_basis must be [num_mels, n_fft / 2 + 1] = [{num_mels}, {n_fft // 2 + 1}], got {tuple(mb.shape)}")
    return mb


def _wave_to_spec(y, n_fft, hop_size, win_size, lengths, basis, who):
    """The shared body of the two waveform forms -> (out [B, rows, T], spec_lengths [B] int64 on the device or None)."""
    from . import vits2

    dev = y.device
    B, N = y.shape
    T = frame_count(N, n_fft, hop_size)
    if B < 1 or T < 1:
        raise ValueError(f"{who}: " + (_short(n_fft, hop_size) if B else "an empty batch"))
    on_device = isinstance(lengths, torch.Tensor) and lengths.is_cuda
    lens_dev = spec_lengths = None
    if lengths is not None and not on_device:  # on the host: checked here, no status read
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(v > N for v in host):
            raise ValueError(f"{who}: lengths must be [B] = [{B}] sample counts of at most {N}, got {host}")
        counts = [frame_count(v, n_fft, hop_size) for v in host]
        if min(counts) < 1:
            raise ValueError(f"{who}: " + _short(n_fft, hop_size))
        lens_dev = torch.tensor(host, dtype=torch.int32).to(dev)
        spec_lengths = torch.tensor(counts, dtype=torch.int64).to(dev)
    elif on_device:
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"{who}: lengths must be [B] = [{B}], got {tuple(lengths.shape)}")
        lens_dev = lengths.to(device=dev, dtype=torch.int32).contiguous()
        spec_lengths = 1 + torch.div(lens_dev.to(torch.int64) + (2 * pad_of(n_fft, hop_size) - n_fft), hop_size, rounding_mode="floor")
    eng = vits2._align_engine(dev)
    out = eng.spectrogram(y.detach().contiguous(), lens_dev, hann(win_size, dev), n_fft, hop_size, T, basis, check=on_device)
    return out, spec_lengths


def spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center=False, *, lengths=None):
    """mel_processing.spectrogram_torch: y [B, samples] -> sqrt(re^2 + im^2 + 1e-6) of the Hann-windowed STFT of y reflect-padded by
    int((n_fft - hop_size) / 2), [B, n_fft / 2 + 1, T]; with ``lengths`` -> (spec, spec_lengths)."""
    _check_wave(y, n_fft, hop_size, win_size, center, "spectrogram_torch")
    spec, spec_lengths = _wave_to_spec(y, n_fft, hop_size, win_size, lengths, None, "spectrogram_torch")
    return spec if lengths is None else (spec, spec_lengths)


def spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax, *, mel_basis=None, lengths=None):
    """mel_processing.spec_to_mel_torch: spec [B, n_fft / 2 + 1, T] -> log(clamp(mel_basis @ spec, 1e-5)) [B, num_mels, T]; with
    ``lengths`` (frames per utterance) frames past them are zeros and the result is (mel, lengths)."""
    from . import vits2

    who = "spec_to_mel_torch"
    if not spec.is_cuda:
        raise NotImplementedError(f"{who} runs on a ROCm device only: there is no CPU fallback")
    if spec.dtype != torch.float32:
        raise NotImplementedError(f"{who} is exact fp32: got {spec.dtype}")
    if n_fft not in N_FFTS:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"n_fft = {n_fft}: built for {N_FFTS}")
    if spec.dim() != 3 or spec.shape[1] != n_fft // 2 + 1 or spec.shape[0] < 1 or spec.shape[2] < 1:
        raise ValueError(f"{who}: spec must be [B, n_fft / 2 + 1, T] = [B, {n_fft // 2 + 1}, T], got {tuple(spec.shape)}")
    dev = spec.device
    basis = _basis(mel_basis, n_fft, num_mels, sampling_rate, fmin, fmax, dev)
    frames = None if lengths is None else torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    mel = vits2._align_engine(dev).spec_to_mel(spec.detach().contiguous(), frames, n_fft, basis)
    return mel if lengths is None else (mel, frames.to(torch.int64))


def mel_spectrogram_torch(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, *, mel_basis=None, lengths=None):
    """mel_processing.mel_spectrogram_torch: y [B, samples] -> log-mel [B, num_mels, T] in one kernel (the linear spectrogram stays on
    the chip); with ``lengths`` -> (mel, spec_lengths)."""
    _check_wave(y, n_fft, hop_size, win_size, center, "mel_spectrogram_torch")
    basis = _basis(mel_basis, n_fft, num_mels, sampling_rate, fmin, fmax, y.device)
    mel, spec_lengths = _wave_to_spec(y, n_fft, hop_size, win_size, lengths, basis, "mel_spectrogram_torch")
    return mel if lengths is None else (mel, spec_lengths)
