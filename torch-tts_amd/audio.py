"""Mel -> waveform step after the decoder path: the inference half of the reference's
``AudioFrontend`` (tacotron/data/audio.py:25-76: ``mel_inv``, ``decode``), ``m_rev`` (data/dataset.py:183-184)
and ``synth_audio`` (inference.py:13-22).

The reference builds these from torchaudio (``InverseMelScale``, ``GriffinLim``, ``DB_to_amplitude``,
``amplitude_to_DB``; torchaudio >= 2.2.1 per tacotron/requirements.txt), which is not installed here, so the
published algorithms are restated on plain torch ops and run on whatever device the tensors live on (FFTs go
to rocFFT through ``torch.stft`` / ``torch.istft``): this step is I/O + FFT, there is no hand-written kernel
in those.  PARITY UNPINNED against torchaudio itself: without it no reference vectors can be produced, and the
reference's Griffin-Lim starts from a random phase (``rand_init=True``); tests check the algebraic properties instead.

The same step as HIP kernels, batched and length-aware (include/ttsdec.h ttsdec_mel_to_magnitude / ttsdec_griffinlim,
csrc/griffinlim.hip): ``AudioFrontend.mel_to_magnitude``, ``griffinlim_native`` and ``synth_audio_native``.  ROCm-only,
exact fp32, no fallback.  With the initial phase an explicit input the algorithm is deterministic, and what is pinned
(tests/test_griffinlim_hip.py) is parity with the published algorithm as the functions above state it, run in fp64.

The analysis half, ``AudioFrontend.encode`` (data/audio.py:55-67: peak normalisation, ``Spectrogram(power=2, normalized=True)``,
``MelScale``, ``amplitude_to_DB``), is restated on torch ops in the same way (no resampling), and runs as HIP kernels on a padded
batch through ``AudioFrontend.encode_native`` (ttsdec_mel_analysis, csrc/analysis.hip; tests/test_analysis_hip.py).

Its first line, ``resample(wave, orig_freq=sr, new_freq=config.sample_rate)`` (data/audio.py:55-58), is ``resample`` here (torchaudio's
``functional.resample`` with its defaults, restated on torch ops: the oracle when run in fp64) and ``resample_native`` on HIP
(ttsdec_resample, csrc/resample.hip; tests/test_resample_hip.py); ``encode_native(..., sr=...)`` chains the two calls on the device,
and ``xref_native`` gives the ``xref`` / ``xref_lengths`` pair of ``Tacotron.forward`` from a reference waveform at any rate."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib


@dataclass
class AudioFrontendConfig:  # data/audio.py:9-22
    sample_rate: int = 16000
    hop_length: int = 256
    win_length: int = 768
    num_mels: int = 80
    fmin: int = 50
    fmax: int = 7600

    def from_json(self, json):
        for key in json:
            self.__setattr__(key, json[key])
        return self


def m_fwd(x):  # data/dataset.py:179-180
    return torch.clip((x + 100) / 100, min=0)


def m_rev(x):  # data/dataset.py:183-184
    return (x * 100) - 100


def _hz_to_mel_slaney(f: float) -> float:
    f_sp = 200.0 / 3
    if f < 1000.0:
        return f / f_sp
    return 1000.0 / f_sp + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _mel_to_hz_slaney(m: torch.Tensor) -> torch.Tensor:
    f_sp = 200.0 / 3
    min_log_mel = 1000.0 / f_sp
    logstep = math.log(6.4) / 27.0
    return torch.where(m >= min_log_mel, 1000.0 * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """Triangular mel filterbank [n_freqs, n_mels], Slaney scale and Slaney area normalisation
    (what MelScale / InverseMelScale(mel_scale="slaney", norm="slaney") use, data/audio.py:34-51)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(_hz_to_mel_slaney(f_min), _hz_to_mel_slaney(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = _mel_to_hz_slaney(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.minimum(down, up), min=0.0)
    fb = fb * (2.0 / (f_pts[2 : n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb.to(torch.float32)


def db_to_amplitude(x: torch.Tensor, ref: float, power: float) -> torch.Tensor:
    return ref * torch.pow(torch.pow(10.0, 0.1 * x), power)


def amplitude_to_db(x: torch.Tensor, multiplier: float, amin: float, db_multiplier: float) -> torch.Tensor:
    return multiplier * torch.log10(torch.clamp(x, min=amin)) - multiplier * db_multiplier


def griffinlim(specgram: torch.Tensor, n_fft: int, hop_length: int, win_length: int, power: float = 2.0, n_iter: int = 32,
               momentum: float = 0.99, rand_init: bool = True, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Fast Griffin-Lim (Perraudin et al. 2013) as in torchaudio.functional.griffinlim: specgram [..., n_freqs, frames]
    (power spectrogram for power=2) -> waveform [..., time]."""
    window = torch.hann_window(win_length, device=specgram.device, dtype=specgram.dtype)
    shape = specgram.shape
    spec = specgram.reshape(-1, shape[-2], shape[-1]).pow(1.0 / power)
    mom = momentum / (1 + momentum)
    if rand_init:
        re = torch.rand(spec.shape, generator=generator, device=spec.device if generator is None or generator.device.type != "cpu" else "cpu")
        im = torch.rand(spec.shape, generator=generator, device=re.device)
        angles = torch.complex(re, im).to(spec.device)
    else:
        angles = torch.full(spec.shape, 1.0, dtype=torch.complex64, device=spec.device)
    tprev = torch.zeros_like(angles)
    for _ in range(n_iter):
        inverse = torch.istft(spec * angles, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window)
        rebuilt = torch.stft(inverse, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=True,
                             pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * mom
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    wave = torch.istft(spec * angles, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window)
    return wave.reshape(shape[:-2] + wave.shape[-1:])


def _resample_plan(orig_freq: int, new_freq: int, lowpass_filter_width: int, rolloff: float, who: str):
    """(o, n, base, width, taps) of a rate pair: o / n the rates over their gcd, base = min(o, n) * rolloff the cutoff, width =
    ceil(lowpass_filter_width * o / base), taps = 2 * width + o."""
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"{who}: the rates must be positive integers, got {orig_freq} -> {new_freq}")
    if int(lowpass_filter_width) != lowpass_filter_width or lowpass_filter_width < 1:
        raise ValueError(f"{who}: lowpass_filter_width must be an integer >= 1, got {lowpass_filter_width}")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"{who}: rolloff must be in (0, 1], got {rolloff}")
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    return o, n, base, width, 2 * width + o


def resample(wave: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.resample with its defaults (``sinc_interp_hann``): wave [..., time] -> [..., ceil(n * time / o)], on
    wave's device in wave's dtype.  The polyphase kernel [n, taps] is evaluated in fp64 and rounded once to that dtype; the filter is a
    conv1d of stride o with n output channels, interleaved.  Equal rates return the input as it is."""
    o, n, base, width, taps = _resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, "resample")
    if o == n:
        return wave
    if not wave.is_floating_point():
        raise TypeError(f"resample: wave must be floating point, got {wave.dtype}")
    lpw = lowpass_filter_width
    idx = torch.arange(-width, width + o, dtype=torch.float64, device=wave.device)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64, device=wave.device)[:, None, None] / n + idx
    t = (t * base).clamp(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    kernel = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * (window * (base / o))
    kernel = kernel.to(wave.dtype)
    shape = wave.shape
    x = wave.reshape(-1, shape[-1])
    x = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(x[:, None], kernel, stride=o)  # [rows, n, blocks]
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[..., : -(-n * shape[-1] // o)]
    return y.reshape(shape[:-1] + y.shape[-1:])


class AudioFrontend:
    """data/audio.py's AudioFrontend: ``encode`` (waveform -> linear dB and mel dB), ``mel_inv`` (mel dB -> linear dB) and ``decode``
    (linear dB -> waveform by Griffin-Lim)."""

    def __init__(self, config: AudioFrontendConfig, device: Optional[torch.device] = None):
        self.config = config
        self.n_fft = config.win_length
        self.n_freqs = self.n_fft // 2 + 1
        self.fb = melscale_fbanks(self.n_freqs, float(config.fmin), float(config.fmax), config.num_mels, config.sample_rate)
        if device is not None:
            self.fb = self.fb.to(device)
        self._P: Dict[str, torch.Tensor] = {}  # inverse_basis() per device

    def stft_to_mels(self, D: torch.Tensor) -> torch.Tensor:  # MelScale: [..., n_freqs, T] -> [..., n_mels, T]
        return torch.matmul(D.transpose(-1, -2), self.fb.to(D.device)).transpose(-1, -2)

    def mels_to_stft(self, M: torch.Tensor) -> torch.Tensor:
        """InverseMelScale (torchaudio >= 2.1): least-squares solution of fb^T D = M, clamped at zero."""
        fbT = self.fb.to(M.device).transpose(-1, -2)  # [n_mels, n_freqs]
        lead = M.shape[:-2]
        m2 = M.reshape(-1, M.shape[-2], M.shape[-1])
        # driver "gels" is torchaudio's default and the only one the GPU backend offers; LAPACK's default
        # (gelsy) returns nothing useful here because the filterbank has all-zero rows above f_max
        sol = torch.linalg.lstsq(fbT.unsqueeze(0).expand(m2.shape[0], -1, -1).contiguous(), m2, driver="gels").solution
        return torch.relu(sol).reshape(lead + sol.shape[-2:])

    def inverse_basis(self, device=None) -> torch.Tensor:
        """P = fb (fb^T fb)^-1 [n_freqs, n_mels]: ``P @ M`` is the minimum-norm solution of fb^T D = M, which is what
        ``lstsq(driver="gels")`` returns in ``mels_to_stft`` (fb^T has full row rank).  Made once in fp64 on the host and
        rounded once to fp32."""
        key = str(torch.device(device) if device is not None else "cpu")
        if "cpu" not in self._P:
            fb = self.fb.detach().to("cpu", torch.float64)
            self._P["cpu"] = torch.linalg.solve(fb.T @ fb, fb.T).T.contiguous().to(torch.float32)
        if key not in self._P:
            self._P[key] = self._P["cpu"].to(device)
        return self._P[key]

    def mel_to_magnitude(self, y: torch.Tensor, lengths=None) -> torch.Tensor:
        """y [B, T, n_mels] (or [T, n_mels]), the model's normalised mel -> the magnitude [B, n_freqs, T] Griffin-Lim starts
        from: ``db_to_amplitude(mel_inv(m_rev(y)), 1, 1).sqrt()`` of every utterance in one kernel.  ``lengths`` ([B] mel
        frames, host or device): frames past them are zeros."""
        who = "AudioFrontend.mel_to_magnitude"
        _check_native(y, self.n_fft, self.config.hop_length, self.n_fft, who)
        y3 = y.unsqueeze(0) if y.dim() == 2 else y
        if y3.dim() != 3 or y3.shape[2] != self.config.num_mels:
            raise ValueError(f"{who}: y must be [B, T, n_mels = {self.config.num_mels}], got {tuple(y.shape)}")
        B, T, _ = y3.shape
        frames, on_device = _frames_arg(lengths, B, T, y.device, who)
        mag = _engine(y.device).mel_to_magnitude(y3.detach().contiguous(), self.inverse_basis(y.device), frames, self.n_fft, check=on_device)
        return mag[0] if y.dim() == 2 else mag

    def spectrogram(self, wave: torch.Tensor) -> torch.Tensor:
        """Spectrogram(power=2, normalized=True, center=True) (data/audio.py:50-52): [..., time] -> [..., n_freqs, 1 + time // hop],
        the "window" normalisation (by sqrt(sum w^2)) applied before the power."""
        window = torch.hann_window(self.n_fft, device=wave.device, dtype=wave.dtype)
        X = torch.stft(wave, n_fft=self.n_fft, hop_length=self.config.hop_length, win_length=self.n_fft, window=window, center=True,
                       pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        X = X / window.pow(2.0).sum().sqrt()
        return X.abs().pow(2.0)

    def encode(self, wave: torch.Tensor, sr: int):  # data/audio.py:55-67
        """wave [time] (or [..., time], normalised by the one peak of the whole tensor, as the reference has it) -> (D_db [T, n_freqs],
        M_db [T, n_mels]) in wave's dtype on its device, T = 1 + time // hop_length."""
        if sr != self.config.sample_rate:
            raise NotImplementedError(f"AudioFrontend.encode: resampling ({sr} -> {self.config.sample_rate} Hz) is not built: resample the "
                                      "waveform first")
        wave = wave / wave.abs().max()
        D = self.spectrogram(wave)
        M = torch.matmul(D.mT, self.fb.to(device=D.device, dtype=D.dtype)).mT  # stft_to_mels, in wave's dtype
        D_db = amplitude_to_db(D, 10, 1e-12, 0)
        M_db = amplitude_to_db(M, 10, 1e-12, 0)
        return D_db.mT, M_db.mT

    def encode_native(self, wave: torch.Tensor, lengths=None, *, spectrogram: bool = True, sr: Optional[int] = None):
        """``encode`` of every utterance of a padded batch in one call (ttsdec_mel_analysis, csrc/analysis.hip): wave [B, N] (or [N])
        fp32 on a ROCm device at the configured sample rate -> (D_db [B, T, n_freqs], M_db [B, T, n_mels], frames [B] int32),
        T = 1 + N // hop_length; for 1-D input the reference's 2-D shapes and a scalar count.  ``lengths`` ([B] samples, host or
        device): every utterance is normalised by its own peak and reflected at its own end, has 1 + length // hop_length frames and
        exact zeros past them.  ``spectrogram=False`` leaves D_db out (None): it is 87 % of the bytes the call writes.  ``sr``: the
        rate of ``wave`` and ``lengths``; one that differs from the configured rate sends the batch through ``resample_native`` first
        (the two calls chain on the device, the analysis reads the resampled lengths, and every peak is taken after resampling, as the
        reference has it); None or the configured rate is the call without it."""
        who = "AudioFrontend.encode_native"
        if sr is not None and sr != self.config.sample_rate:
            _check_native(wave, self.n_fft, self.config.hop_length, self.n_fft, who)
            wave, lengths = resample_native(wave, sr, self.config.sample_rate, lengths)
            if wave.dim() == 1:
                lengths = None  # (the row is the utterance)
        _check_native(wave, self.n_fft, self.config.hop_length, self.n_fft, who)
        w2 = wave.unsqueeze(0) if wave.dim() == 1 else wave
        if w2.dim() != 2:
            raise ValueError(f"{who}: wave must be [B, N] or [N], got {tuple(wave.shape)}")
        dev = wave.device
        B, N = w2.shape
        half = self.n_fft // 2
        if N <= half:
            raise ValueError(f"{who}: {N} samples: an utterance needs more than n_fft / 2 = {half} to be reflect-padded")
        if lengths is None:
            lens = None
        elif isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if tuple(lengths.shape) != (B,):
                raise ValueError(f"{who}: lengths must be [B] = [{B}], got {tuple(lengths.shape)}")
            lens = lengths.to(device=dev, dtype=torch.int32).contiguous()
        else:
            host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
            if len(host) != B or any(v <= half or v > N for v in host):
                raise ValueError(f"{who}: lengths must be [B] = [{B}] sample counts in [{half + 1}, {N}], got {host}")
            lens = torch.tensor(host, dtype=torch.int32).to(dev)
        key = (self.n_fft, str(dev))
        if key not in _windows:
            _windows[key] = torch.hann_window(self.n_fft).to(dtype=torch.float32, device=dev)
        fb = self.fb.detach().to(device=dev, dtype=torch.float32).contiguous()
        D_db, M_db, frames = _engine(dev).mel_analysis(w2.detach().contiguous(), lens, _windows[key], fb, self.config.hop_length, spectrogram)
        if wave.dim() == 1:
            return (D_db[0] if spectrogram else None), M_db[0], frames[0]
        return D_db, M_db, frames

    def mel_inv(self, M_db: torch.Tensor) -> torch.Tensor:  # data/audio.py:73-76
        M = db_to_amplitude(M_db.mT, 1, 1)
        D = self.mels_to_stft(M)
        return amplitude_to_db(D, 10, 1e-12, 0)

    def decode(self, D_db: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:  # data/audio.py:69-71
        D = db_to_amplitude(D_db, 1, 1)
        return griffinlim(D, self.n_fft, self.config.hop_length, self.n_fft, power=2.0, generator=generator)


def synth_audio(y: torch.Tensor, audio_frontend: AudioFrontend, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """inference.py:13-22: y [B, T, n_mels] (the model's normalised mel) -> waves [B, time], each peak-normalised."""
    wave = []
    for y_i in y:
        D_db = audio_frontend.mel_inv(m_rev(y_i))
        w = audio_frontend.decode(D_db, generator=generator)
        wave.append(w / w.abs().max())
    return torch.stack(wave)


# ---------------------------------------------------------------------------------------------------------------------------
# The same step through the HIP kernels (csrc/griffinlim.hip)
# ---------------------------------------------------------------------------------------------------------------------------
N_FFTS = (256, 512, 1024, 2048)  # what csrc/fft_lds.h has radix plans for
_ENGINES = None
_windows: Dict[tuple, torch.Tensor] = {}


def _engine(device: torch.device):
    """The weightless ttsdec handle of the stand-alone calls, one per device."""
    global _ENGINES
    from .engine import EngineCache, EngineDims

    if _ENGINES is None:
        _ENGINES = EngineCache()
    return _ENGINES.get(EngineDims(), device)


def wave_samples(frames: int, hop_length: int) -> int:
    """Samples of an utterance of ``frames`` mel frames: torch.istft(center=True) gives hop_length * (frames - 1)."""
    return hop_length * (frames - 1)


def _check_native(t: torch.Tensor, n_fft: int, hop_length: int, win_length: int, who: str) -> None:
    """The refusals of the native path, all before any device work."""
    if n_fft not in N_FFTS:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"n_fft = {n_fft}: built for {N_FFTS} (768, the dataclass default, needs a radix-3 pass)")
    if win_length != n_fft:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"win_length = {win_length}: built for win_length == n_fft = {n_fft}")
    if not 1 <= hop_length <= n_fft // 2:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"hop_length = {hop_length}: needs 1 <= hop_length <= n_fft / 2 = {n_fft // 2} (the overlap-added "
                                "squared window must have no zero)")
    if t.dtype != torch.float32:
        raise NotImplementedError(f"{who} is exact fp32: got {t.dtype}")
    if not t.is_cuda:
        raise NotImplementedError(f"{who} runs on a ROCm device only: there is no CPU fallback")


def _frames_arg(lengths, B: int, T: int, device: torch.device, who: str):
    """lengths (None, a sequence, a host or a device tensor of mel frames) -> ([B] int32 on the device or None, whether the host
    has not seen the values)."""
    if T < 2:
        raise ValueError(f"{who}: {T} frame(s): an utterance needs at least 2 frames to have samples")
    if lengths is None:
        return None, False
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"{who}: lengths must be [B] = [{B}], got {tuple(lengths.shape)}")
        return lengths.to(device=device, dtype=torch.int32).contiguous(), True
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(host) != B or any(v < 2 or v > T for v in host):
        raise ValueError(f"{who}: lengths must be [B] = [{B}] frame counts in [2, {T}], got {host}")
    return torch.tensor(host, dtype=torch.int32).to(device), False


def griffinlim_native(mag: torch.Tensor, n_fft: int, hop_length: int, win_length: int, n_iter: int = 32, momentum: float = 0.99,
                      rand_init: bool = True, generator: Optional[torch.Generator] = None, *, lengths=None, angles: Optional[torch.Tensor] = None,
                      tprev: Optional[torch.Tensor] = None, normalize: bool = False, return_state: bool = False):
    """``griffinlim`` through ttsdec_griffinlim, on the magnitude itself (no ``power``): mag [B, n_freqs, T] (or [n_freqs, T]) fp32
    on a ROCm device -> waveform [B, hop_length * (T - 1)].

    The start is ``angles`` ([B, n_freqs, T] complex) when given; else with ``rand_init`` it is drawn by the same two
    ``torch.rand`` calls as ``griffinlim`` makes for a tensor of mag's shape, so one seed gives both paths one start - complex(re, im)
    with re, im in [0, 1), not of unit modulus, as torchaudio has it; else all ones.  ``tprev`` (with ``angles``) continues a
    run from its state.  ``lengths`` ([B] mel frames, host or device): every utterance is inverted alone, reflected at its own end,
    and is zero past its hop_length * (frames - 1) samples.  ``normalize``: w / max |w| per utterance.  ``return_state``:
    (wave, rebuilt, angles) - the last rebuilt spectrum (the next ``tprev``) and the phase factors of the final inverse."""
    who = "griffinlim_native"
    _check_native(mag, n_fft, hop_length, win_length, who)
    if not 0 <= momentum < 1:
        raise ValueError(f"{who}: momentum must be in [0, 1), got {momentum}")
    if n_iter < 0:
        raise ValueError(f"{who}: n_iter must be >= 0, got {n_iter}")
    m3 = mag.unsqueeze(0) if mag.dim() == 2 else mag
    if m3.dim() != 3 or m3.shape[1] != n_fft // 2 + 1:
        raise ValueError(f"{who}: mag must be [B, n_fft / 2 + 1 = {n_fft // 2 + 1}, T], got {tuple(mag.shape)}")
    dev = mag.device
    B, bins, T = m3.shape
    frames, on_device = _frames_arg(lengths, B, T, dev, who)

    def state(t, name):
        t = t.unsqueeze(0) if t.dim() == 2 else t
        if tuple(t.shape) != (B, bins, T) or not t.is_complex():
            raise ValueError(f"{who}: {name} must be complex [B, n_freqs, T] = [{B}, {bins}, {T}], got {t.dtype} {tuple(t.shape)}")
        return t.to(device=dev, dtype=torch.complex64).contiguous()

    if tprev is not None and angles is None:
        raise ValueError(f"{who}: tprev continues a run and needs its angles")
    if angles is not None:
        angles = state(angles, "angles")
    elif rand_init:
        re = torch.rand(m3.shape, generator=generator, device=dev if generator is None or generator.device.type != "cpu" else "cpu")
        im = torch.rand(m3.shape, generator=generator, device=re.device)
        angles = torch.complex(re, im).to(dev)
    tprev = state(tprev, "tprev") if tprev is not None else None
    key = (n_fft, str(dev))
    if key not in _windows:
        _windows[key] = torch.hann_window(n_fft).to(dtype=torch.float32, device=dev)
    keep = return_state and n_iter > 0
    out = _engine(dev).griffinlim(m3.detach().contiguous(), frames, _windows[key], n_fft, hop_length,
                                  torch.view_as_real(angles) if angles is not None else None,
                                  torch.view_as_real(tprev) if tprev is not None else None, n_iter, float(momentum), normalize, keep, check=on_device)
    if not return_state:
        return out[0] if mag.dim() == 2 else out
    if keep:
        wave, rebuilt, ang = out
    else:  # no iteration: the state is the one that came in
        wave = out
        ang = angles if angles is not None else torch.ones(B, bins, T, dtype=torch.complex64, device=dev)
        rebuilt = tprev if tprev is not None else torch.zeros_like(ang)
    return (wave[0], rebuilt[0], ang[0]) if mag.dim() == 2 else (wave, rebuilt, ang)


def synth_audio_native(y: torch.Tensor, audio_frontend: AudioFrontend, lengths=None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``synth_audio`` for a padded batch on the device: y [B, T, n_mels] -> waves [B, hop_length * (T - 1)], each utterance
    peak-normalised over its own samples and zero past them; ``lengths`` [B] in mel frames, on the host or the device.  (The two
    ``torch.rand`` calls cover the whole batch, so for B > 1 the start differs from the one ``synth_audio`` draws utterance by
    utterance from the same generator.)"""
    fe = audio_frontend
    mag = fe.mel_to_magnitude(y, lengths)
    return griffinlim_native(mag, fe.n_fft, fe.config.hop_length, fe.n_fft, generator=generator, lengths=lengths, normalize=True)


def resample_native(wave: torch.Tensor, orig_freq: int, new_freq: int, lengths=None, *, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """``resample`` of every utterance of a padded batch in one call (ttsdec_resample, csrc/resample.hip): wave [B, N] (or [N]) fp32 on
    a ROCm device -> (out [B, n_out], lengths_out [B] int32), n_out = ceil(n * N / o); for 1-D input the 1-D wave and a scalar count.
    ``lengths`` ([B] samples, a sequence, a host or a device tensor): samples at or past them are never read, utterance b has
    ceil(n * lengths[b] / o) samples and exact zeros after them.  Equal rates return the input and its lengths."""
    who = "resample_native"
    o, n, _, _, taps = _resample_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, who)
    if o > 1024 or n > 1024 or taps > 16384:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"{orig_freq} -> {new_freq} Hz is {o} / {n} with {taps} taps: built for reduced rates <= 1024 "
                                "and <= 16384 taps (the table has n * taps words)")
    if wave.dtype != torch.float32:
        raise NotImplementedError(f"{who} is exact fp32: got {wave.dtype}")
    if not wave.is_cuda:
        raise NotImplementedError(f"{who} runs on a ROCm device only: there is no CPU fallback")
    w2 = wave.unsqueeze(0) if wave.dim() == 1 else wave
    if w2.dim() != 2 or w2.shape[1] < 1:
        raise ValueError(f"{who}: wave must be [B, N] or [N] with N >= 1, got {tuple(wave.shape)}")
    dev = wave.device
    B, N = w2.shape
    if N > 1 << 30 or -(-n * N // o) > 1 << 30 or B > 65535:
        raise _lib.DimsNotBuilt(_lib.ERR_DIMS, who, f"B = {B}, {N} samples: built for B <= 65535 and at most 2^30 samples in and out")
    on_device = False
    if lengths is None:
        lens = None
    elif isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if tuple(lengths.shape) != (B,):
            raise ValueError(f"{who}: lengths must be [B] = [{B}], got {tuple(lengths.shape)}")
        lens, on_device = lengths.to(device=dev, dtype=torch.int32).contiguous(), True
    else:
        host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(host) != B or any(v < 0 or v > N for v in host):
            raise ValueError(f"{who}: lengths must be [B] = [{B}] sample counts in [0, {N}], got {host}")
        lens = torch.tensor(host, dtype=torch.int32).to(dev)
    if o == n:
        counts = lens if lens is not None else torch.full((B,), N, dtype=torch.int32, device=dev)
        return (wave, counts[0]) if wave.dim() == 1 else (wave, counts)
    out, counts = _engine(dev).resample(w2.detach().contiguous(), lens, int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff),
                                        -(-n * N // o), check=on_device)
    return (out[0], counts[0]) if wave.dim() == 1 else (out, counts)


def xref_native(frontend: AudioFrontend, wave: torch.Tensor, lengths=None, sr: Optional[int] = None):
    """The reference-audio input of ``Tacotron.forward`` and the style encoders (inference.py ``--ref``): ``m_fwd`` of
    ``encode_native(wave, lengths, spectrogram=False, sr=sr)`` -> (xref [B, T, n_mels], frames [B] int32), exact zeros at the frames
    at or past each utterance's count (``m_fwd(0)`` is 1, so they are masked)."""
    _, M_db, frames = frontend.encode_native(wave, lengths, spectrogram=False, sr=sr)
    xref = m_fwd(M_db)
    if M_db.dim() == 3:
        live = torch.arange(M_db.shape[1], device=M_db.device)[None, :] < frames[:, None]
        xref = torch.where(live[:, :, None], xref, torch.zeros_like(xref))
    return xref, frames
