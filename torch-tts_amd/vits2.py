"""Drop-ins for the VITS2 second hot path of the reference:

* ``TextEncoder``                         - vits2/models.py:330-380 (same constructor, parameters, state-dict keys;
                                             ``forward(x, x_lengths, g=None) -> (x, m, logs, x_mask)``)
* ``ResidualCouplingTransformersBlock``   - vits2/models.py:681-810 with ``transformer_flow_type="pre_conv"``
                                             (``forward(x, x_mask, g=None, reverse=True)``)
* ``Generator`` (+ ``ResBlock1``)         - the HiFi-GAN generator, vits2/models.py:900-974 and modules.py:221-315
                                             (``forward(x, g=None) -> [B, 1, T * prod(upsample_rates)]``; ``ttsgen_*``)
* ``StochasticDurationPredictor``         - vits2/models.py:29-137: ``forward(x, x_mask, g=None, reverse=True, noise_scale=1.0)
                                             -> logw [B, 1, T]`` (``ttsdur_*``), and the other direction as ``nll(x, x_mask, w,
                                             g=None) -> [B]``, the likelihood of given durations (``ttsvits_durnll_*``)
* ``DurationPredictor``                   - vits2/models.py:140-180 (``forward(x, x_mask, g=None) -> logw [B, 1, T]``)
* ``infer(net_g, x, x_lengths, ...)``     - SynthesizerTrn.infer (models.py:1288-1323) over the four drop-ins, channel-last
                                             from the ids to the waveform
* ``PosteriorEncoder``                    - vits2/models.py:858-897 (``forward(x, x_lengths, g=None) -> (z, m, logs, x_mask)``;
                                             ``ttspost_*``)
* ``voice_conversion(net_g, y, ...)``     - SynthesizerTrn.voice_conversion (models.py:1328-1336) over enc_q, flow (both
                                             directions) and dec
* ``maximum_path(neg_cent, mask)``        - monotonic_align.maximum_path (monotonic_align/__init__.py:6-19) on the device
* ``align(z_p, m_p, logs_p, ...)``        - the no_grad block of SynthesizerTrn.forward (models.py:1224-1254): neg_cent and the search
* ``forced_alignment(net_g, x, ..., y, ...)`` - token durations of an utterance: enc_p, enc_q, flow forward, align
* ``spectrogram_torch`` / ``spec_to_mel_torch`` / ``mel_spectrogram_torch`` - mel_processing.py:58-187 (re-exported from
                                             ``mel_processing``), and ``voice_conversion_from_audio`` / ``forced_alignment_from_audio``
* ``DiscriminatorS`` / ``DiscriminatorP`` / ``MultiPeriodDiscriminator`` - the waveform discriminators, vits2/models.py:977-1110
                                             (``forward(x) -> (scores, fmap)``, ``forward(y, y_hat)`` -> the four lists;
                                             ``ttsvits_disc_*``), with ``feature_loss`` / ``discriminator_loss`` / ``generator_loss``
                                             (losses.py:7-34) as torch ops on the device
* ``DurationDiscriminatorV1`` / ``DurationDiscriminatorV2`` - the duration discriminators, vits2/models.py:183-329
                                             (``forward(x, x_mask, dur_r, dur_hat, g=None)`` -> ``[p_r, p_hat]`` / ``[[p_r], [p_hat]]``,
                                             ``forward_probability``; ``ttsvits_durdisc_*``), and
                                             ``duration_discriminator_scores(net_g, net_dur_disc, x, ..., y, ...)`` - what train.py:414
                                             feeds and gets from them
* ``duration_loss(net_g, x, ..., y, ...)`` - SynthesizerTrn.forward up to ``l_length`` (models.py:1214-1267), the VL/dur of the
                                             reference's validation, and ``duration_loss_from_audio``
* ``synthesizer_forward(net_g, x, ..., y, ...)`` - SynthesizerTrn.forward as a whole (models.py:1214-1286) in eval mode: its eight results
* ``validation_losses(net_g, net_d, ...)`` - the loss terms of train.py:341-425, forward only, and ``validation_losses_from_audio``;
                                             ``kl_loss`` (losses.py:37-46), ``slice_segments`` / ``rand_slice_segments`` (commons.py:50-66)
                                             (``ttsvits_kl_loss`` / ``ttsvits_slice_segments`` / ``ttsvits_sliced_l1``)

All hold the reference's parameters (so checkpoints load) and run inference through the HIP library
(``ttsvits_*`` / ``ttsgen_*`` / ``ttsdur_*`` / ``ttspost_*`` in include/ttsdec.h).  The library works on channel-last activations;
the [B, C, T] tensors of the reference API are transposed here.  Training (gradients) and time-varying speaker
conditioning are outside the path and raise."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from .engine import STREAM, WS, EngineCache, Handle, PackedWeightsMixin, _require_device


def speaker_rows(g: Optional[torch.Tensor], B: int, gin_channels: int, owner: str) -> Optional[torch.Tensor]:
    """g as the C ABI takes it: [B, gin] fp32 from the reference's [B, gin, 1] (models.py: g = emb_g(sid).unsqueeze(-1));
    owner names the module in the messages ("a generator")."""
    if g is None:
        return None
    if not gin_channels:
        raise ValueError(f"g was given to {owner} built with gin_channels = 0")
    _require_device(g, "g")
    if g.dim() == 3:
        if g.shape[2] != 1:
            raise NotImplementedError("a time-varying g [B, gin, T] is outside the HIP path (the reference's callers pass [B, gin, 1])")
        g = g[:, :, 0]
    if tuple(g.shape) != (B, gin_channels):
        raise ValueError(f"g must be [B, gin_channels(, 1)] = [{B}, {gin_channels}(, 1)], got {tuple(g.shape)}")
    return g.to(torch.float32).contiguous()


def inference_only(module: nn.Module, owner: str, x: Optional[torch.Tensor] = None, *, fp32: bool = False) -> None:
    """The guard in front of a module's HIP path: no autograd through the parameters (or x); with x given, x and the parameters
    on a ROCm device, and with fp32 also torch.float32.  owner names the module in the messages ("generator")."""
    # (parameters() is walked only where a check needs it: under no_grad the text encoder's and the flow's guard costs nothing)
    if x is not None and (not x.is_cuda or any(not p.is_cuda for p in module.parameters())):
        raise NotImplementedError(f"the HIP {owner} runs on a ROCm device only: move the module and its input there")
    if fp32 and (x.dtype != torch.float32 or any(p.dtype != torch.float32 for p in module.parameters())):
        raise NotImplementedError(f"the HIP {owner} is exact fp32: input and parameters must be torch.float32")
    if torch.is_grad_enabled() and ((x is not None and x.requires_grad) or any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError(f"the HIP {owner} is inference-only: call under torch.no_grad()")


class _LayerNorm(nn.Module):  # modules.LayerNorm: parameters gamma / beta
    def __init__(self, channels, eps=1e-5):
        super().__init__()
        self.channels, self.eps = channels, eps
        self.gamma = nn.Parameter(torch.ones(channels))
        self.beta = nn.Parameter(torch.zeros(channels))


class _MultiHeadAttention(nn.Module):  # attentions.MultiHeadAttention parameter holder (attentions.py:181-232)
    def __init__(self, channels, out_channels, n_heads, p_dropout=0.0, window_size=None):
        super().__init__()
        assert channels % n_heads == 0
        self.n_heads, self.window_size, self.k_channels = n_heads, window_size, channels // n_heads
        self.conv_q = nn.Conv1d(channels, channels, 1)
        self.conv_k = nn.Conv1d(channels, channels, 1)
        self.conv_v = nn.Conv1d(channels, channels, 1)
        self.conv_o = nn.Conv1d(channels, out_channels, 1)
        if window_size is not None:
            std = self.k_channels**-0.5
            self.emb_rel_k = nn.Parameter(torch.randn(1, window_size * 2 + 1, self.k_channels) * std)
            self.emb_rel_v = nn.Parameter(torch.randn(1, window_size * 2 + 1, self.k_channels) * std)
        nn.init.xavier_uniform_(self.conv_q.weight)
        nn.init.xavier_uniform_(self.conv_k.weight)
        nn.init.xavier_uniform_(self.conv_v.weight)


class _FFN(nn.Module):  # attentions.FFN parameter holder (attentions.py:385-410)
    def __init__(self, in_channels, out_channels, filter_channels, kernel_size):
        super().__init__()
        self.conv_1 = nn.Conv1d(in_channels, filter_channels, kernel_size)
        self.conv_2 = nn.Conv1d(filter_channels, out_channels, kernel_size)


class Encoder(nn.Module):
    """attentions.Encoder parameter layout (attentions.py:14-75)."""

    def __init__(self, hidden_channels, filter_channels, n_heads, n_layers, kernel_size=1, p_dropout=0.0, window_size=4, **kwargs):
        super().__init__()
        self.hidden_channels, self.filter_channels, self.n_heads = hidden_channels, filter_channels, n_heads
        self.n_layers, self.kernel_size, self.window_size = n_layers, kernel_size, window_size
        # attentions.py:41-52: a speaker-conditioned encoder adds spk_emb_linear(g) to the input of layer cond_layer_idx (2 unless given)
        self.gin_channels = int(kwargs.get("gin_channels", 0) or 0)
        self.cond_layer_idx = n_layers
        if self.gin_channels:
            self.spk_emb_linear = nn.Linear(self.gin_channels, hidden_channels)
            self.cond_layer_idx = kwargs.get("cond_layer_idx", 2)
            assert self.cond_layer_idx < n_layers, "cond_layer_idx should be less than n_layers"
        self.attn_layers = nn.ModuleList(_MultiHeadAttention(hidden_channels, hidden_channels, n_heads, window_size=window_size) for _ in range(n_layers))
        self.norm_layers_1 = nn.ModuleList(_LayerNorm(hidden_channels) for _ in range(n_layers))
        self.ffn_layers = nn.ModuleList(_FFN(hidden_channels, hidden_channels, filter_channels, kernel_size) for _ in range(n_layers))
        self.norm_layers_2 = nn.ModuleList(_LayerNorm(hidden_channels) for _ in range(n_layers))

    def weight_tensors(self) -> List[torch.Tensor]:
        out = []
        for i in range(self.n_layers):
            a, f = self.attn_layers[i], self.ffn_layers[i]
            out += [a.conv_q.weight, a.conv_q.bias, a.conv_k.weight, a.conv_k.bias, a.conv_v.weight, a.conv_v.bias, a.conv_o.weight, a.conv_o.bias]
            if self.window_size is not None:
                out += [a.emb_rel_k, a.emb_rel_v]
            out += [self.norm_layers_1[i].gamma, self.norm_layers_1[i].beta, f.conv_1.weight, f.conv_1.bias, f.conv_2.weight, f.conv_2.bias,
                    self.norm_layers_2[i].gamma, self.norm_layers_2[i].beta]
        return out


class VitsEngine(Handle):
    """One ttsvits handle on one device."""

    PREFIX = "ttsvits"

    def __init__(self, dims: Dict[str, int], device: torch.device):
        dims = dict(dict(gin_channels=0, cond_layer_idx=0), **dims)
        try:
            super().__init__(dims, _lib.VitsDims(*[int(dims[n]) for n, _ in _lib.VitsDims._fields_]), device)
        except _lib.DimsNotBuilt:
            # the one refusal of ttsvits_create that is not about a single field: a head wider than the attention kernels hold
            stacks = [("the text encoder", dims["hidden_channels"], dims["n_heads"])]
            if dims["n_flows"] > 0:
                stacks.append(("the flow's pre_transformer", dims["inter_channels"] // 2, dims["flow_tf_heads"]))
            for owner, ch, heads in stacks:
                if ch > 0 and heads > 0 and ch // heads > _lib.VITS_MAX_HEAD_WIDTH:
                    raise _lib.DimsNotBuilt(_lib.ERR_DIMS, "ttsvits_create", f"head width {ch // heads} ({ch} channels / {heads} heads) of {owner}: the "
                                            f"attention kernels are built for up to {_lib.VITS_MAX_HEAD_WIDTH}") from None
            raise
        self.status = torch.zeros(1, dtype=torch.int32, device=device)  # bit 0: an id outside the table (ttsvits_text_encoder)

    def text_encoder(self, ids: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor] = None):
        _require_device(ids, "ids")
        B, T = ids.shape
        g = speaker_rows(g, B, self.dims["gin_channels"], "a module")
        ids = ids.to(torch.int64).contiguous()
        self.status.zero_()
        lens = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        H, I = self.dims["hidden_channels"], self.dims["inter_channels"]
        x = torch.empty(B, T, H, device=self.device)
        m = torch.empty(B, T, I, device=self.device)
        logs = torch.empty(B, T, I, device=self.device)
        ws = self.sized_workspace("te", "ttsvits_text_encoder_workspace_bytes", B, T)
        self.call("ttsvits_text_encoder", ids, lens, g, B, T, x, m, logs, WS(ws), STREAM, self.status)
        # nn.Embedding raises IndexError on an id outside the table (models.py:370): the kernel clamps and reports through the status
        # word - one host sync here, behind the queued launches (no scan of the ids before them)
        if int(self.status) & 1:
            raise IndexError(f"token id out of range [0, {self.dims['n_vocab']}) in the text encoder's input")
        return x, m, logs

    def _flow(self, fn: str, z_cl: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor]) -> torch.Tensor:
        """One direction of the flow (the C function fn) on z_cl [B, T, inter] channel-last.  A contiguous fp32 z_cl is passed as it
        is, without a copy, whatever its alignment (a view into a larger buffer may be only 4-byte aligned: the library then takes
        its one-element kernels for the first coupling)."""
        _require_device(z_cl, "z")
        B, T, _ = z_cl.shape
        g = speaker_rows(g, B, self.dims["gin_channels"], "a module")
        z_cl = z_cl.to(torch.float32).contiguous()
        lens = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty_like(z_cl)
        ws = self.sized_workspace("flow", "ttsvits_flow_workspace_bytes", B, T)
        self.call(fn, z_cl, lens, g, B, T, out, WS(ws), STREAM)
        return out

    def flow_reverse(self, z_cl: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor] = None) -> torch.Tensor:
        """z_cl [B, T, inter] channel-last."""
        return self._flow("ttsvits_flow_reverse", z_cl, lengths, g)

    def flow_forward(self, z_cl: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The forward direction (ttsvits_flow_forward) on z_cl [B, T, inter] channel-last; same workspace as flow_reverse."""
        return self._flow("ttsvits_flow_forward", z_cl, lengths, g)

    # ---- monotonic alignment search (weightless: a handle of any dims serves, bound or not) ----
    _PATH_DTYPES = {torch.float32: _lib.PATH_F32, torch.float16: _lib.PATH_F16, torch.bfloat16: _lib.PATH_BF16}

    def neg_cent(self, z_p, m_p, logs_p, t_y: Optional[torch.Tensor], t_x: Optional[torch.Tensor]) -> torch.Tensor:
        """z_p [B, T_y, C], m_p / logs_p [B, T_x, C] contiguous fp32, t_y / t_x [B] int32 (device) or None -> neg_cent [B, T_y, T_x]
        (include/ttsdec.h ttsvits_neg_cent)."""
        B, T_y, Cc = z_p.shape
        T_x = m_p.shape[1]
        out = torch.empty(B, T_y, T_x, device=self.device)
        self.call("ttsvits_neg_cent", z_p, m_p, logs_p, t_y, t_x, B, T_y, T_x, Cc, out, STREAM)
        return out

    def maximum_path(self, neg_cent: torch.Tensor, t_y: torch.Tensor, t_x: torch.Tensor, dtype: Optional[torch.dtype] = torch.float32,
                     z_p=None, m_p=None, logs_p=None, also=None):
        """neg_cent [B, T_y, T_x] contiguous fp32, t_y / t_x [B] int32 (device) -> path [B, T_y, T_x] of ``dtype`` (None: not
        written), frame_token [B, T_y] int32, dur [B, T_x] int32 (include/ttsdec.h ttsvits_maximum_path).  With z_p, m_p, logs_p given,
        neg_cent is an output buffer and the call is ttsvits_align.  Reads the status word back: the call's one host sync.
        ``also``: (flag, message) - a device flag [1] int32 of the caller's, read in the same transfer; ValueError(message) when it
        is set and the search itself refused nothing."""
        B, T_y, T_x = neg_cent.shape
        if T_x > _lib.ALIGN_MAX_TX:
            raise _lib.DimsNotBuilt(_lib.ERR_DIMS, "ttsvits_maximum_path", f"T_x = {T_x} tokens: the search is built for up to {_lib.ALIGN_MAX_TX}")
        ws = self.sized_workspace("align", "ttsvits_align_workspace_bytes", B, T_y, T_x)
        # (a dtype the kernel does not store - fp64, integers - is written as fp32 and converted)
        kdt = dtype if dtype in self._PATH_DTYPES else torch.float32
        path = torch.empty(B, T_y, T_x, dtype=kdt, device=self.device) if dtype is not None else None
        ft = torch.empty(B, T_y, dtype=torch.int32, device=self.device)
        dur = torch.empty(B, T_x, dtype=torch.int32, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        if z_p is None:
            self.call("ttsvits_maximum_path", neg_cent, t_y, t_x, B, T_y, T_x, path, self._PATH_DTYPES[kdt], ft, dur, status, WS(ws), STREAM)
        else:
            self.call("ttsvits_align", z_p, m_p, logs_p, t_y, t_x, B, T_y, T_x, z_p.shape[2], neg_cent, path, self._PATH_DTYPES[kdt], ft, dur, status,
                      WS(ws), STREAM)
        if also is None:
            flags, more = int(status.item()), 0
        else:
            flags, more = torch.cat([status, also[0].to(torch.int32).reshape(1)]).tolist()
        if flags & 4:
            raise ValueError(f"an utterance's length from the mask exceeds the tensor [T_y, T_x] = [{T_y}, {T_x}]")
        if flags & 1:
            raise ValueError("an utterance has no frames or no tokens (t_y < 1 or t_x < 1): monotonic alignment search is undefined")
        if flags & 2:
            raise ValueError("an utterance has fewer frames than tokens (t_y < t_x): no monotonic path gives every token a frame")
        if more:
            raise ValueError(also[1])
        if path is not None and path.dtype != dtype:
            path = path.to(dtype)
        return path, ft, dur

    # ---- spectrogram front-end (weightless too; mel_processing.py holds the reference-named entry points) ----
    def _spec_workspace(self, n_fft: int, n_mels: int, name: str) -> torch.Tensor:
        return self.sized_workspace("spec", "ttsvits_spec_workspace_bytes", n_fft, n_mels, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, name, f"n_fft = {n_fft}, n_mels = {n_mels}: built for n_fft 256 / 512 / 1024 / 2048, n_mels <= 256"))

    def spectrogram(self, wav: torch.Tensor, lengths: Optional[torch.Tensor], window: torch.Tensor, n_fft: int, hop_size: int, T: int,
                    mel_basis: Optional[torch.Tensor] = None, *, check: bool = False) -> torch.Tensor:
        """wav [B, N] contiguous fp32, lengths [B] int32 (device) or None, window [win_size] -> spec [B, n_fft / 2 + 1, T], or with
        mel_basis [n_mels, bins] the log-mel [B, n_mels, T] (ttsvits_spectrogram / ttsvits_mel_spectrogram).  check: read the status
        word back (one host sync) and raise for an utterance the kernel refused - for lengths the host has not seen."""
        B, N = wav.shape
        n_mels = 0 if mel_basis is None else int(mel_basis.shape[0])
        name = "ttsvits_mel_spectrogram" if n_mels else "ttsvits_spectrogram"
        ws = self._spec_workspace(n_fft, n_mels, name)
        out = torch.empty(B, n_mels or n_fft // 2 + 1, T, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device) if check else None
        mel_args = (mel_basis, n_mels) if n_mels else ()
        self.call(name, wav, lengths, B, N, window, n_fft, hop_size, window.numel(), *mel_args, out, T, status, WS(ws), STREAM)
        if check:
            flags = int(status.item())
            if flags & 4:
                raise ValueError(f"an utterance's length exceeds the waveform tensor's {N} samples")
            if flags & 3:
                raise ValueError(f"an utterance is no longer than the reflect padding ({int((n_fft - hop_size) / 2)} samples) or too short for "
                                 f"one frame of n_fft = {n_fft}: its spectrogram is undefined")
        return out

    def spec_to_mel(self, spec: torch.Tensor, frames: Optional[torch.Tensor], n_fft: int, mel_basis: torch.Tensor) -> torch.Tensor:
        """spec [B, n_fft / 2 + 1, T] contiguous fp32, frames [B] int32 (device) or None -> log-mel [B, n_mels, T] (ttsvits_spec_to_mel)."""
        B, _, T = spec.shape
        n_mels = int(mel_basis.shape[0])
        ws = self._spec_workspace(n_fft, n_mels, "ttsvits_spec_to_mel")
        mel = torch.empty(B, n_mels, T, device=self.device)
        self.call("ttsvits_spec_to_mel", spec, frames, B, n_fft, T, mel_basis, n_mels, mel, WS(ws), STREAM)
        return mel

    # ---- the validation step's glue (weightless; csrc/evalstep.hip) ----
    def kl_loss(self, z_p, logs_q, m_p, logs_p, frame_token: Optional[torch.Tensor], t_y: torch.Tensor, expand: bool = False):
        """z_p, logs_q [B, T_y, C], m_p, logs_p [B, T_x, C] contiguous fp32 channel-last, frame_token [B, T_y] int32 or None (the
        prior is per frame), t_y [B] int32 (device) -> (kl [2]: the sum and the reference's kl_loss, kl_rows [B], m_p_exp,
        logs_p_exp [B, T_y, C] or None, None without ``expand``) (include/ttsdec.h ttsvits_kl_loss).  No host read."""
        B, T_y, Cc = z_p.shape
        T_x = m_p.shape[1]
        ws = self.sized_workspace("kl", "ttsvits_kl_loss_workspace_bytes", B, T_y, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsvits_kl_loss", f"B = {B}, T_y = {T_y}: more than 65535 utterances or 2^31 frames"))
        kl = torch.empty(2, device=self.device)
        rows = torch.empty(B, device=self.device)
        m_exp = torch.empty(B, T_y, Cc, device=self.device) if expand else None
        logs_exp = torch.empty(B, T_y, Cc, device=self.device) if expand else None
        self.call("ttsvits_kl_loss", z_p, logs_q, m_p, logs_p, frame_token, t_y, B, T_y, T_x, Cc, m_exp, logs_exp, rows, kl, WS(ws), STREAM)
        return kl, rows, m_exp, logs_exp

    def slice_segments(self, x: torch.Tensor, ids: torch.Tensor, outer: int, T: int, inner: int, seg: int, scale: int = 1):
        """x contiguous fp32 viewed as [B, outer, T, inner], ids [B] int64 / int32 (device) -> (out [B, outer, seg, inner] flat as
        [B, outer * seg * inner], status [1] int32 on the device: 1 = a start outside [0, T - seg], that slice zeros)
        (ttsvits_slice_segments).  No host read."""
        B = x.shape[0]
        out = torch.empty(B, outer * seg * inner, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.call("ttsvits_slice_segments", x, ids, int(ids.dtype == torch.int64), B, outer, T, inner, seg, scale, out, status, STREAM)
        return out, status

    def sliced_l1(self, a: torch.Tensor, y: torch.Tensor, ids: Optional[torch.Tensor]):
        """a [B, C, T_a], y [B, C, seg] contiguous fp32, ids [B] int64 / int32 (device) or None (seg == T_a) -> (l1 [2]: the sum
        of |a[b, c, ids[b] + t] - y[b, c, t]| and its mean, l1_rows [B], status [1]) (ttsvits_sliced_l1).  No host read."""
        B, Cc, T_a = a.shape
        l1 = torch.empty(2, device=self.device)
        rows = torch.empty(B, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.call("ttsvits_sliced_l1", a, y, ids, int(ids is not None and ids.dtype == torch.int64), B, Cc, T_a, y.shape[2], rows, l1, status, STREAM)
        return l1, rows, status


_DEFAULT_FLOW = dict(flow_hidden=4, flow_kernel=1, flow_wn_layers=1, n_flows=0, flow_tf_layers=0, flow_tf_heads=1, flow_tf_kernel=1)


class TextEncoder(PackedWeightsMixin, nn.Module):
    def __init__(self, n_vocab, out_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        self.n_vocab, self.out_channels, self.hidden_channels, self.filter_channels = n_vocab, out_channels, hidden_channels, filter_channels
        self.n_heads, self.n_layers, self.kernel_size, self.p_dropout, self.gin_channels = n_heads, n_layers, kernel_size, p_dropout, gin_channels
        self.emb = nn.Embedding(n_vocab, hidden_channels)
        nn.init.normal_(self.emb.weight, 0.0, hidden_channels**-0.5)
        self.encoder = Encoder(hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout, gin_channels=gin_channels)  # models.py:358-366
        self.proj = nn.Conv1d(hidden_channels, out_channels * 2, 1)
        self.precision = "f32"  # arithmetic of the GEMMs: "f32" (the reference's own: exact fp32, default) or "split_f16" (two fp16 planes, opt-in: ~1.8x faster)
        self._engines = EngineCache(VitsEngine)

    def _dims(self):
        d = dict(n_vocab=self.n_vocab, inter_channels=self.out_channels, hidden_channels=self.hidden_channels, filter_channels=self.filter_channels,
                 n_heads=self.n_heads, n_layers=self.n_layers, kernel_size=self.kernel_size, window_size=self.encoder.window_size,
                 gin_channels=self.gin_channels, cond_layer_idx=self.encoder.cond_layer_idx if self.gin_channels else 0)
        d.update(_DEFAULT_FLOW)
        return d

    def forward(self, x, x_lengths, g=None):
        xo, m, logs = self.forward_cl(x, x_lengths, g)
        T = x.shape[1]
        x_mask = (torch.arange(T, device=x.device)[None, :] < x_lengths.to(x.device)[:, None]).unsqueeze(1).to(xo.dtype)
        return xo.transpose(1, 2), m.transpose(1, 2), logs.transpose(1, 2), x_mask

    def forward_cl(self, x, x_lengths, g=None):
        """forward's x, m, logs channel-last [B, T, C] (the library's own layout; ``infer`` chains it)."""
        inference_only(self, "text encoder")
        eng = self._engines.get(self._dims(), x.device)
        eng.set_precision(self.precision)
        eng.ensure_packed(self.weight_tensors())
        return eng.text_encoder(x, x_lengths, g)

    def weight_tensors(self) -> List[torch.Tensor]:
        """ttsvits_pack_weights' order (include/ttsdec.h) up to the text encoder's last tensor; a handle without flows takes no more."""
        spk = [self.encoder.spk_emb_linear.weight, self.encoder.spk_emb_linear.bias] if self.gin_channels else []
        return [self.emb.weight] + spk + self.encoder.weight_tensors() + [self.proj.weight, self.proj.bias]


class _WN(nn.Module):
    """modules.WN parameter layout (modules.py:133-183): weight-normalised convs (weight_g / weight_v)."""

    def __init__(self, hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=0, p_dropout=0):
        super().__init__()
        if dilation_rate != 1:
            raise NotImplementedError("WN with dilation_rate != 1 is outside the HIP path")
        self.hidden_channels, self.n_layers, self.kernel, self.gin_channels = hidden_channels, n_layers, kernel_size, gin_channels
        self.in_layers, self.res_skip_layers = nn.ModuleList(), nn.ModuleList()
        if gin_channels != 0:  # modules.py:149-153
            self.cond_layer = nn.utils.weight_norm(nn.Conv1d(gin_channels, 2 * hidden_channels * n_layers, 1), name="weight")
        for i in range(n_layers):
            self.in_layers.append(nn.utils.weight_norm(nn.Conv1d(hidden_channels, 2 * hidden_channels, kernel_size, padding=(kernel_size - 1) // 2), name="weight"))
            rs = 2 * hidden_channels if i < n_layers - 1 else hidden_channels
            self.res_skip_layers.append(nn.utils.weight_norm(nn.Conv1d(hidden_channels, rs, 1), name="weight"))

    def weight_tensors(self):
        out = []
        if self.gin_channels != 0:
            out += [torch._weight_norm(self.cond_layer.weight_v, self.cond_layer.weight_g, 0), self.cond_layer.bias]
        for i in range(self.n_layers):
            for l in (self.in_layers[i], self.res_skip_layers[i]):
                w = torch._weight_norm(l.weight_v, l.weight_g, 0)  # effective weight g * v / ||v||
                out += [w, l.bias]
        return out


class ResidualCouplingTransformersLayer(nn.Module):
    """Parameter layout of models.py:436-505 (mean_only)."""

    def __init__(self, channels, hidden_channels, kernel_size, dilation_rate, n_layers, p_dropout=0, gin_channels=0, mean_only=False):
        super().__init__()
        if not mean_only:
            raise NotImplementedError("only mean_only=True (what ResidualCouplingTransformersBlock builds) is on the HIP path")
        self.channels, self.hidden_channels, self.half_channels = channels, hidden_channels, channels // 2
        self.pre_transformer = Encoder(self.half_channels, self.half_channels, n_heads=2, n_layers=2, kernel_size=3, p_dropout=0.1, window_size=None)
        self.pre = nn.Conv1d(self.half_channels, hidden_channels, 1)
        self.enc = _WN(hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=gin_channels, p_dropout=p_dropout)
        # (present in the reference's state dict, unused by its forward: models.py:513-515)
        self.post_transformer = Encoder(hidden_channels, hidden_channels, n_heads=2, n_layers=2, kernel_size=3, p_dropout=0.1, window_size=None)
        self.post = nn.Conv1d(hidden_channels, self.half_channels, 1)
        self.post.weight.data.zero_()
        self.post.bias.data.zero_()

    def weight_tensors(self):
        return self.pre_transformer.weight_tensors() + [self.pre.weight, self.pre.bias] + self.enc.weight_tensors() + [self.post.weight, self.post.bias]


class _Flip(nn.Module):
    pass


class ResidualCouplingTransformersBlock(PackedWeightsMixin, nn.Module):
    def __init__(self, channels, hidden_channels, kernel_size, dilation_rate, n_layers, n_flows=4, gin_channels=0,
                 use_transformer_flows=False, transformer_flow_type="pre_conv"):
        super().__init__()
        self._watch_state_dict_loads()
        if not use_transformer_flows or transformer_flow_type != "pre_conv":
            raise NotImplementedError("only use_transformer_flows=True with transformer_flow_type='pre_conv' (the ModelConfig default) is built")
        self.channels, self.hidden_channels, self.kernel_size, self.n_layers, self.n_flows = channels, hidden_channels, kernel_size, n_layers, n_flows
        self.gin_channels = gin_channels
        self.flows = nn.ModuleList()
        for _ in range(n_flows):
            self.flows.append(ResidualCouplingTransformersLayer(channels, hidden_channels, kernel_size, dilation_rate, n_layers,
                                                                gin_channels=gin_channels, mean_only=True))
            self.flows.append(_Flip())
        self.precision = "f32"  # arithmetic of the GEMMs: "f32" (the reference's own: exact fp32, default) or "split_f16" (two fp16 planes, opt-in: ~1.8x faster)
        self._engines = EngineCache(VitsEngine)

    def _dims(self):
        return dict(n_vocab=1, inter_channels=self.channels, hidden_channels=4, filter_channels=4, n_heads=1, n_layers=0, kernel_size=1, window_size=0,
                    flow_hidden=self.hidden_channels, flow_kernel=self.kernel_size, flow_wn_layers=self.n_layers, n_flows=self.n_flows,
                    flow_tf_layers=2, flow_tf_heads=2, flow_tf_kernel=3, gin_channels=self.gin_channels, cond_layer_idx=0)

    def forward(self, x, x_mask, g=None, reverse=False):
        if not reverse:
            # (the reference's forward direction also returns the training logdet; its inference use - the flow step of
            # voice_conversion - is forward_cl)
            raise NotImplementedError("forward(reverse=False) is the training direction and is not on the HIP path: call forward_cl(x_cl, "
                                      "lengths, g) for the forward pass without logdet, or vits2.voice_conversion")
        lengths = x_mask[:, 0, :].sum(dim=1).round().to(torch.int32)  # sequence_mask is a prefix mask
        out = self.reverse_cl(x.transpose(1, 2), lengths, g)
        return out.transpose(1, 2)

    def reverse_cl(self, z_cl, lengths, g=None):
        """The reverse pass on channel-last z [B, T, channels] with lengths [B] (``infer`` chains it)."""
        return self._engine(z_cl).flow_reverse(z_cl, lengths, g)

    def forward_cl(self, x_cl, lengths, g=None):
        """The forward direction (models.py:803-806: layer_0, Flip, ..., layer_{n-1}, Flip) on channel-last x [B, T, channels] with
        lengths [B] -> [B, T, channels]; the logdet is not computed (``voice_conversion`` chains it)."""
        return self._engine(x_cl).flow_forward(x_cl, lengths, g)

    def _engine(self, z_cl) -> VitsEngine:
        inference_only(self, "flow")
        eng = self._engines.get(self._dims(), z_cl.device)
        eng.set_precision(self.precision)
        eng.ensure_packed(self.weight_tensors, key_tensors=list(self.parameters()))
        return eng

    def weight_tensors(self) -> List[Optional[torch.Tensor]]:
        """ttsvits_pack_weights' order (include/ttsdec.h): None for the tensors of the (absent) text encoder."""
        # emb, (spk_emb_linear.{weight,bias},) proj.weight, proj.bias
        ts: List[Optional[torch.Tensor]] = [None] * (5 if self.gin_channels else 3)
        for i in range(self.n_flows):
            ts += self.flows[2 * i].weight_tensors()  # (materialises the weight-normed conv weights)
        return ts


# ---------------------------------------------------------------------------------------------------------------------------
# HiFi-GAN generator (models.py:900-974): z -> waveform through ttsgen_* (include/ttsdec.h)
# ---------------------------------------------------------------------------------------------------------------------------
LRELU_SLOPE = 0.1  # modules.LRELU_SLOPE


def _get_padding(kernel_size, dilation=1):  # commons.py:14-15
    return int((kernel_size * dilation - dilation) / 2)


def _effective_weight(conv: nn.Module) -> torch.Tensor:
    """The weight a conv applies: g * v / ||v|| while torch.nn.utils.weight_norm is on (dim 0 - for a ConvTranspose1d weight
    [in, out, k] that is per INPUT channel, as the reference's ups.i.weight_g [in, 1, 1] says), else the plain weight."""
    if hasattr(conv, "weight_g"):
        return torch._weight_norm(conv.weight_v, conv.weight_g, 0)
    return conv.weight


class ResBlock1(nn.Module):
    """modules.ResBlock1 parameter layout (modules.py:221-294): convs1 (dilated) and convs2, weight-normalised.  Runs only as a
    part of ``Generator`` (the library fuses its layers into the generator's GEMM epilogues)."""

    def __init__(self, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        wn = nn.utils.weight_norm
        self.channels, self.kernel_size, self.dilation = channels, kernel_size, tuple(dilation)
        self.convs1 = nn.ModuleList(wn(nn.Conv1d(channels, channels, kernel_size, 1, dilation=d, padding=_get_padding(kernel_size, d)))
                                    for d in dilation)
        self.convs2 = nn.ModuleList(wn(nn.Conv1d(channels, channels, kernel_size, 1, dilation=1, padding=_get_padding(kernel_size, 1)))
                                    for _ in dilation)
        for c in list(self.convs1) + list(self.convs2):  # commons.init_weights
            c.weight_v.data.normal_(0.0, 0.01)

    def remove_weight_norm(self):
        for c in list(self.convs1) + list(self.convs2):
            nn.utils.remove_weight_norm(c)

    def weight_tensors(self) -> List[torch.Tensor]:
        out = []
        for c in list(self.convs1) + list(self.convs2):
            out += [_effective_weight(c), c.bias]
        return out


def _precision_code(mode: str) -> int:
    """"f32" / "split_f16" -> TTSDEC_PREC_*; anything else is a ValueError."""
    try:
        return {"f32": _lib.PREC_F32, "split_f16": _lib.PREC_SPLIT_F16}[mode]
    except (KeyError, TypeError):
        raise ValueError(f'precision must be "f32" or "split_f16", got {mode!r}') from None


class GenEngine(Handle):
    """One ttsgen handle on one device."""

    PREFIX = "ttsgen"

    def __init__(self, dims: Dict, device: torch.device):
        d = _lib.GenDims()
        d.initial_channel, d.upsample_initial_channel = dims["initial_channel"], dims["upsample_initial_channel"]
        d.n_up, d.n_res = len(dims["upsample_rates"]), len(dims["resblock_kernel_sizes"])
        if d.n_up > _lib.GEN_MAX_UP or d.n_res > _lib.GEN_MAX_RES:
            raise NotImplementedError("more upsampling stages / resblocks than the library's ttsgen_dims holds")
        for i, (u, k) in enumerate(zip(dims["upsample_rates"], dims["upsample_kernel_sizes"])):
            d.up_rates[i], d.up_kernels[i] = u, k
        n_dil = {len(ds) for ds in dims["resblock_dilation_sizes"]}
        d.n_dil = n_dil.pop() if len(n_dil) == 1 else -1
        for j, (k, ds) in enumerate(zip(dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"])):
            d.res_kernels[j] = k
            for l, dl in enumerate(list(ds)[:3]):
                d.res_dilations[j][l] = dl
        d.resblock = 1 if str(dims["resblock"]) == "1" else 2
        d.gin_channels = dims["gin_channels"]
        super().__init__(dims, d, device)
        self.up_total = math.prod(dims["upsample_rates"])
        self._planes: Optional[torch.Tensor] = None  # the split-fp16 weight planes (ttsvits_generator_pack_planes) ...
        self._planes_of = None                       # ... and the fp32 blob they were split from

    def planes(self) -> torch.Tensor:
        """The fp16 planes of the bound fp32 blob: built on the first split-fp16 call, rebuilt after every repack (a repack makes
        a new blob tensor)."""
        nbytes = int(self._lib.ttsvits_generator_planes_bytes(self._h))
        if self._planes is None or self._planes_of is not self.blob:
            planes = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.call("ttsvits_generator_pack_planes", planes, STREAM)
            self._planes, self._planes_of = planes, self.blob
        return self._planes

    def forward(self, z_cl: torch.Tensor, g: Optional[torch.Tensor], n_stages: Optional[int] = None, precision: str = "f32") -> torch.Tensor:
        """z_cl [B, T, C] channel-last fp32 -> [B, T * prod(u)]; n_stages (test aid): the activated output of that many stages,
        [B * T_s, C_s], read from the workspace; precision "f32" or "split_f16" (ttsvits_generator_forward)."""
        B, T, _ = z_cl.shape
        prec = _precision_code(precision)
        planes = self.planes() if prec == _lib.PREC_SPLIT_F16 else None
        ws = self.sized_workspace("forward", "ttsvits_generator_workspace_bytes", prec, B, T,
                                  refusal=NotImplementedError(f"one utterance of {T} frames exceeds the generator's 2-GiB group bound"))
        n_up = len(self.dims["upsample_rates"])
        out = torch.empty(B, T * self.up_total, device=self.device) if n_stages is None else None
        self.call("ttsvits_generator_forward", prec, planes, z_cl, g, B, T, n_up if n_stages is None else n_stages, out, WS(ws), STREAM)
        if n_stages is None:
            return out
        rates = self.dims["upsample_rates"][:n_stages]
        Ts = T * math.prod(rates)
        Cs = self.dims["upsample_initial_channel"] >> n_stages
        return ws[: B * Ts * Cs * 4].view(torch.float32).view(B, Ts, Cs).clone()


class Generator(PackedWeightsMixin, nn.Module):
    """models.Generator (models.py:900-974): same constructor, parameters and state-dict keys (weight-normalised ``ups`` and
    ``resblocks``; ``remove_weight_norm()`` turns them into plain ``weight``s, and both forms load and run).  ``forward(x
    [B, C, T], g=None) -> [B, 1, T * prod(upsample_rates)]`` runs in the HIP library, in exact fp32 unless ``precision`` is set to
    "split_f16"; inference only."""

    def __init__(self, initial_channel, resblock, resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates, upsample_initial_channel,
                 upsample_kernel_sizes, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        if str(resblock) != "1":
            raise NotImplementedError("only ResBlock1 (resblock='1', the ModelConfig default) is built in the HIP library")
        self.num_kernels = len(resblock_kernel_sizes)
        self.num_upsamples = len(upsample_rates)
        self._cfg = dict(initial_channel=initial_channel, resblock=str(resblock), resblock_kernel_sizes=list(resblock_kernel_sizes),
                         resblock_dilation_sizes=[list(d) for d in resblock_dilation_sizes], upsample_rates=list(upsample_rates),
                         upsample_initial_channel=upsample_initial_channel, upsample_kernel_sizes=list(upsample_kernel_sizes),
                         gin_channels=gin_channels)
        self.conv_pre = nn.Conv1d(initial_channel, upsample_initial_channel, 7, 1, padding=3)
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            self.ups.append(nn.utils.weight_norm(nn.ConvTranspose1d(upsample_initial_channel // (2**i), upsample_initial_channel // (2 ** (i + 1)),
                                                                    k, u, padding=(k - u) // 2)))
        self.resblocks = nn.ModuleList()
        ch = upsample_initial_channel
        for i in range(len(self.ups)):
            ch = upsample_initial_channel // (2 ** (i + 1))
            for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(ResBlock1(ch, k, d))
        self.conv_post = nn.Conv1d(ch, 1, 7, 1, padding=3, bias=False)
        for u in self.ups:  # commons.init_weights
            u.weight_v.data.normal_(0.0, 0.01)
        self.gin_channels = gin_channels
        if gin_channels != 0:
            self.cond = nn.Conv1d(gin_channels, upsample_initial_channel, 1)
        self._engines = EngineCache(GenEngine)
        self.precision = "f32"  # arithmetic of the GEMMs: "f32" (the reference's own: exact fp32, default) or "split_f16" (two fp16 planes, opt-in)

    def remove_weight_norm(self):
        for l in self.ups:
            nn.utils.remove_weight_norm(l)
        for l in self.resblocks:
            l.remove_weight_norm()
        self.invalidate()

    def weight_tensors(self) -> List[torch.Tensor]:
        """The effective fp32 weights in ttsgen_pack_weights' order (include/ttsdec.h)."""
        out = [self.conv_pre.weight, self.conv_pre.bias]
        for u in self.ups:
            out += [_effective_weight(u), u.bias]
        for rb in self.resblocks:
            out += rb.weight_tensors()
        out.append(self.conv_post.weight)
        if self.gin_channels:
            out += [self.cond.weight, self.cond.bias]
        return out

    def _engine(self, x: torch.Tensor) -> GenEngine:
        _precision_code(self.precision)
        inference_only(self, "generator", x, fp32=True)
        eng = self._engines.get(self._cfg, x.device)
        eng.ensure_packed(self.weight_tensors, key_tensors=list(self.parameters()))
        return eng

    def _speaker(self, g: Optional[torch.Tensor], B: int) -> Optional[torch.Tensor]:
        return speaker_rows(g, B, self.gin_channels, "a generator")

    def forward(self, x, g=None):
        eng = self._engine(x)
        B = x.shape[0]
        out = eng.forward(x.transpose(1, 2).contiguous(), self._speaker(g, B), precision=self.precision)  # (a copy also makes infer's sliced z contiguous)
        return out.unsqueeze(1)

    def forward_cl(self, z_cl, g=None):
        """forward on channel-last z [B, T, C] -> [B, T * prod(upsample_rates)] (``infer`` chains it)."""
        eng = self._engine(z_cl)
        return eng.forward(z_cl.contiguous(), self._speaker(g, z_cl.shape[0]), precision=self.precision)

    def stage_outputs(self, x, g=None, n_stages=0) -> torch.Tensor:
        """Test aid: the activated output of the first ``n_stages`` upsampling stages (0: conv_pre's), channel-last
        [B, T_s, C_s] - leaky_relu(x, 0.1), or 0.01 after the last stage."""
        eng = self._engine(x)
        return eng.forward(x.transpose(1, 2).contiguous(), self._speaker(g, x.shape[0]), n_stages=n_stages, precision=self.precision)


# ---------------------------------------------------------------------------------------------------------------------------
# Waveform discriminators (models.py:977-1110) through ttsvits_disc_* (include/ttsdec.h), and the three GAN terms of losses.py:7-34
# ---------------------------------------------------------------------------------------------------------------------------
class DiscEngine(Handle):
    """One ttsvits_disc handle on one device: DiscriminatorP(period) or, with period 0, DiscriminatorS."""

    PREFIX = "ttsvits_disc"

    def __init__(self, dims: Dict, device: Optional[torch.device]):
        super().__init__(dims, _lib.DiscDims(dims["period"], dims["kernel_size"], dims["stride"]), device)
        self.p = dims["period"] or 1
        if dims["period"]:  # (Co, kernel, stride) of every conv and of conv_post
            k, s = dims["kernel_size"], dims["stride"]
            self.layers = [(32, k, s), (128, k, s), (512, k, s), (1024, k, s), (1024, k, 1), (1, 3, 1)]
        else:
            self.layers = [(16, 15, 1), (64, 41, 4), (256, 41, 4), (1024, 41, 4), (1024, 41, 4), (1024, 5, 1), (1, 3, 1)]

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self._fn("workspace_bytes")(self._h, B, T))

    def heights(self, T: int) -> List[int]:
        """Rows per column after every conv and after conv_post (H = ceil(T / p) before them)."""
        H, out = -(-T // self.p), []
        for _, k, s in self.layers:
            H = (H + 2 * ((k - 1) // 2) - k) // s + 1
            out.append(H)
        return out

    def forward(self, y: torch.Tensor, with_fmaps: bool = True):
        """y [B, T] contiguous fp32 -> (scores [B, H_last * p], the convs' activated outputs [B, p, H_i, C_i] channels-last, or None:
        a scores-only call keeps them in the workspace)."""
        B, T = y.shape
        p = self.p
        if T % p and p - T % p >= T:
            raise ValueError(f"{T} samples cannot be reflect-padded to a multiple of the period {p}: the pad ({p - T % p}) must be smaller than T")
        nbytes = self.workspace_bytes(B, T)
        if nbytes == 0:
            raise _lib.DimsNotBuilt(_lib.ERR_DIMS, "ttsvits_disc_forward", f"B = {B}, T = {T}: an activation's indices leave 32 bits; split the batch")
        Hs = self.heights(T)
        scores = torch.empty(B, Hs[-1] * p, device=self.device)
        fm, arr, ws = None, None, None
        if with_fmaps:
            fm = [torch.empty(B, p, H, C, device=self.device) for H, (C, _, _) in zip(Hs[:-1], self.layers[:-1])]
            arr = (ctypes.c_void_p * len(fm))(*[t.data_ptr() for t in fm])
        else:
            ws = self.workspace("forward", nbytes)
        self.call("ttsvits_disc_forward", y, B, T, scores, arr, WS(ws), STREAM)
        return scores, fm


class _DiscriminatorBase(PackedWeightsMixin, nn.Module):
    """What DiscriminatorP and DiscriminatorS share: ``convs`` and ``conv_post`` (weight-normalised, the reference's state-dict
    keys), packed from their effective weights, and the call.  Inference only, exact fp32, eval mode."""

    def _setup(self, dims: Dict, use_spectral_norm: bool) -> None:
        if use_spectral_norm:
            raise NotImplementedError("use_spectral_norm=True is not built in the HIP library (weight norm only)")
        self.use_spectral_norm = False
        self._watch_state_dict_loads()
        self._cfg = dims
        self._engines = EngineCache(DiscEngine)

    def weight_tensors(self) -> List[torch.Tensor]:
        """The effective fp32 weights in ttsvits_disc_pack_weights' order (include/ttsdec.h)."""
        out = []
        for c in list(self.convs) + [self.conv_post]:
            out += [_effective_weight(c), c.bias]
        return out

    def _run(self, x: torch.Tensor, with_fmaps: bool):
        if x.dim() != 3 or x.shape[1] != 1 or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"x must be [B, 1, T], got {tuple(x.shape)}")
        p = self._cfg["period"] or 1
        T = x.shape[2]
        if T % p and p - T % p >= T:  # (before any launch, the weight packing included)
            raise ValueError(f"{T} samples cannot be reflect-padded to a multiple of the period {p}: the pad ({p - T % p}) must be smaller than T")
        inference_only(self, "discriminator", x, fp32=True)
        eng = self._engines.get(self._cfg, x.device)
        eng.ensure_packed(self.weight_tensors, key_tensors=list(self.parameters()))
        return eng.forward(x[:, 0].contiguous(), with_fmaps)

    def forward(self, x):
        """x [B, 1, T] -> (scores [B, L], fmap): the reference's shapes.  Every fmap but the last is a PERMUTED VIEW of the
        library's channels-last buffer (same shape and values as the reference's, other strides; ``.contiguous()`` copies);
        the last one is a view of the scores."""
        scores, fm = self._run(x, True)
        return scores, self._as_reference(scores, fm)

    def scores(self, x) -> torch.Tensor:
        """forward's scores alone: the feature maps stay in a workspace and are not returned."""
        return self._run(x, False)[0]


class DiscriminatorP(_DiscriminatorBase):
    """models.DiscriminatorP (models.py:977-1053): same constructor, parameters and state-dict keys."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        self._setup(dict(period=int(period), kernel_size=int(kernel_size), stride=int(stride)), use_spectral_norm)
        self.period = period
        wn, pad = nn.utils.weight_norm, (_get_padding(kernel_size, 1), 0)
        ch = [1, 32, 128, 512, 1024, 1024]
        self.convs = nn.ModuleList(wn(nn.Conv2d(ch[i], ch[i + 1], (kernel_size, 1), (stride if i < 4 else 1, 1), padding=pad)) for i in range(5))
        self.conv_post = wn(nn.Conv2d(1024, 1, (3, 1), 1, padding=(1, 0)))

    def _as_reference(self, scores, fm):
        B = scores.shape[0]
        return [t.permute(0, 3, 2, 1) for t in fm] + [scores.view(B, 1, -1, self.period)]  # [B, p, H, C] -> [B, C, H, p]


class DiscriminatorS(_DiscriminatorBase):
    """models.DiscriminatorS (models.py:1056-1083): same constructor, parameters and state-dict keys."""

    def __init__(self, use_spectral_norm=False):
        super().__init__()
        self._setup(dict(period=0, kernel_size=0, stride=0), use_spectral_norm)
        wn = nn.utils.weight_norm
        self.convs = nn.ModuleList([
            wn(nn.Conv1d(1, 16, 15, 1, padding=7)),
            wn(nn.Conv1d(16, 64, 41, 4, groups=4, padding=20)),
            wn(nn.Conv1d(64, 256, 41, 4, groups=16, padding=20)),
            wn(nn.Conv1d(256, 1024, 41, 4, groups=64, padding=20)),
            wn(nn.Conv1d(1024, 1024, 41, 4, groups=256, padding=20)),
            wn(nn.Conv1d(1024, 1024, 5, 1, padding=2)),
        ])
        self.conv_post = wn(nn.Conv1d(1024, 1, 3, 1, padding=1))

    def _as_reference(self, scores, fm):
        return [t[:, 0].permute(0, 2, 1) for t in fm] + [scores.unsqueeze(1)]  # [B, 1, L, C] -> [B, C, L]


class MultiPeriodDiscriminator(nn.Module):
    """models.MultiPeriodDiscriminator (models.py:1086-1110): DiscriminatorS and DiscriminatorP(2, 3, 5, 7, 11) under
    ``discriminators``; ``forward(y, y_hat)`` returns the reference's four lists.  Each member runs ONCE on the 2B rows of y and
    y_hat together - no kernel's arithmetic depends on the batch, so that is bit-identical to two calls - and the results are
    split by rows (views)."""

    def __init__(self, use_spectral_norm=False):
        super().__init__()
        discs = [DiscriminatorS(use_spectral_norm=use_spectral_norm)]
        discs += [DiscriminatorP(i, use_spectral_norm=use_spectral_norm) for i in [2, 3, 5, 7, 11]]
        self.discriminators = nn.ModuleList(discs)

    def forward(self, y, y_hat):
        if y.shape != y_hat.shape:
            raise ValueError(f"y and y_hat must have one shape, got {tuple(y.shape)} and {tuple(y_hat.shape)}")
        B = y.shape[0]
        both = torch.cat([y, y_hat], 0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d in self.discriminators:
            s, fmap = d(both)
            y_d_rs.append(s[:B])
            y_d_gs.append(s[B:])
            fmap_rs.append([f[:B] for f in fmap])
            fmap_gs.append([f[B:] for f in fmap])
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def feature_loss(fmap_r, fmap_g):
    """losses.py:7-13: twice the summed mean absolute distance of the feature maps (torch ops on the device)."""
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(rl.detach() - gl))
    return loss * 2


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """losses.py:16-25: the least-squares terms per discriminator, (real [n], generated [n])."""
    r_losses = [torch.mean((1 - dr) ** 2) for dr in disc_real_outputs]
    g_losses = [torch.mean(dg**2) for dg in disc_generated_outputs]
    return torch.stack(r_losses), torch.stack(g_losses)


def generator_loss(disc_outputs):
    """losses.py:28-34: mean((1 - D(G))^2) per discriminator, [n]."""
    return torch.stack([torch.mean((1 - dg) ** 2) for dg in disc_outputs])


# ---------------------------------------------------------------------------------------------------------------------------
# Duration predictors (models.py:29-180) and text -> waveform inference (SynthesizerTrn.infer, models.py:1288-1323) through
# ttsdur_* (include/ttsdec.h)
# ---------------------------------------------------------------------------------------------------------------------------
class _DDSConv(nn.Module):
    """modules.DDSConv parameter layout (modules.py:84-115)."""

    def __init__(self, channels, kernel_size, n_layers, p_dropout=0.0):
        super().__init__()
        self.channels, self.kernel_size, self.n_layers, self.p_dropout = channels, kernel_size, n_layers, p_dropout
        self.drop = nn.Dropout(p_dropout)
        self.convs_sep, self.convs_1x1 = nn.ModuleList(), nn.ModuleList()
        self.norms_1, self.norms_2 = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            dilation = kernel_size**i
            padding = (kernel_size * dilation - dilation) // 2
            self.convs_sep.append(nn.Conv1d(channels, channels, kernel_size, groups=channels, dilation=dilation, padding=padding))
            self.convs_1x1.append(nn.Conv1d(channels, channels, 1))
            self.norms_1.append(_LayerNorm(channels))
            self.norms_2.append(_LayerNorm(channels))

    def weight_tensors(self) -> List[torch.Tensor]:
        out = []
        for i in range(self.n_layers):
            out += [self.convs_sep[i].weight, self.convs_sep[i].bias, self.convs_1x1[i].weight, self.convs_1x1[i].bias,
                    self.norms_1[i].gamma, self.norms_1[i].beta, self.norms_2[i].gamma, self.norms_2[i].beta]
        return out


class _ConvFlow(nn.Module):
    """modules.ConvFlow parameter layout (modules.py:459-482), num_bins 10."""

    def __init__(self, in_channels, filter_channels, kernel_size, n_layers, num_bins=10, tail_bound=5.0):
        super().__init__()
        self.in_channels, self.filter_channels, self.kernel_size, self.n_layers = in_channels, filter_channels, kernel_size, n_layers
        self.num_bins, self.tail_bound, self.half_channels = num_bins, tail_bound, in_channels // 2
        self.pre = nn.Conv1d(self.half_channels, filter_channels, 1)
        self.convs = _DDSConv(filter_channels, kernel_size, n_layers, p_dropout=0.0)
        self.proj = nn.Conv1d(filter_channels, self.half_channels * (num_bins * 3 - 1), 1)
        self.proj.weight.data.zero_()
        self.proj.bias.data.zero_()

    def weight_tensors(self) -> List[torch.Tensor]:
        return [self.pre.weight, self.pre.bias] + self.convs.weight_tensors() + [self.proj.weight, self.proj.bias]


class _ElementwiseAffine(nn.Module):  # modules.ElementwiseAffine (modules.py:384-390)
    def __init__(self, channels):
        super().__init__()
        self.channels = channels
        self.m = nn.Parameter(torch.zeros(channels, 1))
        self.logs = nn.Parameter(torch.zeros(channels, 1))


class _Log(nn.Module):  # modules.Log: no parameters (training direction only)
    pass


class DurEngine(Handle):
    """One ttsdur handle on one device."""

    PREFIX = "ttsdur"

    def __init__(self, dims: Dict, device: torch.device):
        super().__init__(dims, _lib.DurDims(*[int(dims[n]) for n, _ in _lib.DurDims._fields_]), device)

    def logw(self, x_cl: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor], noise: Optional[torch.Tensor] = None,
             noise_scale: float = 1.0) -> torch.Tensor:
        """x_cl [B, T, C] contiguous fp32, lengths [B] int32 (device), g [B, gin] or None; noise [B, 2, T] (SDP) -> logw [B, T]."""
        B, T, _ = x_cl.shape
        ws = self.sized_workspace("logw", "ttsdur_workspace_bytes", B, T)
        out = torch.empty(B, T, device=self.device)
        if self.dims["kind"] == _lib.DUR_SDP:
            self.call("ttsdur_sdp_reverse", x_cl, lengths, g, noise, float(noise_scale), B, T, out, WS(ws), STREAM)
        else:
            self.call("ttsdur_dp_forward", x_cl, lengths, g, B, T, out, WS(ws), STREAM)
        return out

    def lengths(self, logw: torch.Tensor, x_lengths: torch.Tensor, length_scale: float):
        """-> cum [B, T] int32, y_len [B] int32 and (max y_len, flags) read back: the call's one host sync."""
        B, T = logw.shape
        cum = torch.empty(B, T, dtype=torch.int32, device=self.device)
        y_len = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(2, dtype=torch.int32, device=self.device)
        self.call("ttsdur_lengths", logw, x_lengths, float(length_scale), B, T, cum, y_len, status, STREAM)
        T_y, flags = status.tolist()
        if flags & 1:
            raise ValueError("non-finite duration: exp(logw) * length_scale is inf or nan for some token")
        if flags & 2:
            raise ValueError("the durations of an utterance sum beyond 2^24 frames, where fp32 stops counting frames exactly")
        return cum, y_len, T_y

    def expand(self, cum, m_cl, logs_cl, eps, noise_scale, T_y, with_attn=True):
        """-> z_p, m_p, logs_p [B, T_y, C] channel-last and attn [B, T_y, T] (include/ttsdec.h ttsdur_expand)."""
        B, T, Cc = m_cl.shape
        if eps.dim() != 3 or eps.shape[0] != B or eps.shape[1] != Cc or eps.shape[2] < T_y:
            raise ValueError(f"the prior noise must be [B, C, >= T_y] = [{B}, {Cc}, >= {T_y}], got {tuple(eps.shape)}")
        eps = eps.to(device=self.device, dtype=torch.float32).contiguous()
        z_p = torch.empty(B, T_y, Cc, device=self.device)
        m_p = torch.empty_like(z_p)
        logs_p = torch.empty_like(z_p)
        attn = torch.empty(B, T_y, T, device=self.device) if with_attn else None
        self.call("ttsdur_expand", cum, m_cl, logs_cl, eps, eps.shape[2], float(noise_scale), B, T, Cc, T_y, z_p, m_p, logs_p, attn, STREAM)
        return z_p, m_p, logs_p, attn


class DurNllEngine(Handle):
    """One ttsvits_durnll handle on one device: the stochastic duration predictor's likelihood (its forward direction)."""

    PREFIX = "ttsvits_durnll"

    def __init__(self, dims: Dict, device: Optional[torch.device]):
        super().__init__(dims, _lib.DurNllDims(*[int(dims[n]) for n, _ in _lib.DurNllDims._fields_]), device)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self._fn("workspace_bytes")(self._h, B, T))

    def forward(self, x_cl: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor], w: torch.Tensor, noise: torch.Tensor,
                parts: bool = False):
        """x_cl [B, T, C], w [B, T], noise [B, 2, T] contiguous fp32, lengths [B] int32 (device), g [B, gin] or None -> nll [B]
        (, terms [B, 4], z [B, 2, T] with ``parts``)."""
        B, T, _ = x_cl.shape
        ws = self.workspace("call", self.workspace_bytes(B, T))
        nll = torch.empty(B, device=self.device)
        terms = torch.empty(B, 4, device=self.device) if parts else None
        z = torch.empty(B, 2, T, device=self.device) if parts else None
        self.call("ttsvits_durnll_forward", x_cl, lengths, g, w, noise, B, T, nll, terms, z, WS(ws), STREAM)
        return (nll, terms, z) if parts else nll


class _TokenOperandsMixin:
    """The reference's [B, C, T] / [B, 1, T] operands as the token-row kernels take them (duration predictors and discriminators)."""

    @staticmethod
    def _channel_last(x: torch.Tensor) -> torch.Tensor:
        """[B, C, T] -> [B, T, C] contiguous; a transposed view of a channel-last buffer (what TextEncoder returns) is not copied."""
        xc = x.transpose(1, 2)
        return xc if xc.is_contiguous() else xc.contiguous()

    @staticmethod
    def _lengths(x_mask: torch.Tensor) -> torch.Tensor:
        return x_mask[:, 0, :].sum(dim=1).round().to(torch.int32)  # sequence_mask is a prefix mask


class _DurationBase(_TokenOperandsMixin, PackedWeightsMixin, nn.Module):
    def _check(self, x: torch.Tensor) -> None:
        inference_only(self, "duration predictor", x, fp32=True)

    def _speaker(self, g: Optional[torch.Tensor], B: int) -> Optional[torch.Tensor]:
        return speaker_rows(g, B, self.gin_channels, "a duration predictor")

    def _engine(self, device) -> DurEngine:
        eng = self._engines.get(self._cfg, device)
        eng.ensure_packed(self.weight_tensors())
        return eng


class StochasticDurationPredictor(_DurationBase):
    """models.StochasticDurationPredictor (models.py:29-137): same constructor, parameters and state-dict keys (the training-only
    post_* modules and flows.1 included; the reverse pass does not read them).  ``forward(x, x_mask, g=g, reverse=True,
    noise_scale=...) -> logw [B, 1, T]`` runs in the HIP library in exact fp32; ``forward`` in the other direction raises, and
    what it would return in eval mode - the likelihood nll [B] of given durations - is ``nll(x, x_mask, w, g=g)``, a method of its
    own with a handle and a blob of its own (every parameter of the module).  ``noise=`` (keyword, test hook) replaces the
    reference's draw torch.randn(B, 2, T) on the CPU generator in either direction."""

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout, n_flows=4, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        filter_channels = in_channels  # models.py:40
        self.in_channels, self.filter_channels, self.kernel_size, self.p_dropout = in_channels, filter_channels, kernel_size, p_dropout
        self.n_flows, self.gin_channels = n_flows, gin_channels
        self.log_flow = _Log()
        self.flows = nn.ModuleList()
        self.flows.append(_ElementwiseAffine(2))
        for _ in range(n_flows):
            self.flows.append(_ConvFlow(2, filter_channels, kernel_size, n_layers=3))
            self.flows.append(_Flip())
        self.post_pre = nn.Conv1d(1, filter_channels, 1)
        self.post_proj = nn.Conv1d(filter_channels, filter_channels, 1)
        self.post_convs = _DDSConv(filter_channels, kernel_size, n_layers=3, p_dropout=p_dropout)
        self.post_flows = nn.ModuleList()
        self.post_flows.append(_ElementwiseAffine(2))
        for _ in range(4):
            self.post_flows.append(_ConvFlow(2, filter_channels, kernel_size, n_layers=3))
            self.post_flows.append(_Flip())
        self.pre = nn.Conv1d(in_channels, filter_channels, 1)
        self.proj = nn.Conv1d(filter_channels, filter_channels, 1)
        self.convs = _DDSConv(filter_channels, kernel_size, n_layers=3, p_dropout=p_dropout)
        if gin_channels != 0:
            self.cond = nn.Conv1d(gin_channels, filter_channels, 1)
        self._cfg = dict(kind=_lib.DUR_SDP, in_channels=in_channels, filter_channels=filter_channels, kernel_size=kernel_size, n_flows=n_flows,
                         gin_channels=gin_channels)
        self._engines = EngineCache(DurEngine)
        self._nll_cfg = dict(in_channels=in_channels, kernel_size=kernel_size, n_flows=n_flows, gin_channels=gin_channels)
        self._nll_engines = EngineCache(DurNllEngine)

    @staticmethod
    def _trunk_tensors(pre, convs, proj, flows) -> List[torch.Tensor]:
        """A conditioning path, then the ElementwiseAffine its flows open with."""
        return [pre.weight, pre.bias] + convs.weight_tensors() + [proj.weight, proj.bias, flows[0].m, flows[0].logs]

    @staticmethod
    def _flow_tensors(flows, ks) -> List[torch.Tensor]:
        """The ConvFlows flows.{2k+1} for k in ks."""
        return [t for k in ks for t in flows[2 * k + 1].weight_tensors()]

    def _cond_tensors(self) -> List[torch.Tensor]:
        return [self.cond.weight, self.cond.bias] if self.gin_channels else []

    def nll_weight_tensors(self) -> List[torch.Tensor]:
        """ttsvits_durnll_pack_weights' order (include/ttsdec.h): every parameter of the module."""
        return (self._trunk_tensors(self.pre, self.convs, self.proj, self.flows) + self._flow_tensors(self.flows, range(self.n_flows))
                + self._trunk_tensors(self.post_pre, self.post_convs, self.post_proj, self.post_flows)
                + self._flow_tensors(self.post_flows, range(4)) + self._cond_tensors())

    @staticmethod
    def _noise(noise, B: int, T: int, device) -> torch.Tensor:
        """The noise operand of either direction: the caller's, or the reference's draw (models.py:95-98, 129-132)."""
        if noise is None:
            noise = torch.randn(B, 2, T)  # drawn on the CPU generator, then moved
        if tuple(noise.shape) != (B, 2, T):
            raise ValueError(f"noise must be [B, 2, T] = [{B}, 2, {T}], got {tuple(noise.shape)}")
        return noise.to(device=device, dtype=torch.float32).contiguous()

    def nll_cl(self, x_cl, lengths, w, g=None, *, noise=None, parts=False):
        """The likelihood on channel-last x [B, T, C] with lengths [B] and durations w [B, T] -> nll [B]; with ``parts`` also
        terms [B, 4] (include/ttsdec.h ttsvits_durnll_forward) and z [B, 2, T] after the last flow."""
        self._check(x_cl)
        B, T, _ = x_cl.shape
        if not w.is_cuda or w.dtype != torch.float32:
            raise NotImplementedError(f"the HIP duration likelihood takes fp32 durations on x's ROCm device ({x_cl.device}), got {w.dtype} on "
                                      f"{w.device}")
        if tuple(w.shape) != (B, T):
            raise ValueError(f"w must be [B, T] = [{B}, {T}], got {tuple(w.shape)}")
        noise = self._noise(noise, B, T, x_cl.device)
        eng = self._nll_engines.get(self._nll_cfg, x_cl.device)
        eng.ensure_packed(self.nll_weight_tensors())
        return eng.forward(x_cl.to(torch.float32).contiguous(), lengths.to(device=x_cl.device, dtype=torch.int32).contiguous(),
                           self._speaker(g, B), w.detach().to(device=x_cl.device).contiguous(), noise, parts)

    def nll(self, x, x_mask, w, g=None, *, noise=None) -> torch.Tensor:
        """What the reference's ``forward(x, x_mask, w, g=g)`` returns in eval mode: x [B, C, T], w [B, 1, T] -> nll [B]."""
        self._check(x)
        if w.dim() != 3 or w.shape[1] != 1:
            raise ValueError(f"w must be [B, 1, T], got {tuple(w.shape)}")
        return self.nll_cl(self._channel_last(x), self._lengths(x_mask), w[:, 0], g, noise=noise)

    def weight_tensors(self) -> List[torch.Tensor]:
        """ttsdur_pack_weights' order (include/ttsdec.h): what the reverse pass reads, the main half without flows.1."""
        return (self._trunk_tensors(self.pre, self.convs, self.proj, self.flows) + self._flow_tensors(self.flows, range(1, self.n_flows))
                + self._cond_tensors())

    def logw_cl(self, x_cl, lengths, g=None, noise_scale=1.0, noise=None) -> torch.Tensor:
        """Reverse pass on channel-last x [B, T, C] with lengths [B] -> logw [B, T] (``infer`` chains it)."""
        self._check(x_cl)
        B, T, _ = x_cl.shape
        noise = self._noise(noise, B, T, x_cl.device)
        eng = self._engine(x_cl.device)
        return eng.logw(x_cl.to(torch.float32).contiguous(), lengths.to(device=x_cl.device, dtype=torch.int32).contiguous(),
                        self._speaker(g, B), noise, noise_scale)

    def forward(self, x, x_mask, w=None, g=None, reverse=False, noise_scale=1.0, *, noise=None):
        if not reverse:
            raise NotImplementedError("forward() of the HIP stochastic duration predictor runs the reverse (inference) direction only; the "
                                      "likelihood of given durations is nll(x, x_mask, w, g=g)")
        self._check(x)
        return self.logw_cl(self._channel_last(x), self._lengths(x_mask), g, noise_scale, noise).unsqueeze(1)


class DurationPredictor(_DurationBase):
    """models.DurationPredictor (models.py:140-180): same constructor, parameters and state-dict keys; ``forward(x, x_mask,
    g=None) -> logw [B, 1, T]`` in the HIP library in exact fp32, inference only."""

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        self.in_channels, self.filter_channels, self.kernel_size, self.p_dropout, self.gin_channels = (
            in_channels, filter_channels, kernel_size, p_dropout, gin_channels)
        self.drop = nn.Dropout(p_dropout)
        self.conv_1 = nn.Conv1d(in_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_1 = _LayerNorm(filter_channels)
        self.conv_2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_2 = _LayerNorm(filter_channels)
        self.proj = nn.Conv1d(filter_channels, 1, 1)
        if gin_channels != 0:
            self.cond = nn.Conv1d(gin_channels, in_channels, 1)
        self._cfg = dict(kind=_lib.DUR_DP, in_channels=in_channels, filter_channels=filter_channels, kernel_size=kernel_size, n_flows=0,
                         gin_channels=gin_channels)
        self._engines = EngineCache(DurEngine)

    def weight_tensors(self) -> List[torch.Tensor]:
        out = [self.conv_1.weight, self.conv_1.bias, self.norm_1.gamma, self.norm_1.beta, self.conv_2.weight, self.conv_2.bias,
               self.norm_2.gamma, self.norm_2.beta, self.proj.weight, self.proj.bias]
        if self.gin_channels:
            out += [self.cond.weight, self.cond.bias]
        return out

    def logw_cl(self, x_cl, lengths, g=None, noise_scale=1.0, noise=None) -> torch.Tensor:
        """forward on channel-last x [B, T, C] with lengths [B] -> logw [B, T] (noise_scale / noise: unused)."""
        self._check(x_cl)
        eng = self._engine(x_cl.device)
        return eng.logw(x_cl.to(torch.float32).contiguous(), lengths.to(device=x_cl.device, dtype=torch.int32).contiguous(),
                        self._speaker(g, x_cl.shape[0]))

    def forward(self, x, x_mask, g=None):
        self._check(x)
        return self.logw_cl(self._channel_last(x), self._lengths(x_mask), g).unsqueeze(1)


# ---------------------------------------------------------------------------------------------------------------------------
# Duration discriminators (models.py:183-329) through ttsvits_durdisc_* (include/ttsdec.h)
# ---------------------------------------------------------------------------------------------------------------------------
class DurDiscEngine(Handle):
    """One ttsvits_durdisc handle on one device: DurationDiscriminatorV1 or V2 (dims["version"])."""

    PREFIX = "ttsvits_durdisc"

    def __init__(self, dims: Dict, device: Optional[torch.device]):
        super().__init__(dims, _lib.DurDiscDims(*[int(dims[n]) for n, _ in _lib.DurDiscDims._fields_]), device)

    def workspace_bytes(self, B: int, T: int, n_dur: int = 2) -> int:
        return int(self._fn("workspace_bytes")(self._h, B, T, n_dur))

    def _workspace(self, B: int, T: int, n_dur: int, what: str) -> torch.Tensor:
        return self.sized_workspace("call", "ttsvits_durdisc_workspace_bytes", B, T, n_dur, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, what, f"B = {B}, T = {T}: the row indices leave 32 bits; split the batch"))

    def trunk(self, x_cl: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        """x_cl [B, T, C] contiguous fp32, lengths [B] int32 (device) -> hidden [B, T, F], zero at masked tokens."""
        B, T, _ = x_cl.shape
        ws = self._workspace(B, T, 1, "ttsvits_durdisc_trunk")
        out = torch.empty(B, T, self.dims["filter_channels"], device=self.device)
        self.call("ttsvits_durdisc_trunk", x_cl, lengths, B, T, out, WS(ws), STREAM)
        return out

    def prob(self, hidden_cl: torch.Tensor, lengths: torch.Tensor, dur: torch.Tensor, with_logits: bool = False):
        """hidden_cl [B, T, F], dur [n_dur, B, T] (n_dur 1 or 2), both contiguous fp32 -> (prob [n_dur, B, T], logits or None)."""
        n_dur, B, T = dur.shape
        ws = self._workspace(B, T, n_dur, "ttsvits_durdisc_prob")
        prob = torch.empty(n_dur, B, T, device=self.device)
        logit = torch.empty_like(prob) if with_logits else None
        self.call("ttsvits_durdisc_prob", hidden_cl, lengths, dur, n_dur, B, T, prob, logit, WS(ws), STREAM)
        return prob, logit


class _DurationDiscriminatorBase(_TokenOperandsMixin, PackedWeightsMixin, nn.Module):
    """What DurationDiscriminatorV1 and V2 share: the reference's constructor, parameters and state-dict keys, and the two calls.
    Inference only, exact fp32, eval mode; ``gin_channels`` and ``g`` are accepted and ignored, as the reference does."""

    VERSION = 0

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        self.in_channels, self.filter_channels, self.kernel_size, self.p_dropout, self.gin_channels = (
            in_channels, filter_channels, kernel_size, p_dropout, gin_channels)
        pad = kernel_size // 2
        if self.VERSION == 1:
            self.drop = nn.Dropout(p_dropout)
        self.conv_1 = nn.Conv1d(in_channels, filter_channels, kernel_size, padding=pad)
        if self.VERSION == 2:
            self.norm_1 = _LayerNorm(filter_channels)
        self.conv_2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=pad)
        if self.VERSION == 2:
            self.norm_2 = _LayerNorm(filter_channels)
        self.dur_proj = nn.Conv1d(1, filter_channels, 1)
        self.pre_out_conv_1 = nn.Conv1d(2 * filter_channels, filter_channels, kernel_size, padding=pad)
        self.pre_out_norm_1 = _LayerNorm(filter_channels)  # (V1 owns both pre_out norms and never uses them: models.py:211-215)
        self.pre_out_conv_2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=pad)
        self.pre_out_norm_2 = _LayerNorm(filter_channels)
        self.output_layer = nn.Sequential(nn.Linear(filter_channels, 1), nn.Sigmoid())
        self._cfg = dict(version=self.VERSION, in_channels=in_channels, filter_channels=filter_channels, kernel_size=kernel_size)
        self._engines = EngineCache(DurDiscEngine)

    def weight_tensors(self) -> List[torch.Tensor]:
        """ttsvits_durdisc_pack_weights' order (include/ttsdec.h): the state dict's, without V1's unused norms."""
        def norm(name):  # (V2 only: V1 has no trunk norms and does not use its pre_out ones)
            return [getattr(self, name).gamma, getattr(self, name).beta] if self.VERSION == 2 else []

        out = [self.conv_1.weight, self.conv_1.bias] + norm("norm_1") + [self.conv_2.weight, self.conv_2.bias] + norm("norm_2")
        out += [self.dur_proj.weight, self.dur_proj.bias, self.pre_out_conv_1.weight, self.pre_out_conv_1.bias] + norm("pre_out_norm_1")
        out += [self.pre_out_conv_2.weight, self.pre_out_conv_2.bias] + norm("pre_out_norm_2")
        return out + [self.output_layer[0].weight, self.output_layer[0].bias]

    def _engine(self, device) -> DurDiscEngine:
        eng = self._engines.get(self._cfg, device)
        eng.ensure_packed(self.weight_tensors())
        return eng

    def _operands(self, x, x_mask, channels: int, durs):
        """The checks both calls share -> (x channel-last, lengths [B] int32, dur [n_dur, B, T] contiguous)."""
        if x.dim() != 3 or x.shape[1] != channels or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"x must be [B, {channels}, T], got {tuple(x.shape)}")
        B, _, T = x.shape
        if x_mask.dim() != 3 or tuple(x_mask.shape) != (B, 1, T):
            raise ValueError(f"x_mask must be [B, 1, T] = [{B}, 1, {T}], got {tuple(x_mask.shape)}")
        for d in durs:
            if d.dim() != 3 or tuple(d.shape) != (B, 1, T):
                raise ValueError(f"a duration tensor must be [B, 1, T] = [{B}, 1, {T}], got {tuple(d.shape)}")
        inference_only(self, "duration discriminator", x, fp32=True)
        # (the kernels read the lengths and the durations through raw device pointers: every operand on x's device, or no launch)
        if x_mask.device != x.device:
            raise NotImplementedError(f"the HIP duration discriminator takes x_mask on x's ROCm device ({x.device}), got {x_mask.device}")
        for d in durs:
            if d.device != x.device or d.dtype != torch.float32:
                raise NotImplementedError(f"the HIP duration discriminator takes fp32 durations on x's ROCm device ({x.device}), got "
                                          f"{d.dtype} on {d.device}")
        dur = torch.stack([d.detach()[:, 0] for d in durs]).contiguous() if durs else None
        lengths = self._lengths(x_mask.detach()).to(device=x.device, dtype=torch.int32).contiguous()
        return self._channel_last(x.detach()), lengths, dur

    def trunk(self, x, x_mask) -> torch.Tensor:
        """forward up to its loop over the durations: x [B, C, T] -> h * x_mask [B, F, T] (a transposed view of the library's
        channel-last buffer) - what ``forward_probability`` takes."""
        x_cl, lengths, _ = self._operands(x, x_mask, self.in_channels, [])
        return self._engine(x.device).trunk(x_cl, lengths).transpose(1, 2)

    def probabilities(self, x, x_mask, durs, with_logits: bool = False):
        """forward_probability for one or two duration tensors [B, 1, T] in one call on the trunk's output x [B, F, T] ->
        (prob [n_dur, B, T], the pre-sigmoid logits or None)."""
        h_cl, lengths, dur = self._operands(x, x_mask, self.filter_channels, list(durs))
        return self._engine(x.device).prob(h_cl, lengths, dur, with_logits)

    def forward_probability(self, x, x_mask, dur, g=None):
        """models.py:222-236 / 298-310: x [B, F, T] (the trunk's output), dur [B, 1, T] -> output_prob [B, T, 1]."""
        return self.probabilities(x, x_mask, [dur])[0][0].unsqueeze(-1)

    def _pair(self, x, x_mask, dur_r, dur_hat):
        x_cl, lengths, dur = self._operands(x, x_mask, self.in_channels, [dur_r, dur_hat])
        eng = self._engine(x.device)
        prob, _ = eng.prob(eng.trunk(x_cl, lengths), lengths, dur)
        return prob[0].unsqueeze(-1), prob[1].unsqueeze(-1)


class DurationDiscriminatorV1(_DurationDiscriminatorBase):
    """models.DurationDiscriminatorV1 (models.py:183-257): same constructor, parameters and state-dict keys (the pre_out norms it
    never uses included); ``forward(x, x_mask, dur_r, dur_hat, g=None) -> [p_r, p_hat]``, each [B, T, 1]."""

    VERSION = 1

    def forward(self, x, x_mask, dur_r, dur_hat, g=None):
        return list(self._pair(x, x_mask, dur_r, dur_hat))


class DurationDiscriminatorV2(_DurationDiscriminatorBase):
    """models.DurationDiscriminatorV2 (models.py:260-329): same constructor, parameters and state-dict keys;
    ``forward(x, x_mask, dur_r, dur_hat, g=None) -> [[p_r], [p_hat]]``, each [B, T, 1]."""

    VERSION = 2

    def forward(self, x, x_mask, dur_r, dur_hat, g=None):
        return [[p] for p in self._pair(x, x_mask, dur_r, dur_hat)]


def infer(net_g, x, x_lengths, sid=None, noise_scale=1, length_scale=1, noise_scale_w=1.0, max_len=None, *, noise=None):
    """SynthesizerTrn.infer (models.py:1288-1323) for a model whose enc_p / dp / flow / dec are this module's drop-ins (emb_g,
    when present, is the reference's nn.Embedding): -> (o [B, 1, T'], attn [B, 1, T_y, T_x], y_mask [B, 1, T_y],
    (z, z_p, m_p, logs_p) [B, inter, T_y]).  Channel-last from the text encoder to the generator; one host sync (T_y).
    ``noise=(e_w, e_z)`` (test hook) replaces the two draws: e_w [B, 2, T_x] of the stochastic duration predictor, e_z
    [B, inter, >= T_y] of the prior (torch.randn_like(m_p))."""
    parts = {"enc_p": TextEncoder, "dp": (StochasticDurationPredictor, DurationPredictor), "flow": ResidualCouplingTransformersBlock,
             "dec": Generator}
    for name, cls in parts.items():
        mod = getattr(net_g, name, None)
        if not isinstance(mod, cls):
            raise TypeError(f"net_g.{name} is {type(mod).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    enc_p, dp, flow, dec = net_g.enc_p, net_g.dp, net_g.flow, net_g.dec
    if not x.is_cuda:
        raise NotImplementedError("vits2.infer runs on a ROCm device only: move the model and the ids there")
    e_w, e_z = noise if noise is not None else (None, None)
    g = None if sid is None else net_g.emb_g(sid).unsqueeze(-1)  # [b, h, 1]
    dev = x.device
    xs, m_cl, logs_cl = enc_p.forward_cl(x, x_lengths, g=g if enc_p.gin_channels else None)  # (models.py:1154-1157: g reaches the
    # text encoder's layers only when it was built speaker-conditioned)
    lengths = x_lengths.to(device=dev, dtype=torch.int32).contiguous()
    logw = dp.logw_cl(xs, lengths, g, noise_scale_w, e_w)
    eng = dp._engines.get(dp._cfg, dev)
    cum, y_len, T_y = eng.lengths(logw, lengths, length_scale)
    if e_z is None:
        e_z = torch.randn(x.shape[0], m_cl.shape[2], T_y, device=dev)  # torch.randn_like(m_p)
    z_p, m_p, logs_p, attn = eng.expand(cum, m_cl, logs_cl, e_z, noise_scale, T_y)
    y_mask = (torch.arange(T_y, device=dev)[None, :] < y_len[:, None]).unsqueeze(1).to(torch.float32)
    z = flow.reverse_cl(z_p, y_len, g)
    o = dec.forward_cl((z * y_mask.transpose(1, 2))[:, :max_len], g).unsqueeze(1)
    return o, attn.unsqueeze(1), y_mask, (z.transpose(1, 2), z_p.transpose(1, 2), m_p.transpose(1, 2), logs_p.transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# Posterior encoder (models.py:858-897) through ttspost_* and voice conversion (SynthesizerTrn.voice_conversion, models.py:1328-1336)
# ---------------------------------------------------------------------------------------------------------------------------
class PostEngine(Handle):
    """One ttspost handle on one device."""

    PREFIX = "ttspost"

    def __init__(self, dims: Dict, device: torch.device):
        super().__init__(dims, _lib.PostDims(*[int(dims[n]) for n, _ in _lib.PostDims._fields_]), device)

    def forward(self, y: torch.Tensor, lengths: torch.Tensor, g: Optional[torch.Tensor], eps: torch.Tensor):
        """y [B, spec, T] contiguous fp32, lengths [B] int32 (device), g [B, gin] or None, eps [B, inter, >= T] -> z, m, logs
        [B, T, inter] channel-last."""
        B, _, T = y.shape
        I = self.dims["inter_channels"]
        ws = self.sized_workspace("forward", "ttspost_workspace_bytes", B, T)
        z = torch.empty(B, T, I, device=self.device)
        m = torch.empty_like(z)
        logs = torch.empty_like(z)
        self.call("ttspost_forward", y, lengths, g, eps, eps.shape[2], B, T, z, m, logs, WS(ws), STREAM)
        return z, m, logs


class PosteriorEncoder(PackedWeightsMixin, nn.Module):
    """models.PosteriorEncoder (models.py:858-897): same constructor, parameters and state-dict keys (``enc`` is the weight-normed
    modules.WN).  ``forward(x [B, spec, T], x_lengths, g=None) -> (z, m, logs, x_mask)`` runs in the HIP library; inference only,
    dilation_rate 1.  ``noise=`` (keyword, test hook) replaces the reference's draw torch.randn_like(m): [B, out_channels, >= T]."""

    def __init__(self, in_channels, out_channels, hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=0):
        super().__init__()
        self._watch_state_dict_loads()
        if dilation_rate != 1:
            raise NotImplementedError("PosteriorEncoder with dilation_rate != 1 is outside the HIP path")
        self.in_channels, self.out_channels, self.hidden_channels = in_channels, out_channels, hidden_channels
        self.kernel_size, self.dilation_rate, self.n_layers, self.gin_channels = kernel_size, dilation_rate, n_layers, gin_channels
        self.pre = nn.Conv1d(in_channels, hidden_channels, 1)
        self.enc = _WN(hidden_channels, kernel_size, dilation_rate, n_layers, gin_channels=gin_channels)
        self.proj = nn.Conv1d(hidden_channels, out_channels * 2, 1)
        self.precision = "f32"  # arithmetic of the GEMMs: "f32" (the reference's own: exact fp32, default) or "split_f16" (two fp16 planes, opt-in)
        self._cfg = dict(spec_channels=in_channels, inter_channels=out_channels, hidden_channels=hidden_channels, kernel_size=kernel_size,
                         n_layers=n_layers, gin_channels=gin_channels)
        self._engines = EngineCache(PostEngine)

    def weight_tensors(self) -> List[torch.Tensor]:
        """ttspost_pack_weights' order (include/ttsdec.h), weight-normed convs as their effective weights."""
        return [self.pre.weight, self.pre.bias] + self.enc.weight_tensors() + [self.proj.weight, self.proj.bias]

    def forward_cl(self, x, x_lengths, g=None, *, noise=None):
        """forward on the reference's x [B, spec, T] -> z, m, logs channel-last [B, T, out_channels] (``voice_conversion`` chains it)."""
        inference_only(self, "posterior encoder", x)
        B, S, T = x.shape
        if S != self.in_channels:
            raise ValueError(f"x must be [B, in_channels, T] with in_channels = {self.in_channels}, got {tuple(x.shape)}")
        dev = x.device
        if noise is None:
            noise = torch.randn(B, self.out_channels, T, device=dev)  # torch.randn_like(m), models.py:894
        if noise.dim() != 3 or noise.shape[0] != B or noise.shape[1] != self.out_channels or noise.shape[2] < T:
            raise ValueError(f"noise must be [B, out_channels, >= T] = [{B}, {self.out_channels}, >= {T}], got {tuple(noise.shape)}")
        g = speaker_rows(g, B, self.gin_channels, "a posterior encoder")
        eng = self._engines.get(self._cfg, dev)
        eng.set_precision(self.precision)
        eng.ensure_packed(self.weight_tensors, key_tensors=list(self.parameters()))
        lengths = x_lengths.to(device=dev, dtype=torch.int32).contiguous()
        return eng.forward(x.to(torch.float32).contiguous(), lengths, g, noise.to(device=dev, dtype=torch.float32).contiguous())

    def forward(self, x, x_lengths, g=None, *, noise=None):
        z, m, logs = self.forward_cl(x, x_lengths, g, noise=noise)
        T = x.shape[2]
        x_mask = (torch.arange(T, device=x.device)[None, :] < x_lengths.to(x.device)[:, None]).unsqueeze(1).to(z.dtype)
        return z.transpose(1, 2), m.transpose(1, 2), logs.transpose(1, 2), x_mask


def voice_conversion(net_g, y, y_lengths, sid_src, sid_tgt, *, noise=None):
    """SynthesizerTrn.voice_conversion (models.py:1328-1336) for a model whose enc_q / flow / dec are this module's drop-ins (emb_g is the
    reference's nn.Embedding): y [B, spec, T] -> (o_hat [B, 1, T * hop], y_mask [B, 1, T], (z, z_p, z_hat) [B, inter, T]).
    Channel-last from the posterior encoder to the generator, no host sync.  ``noise`` (test hook) replaces the posterior's draw
    torch.randn_like(m): [B, inter, >= T]."""
    parts = {"enc_q": PosteriorEncoder, "flow": ResidualCouplingTransformersBlock, "dec": Generator}
    for name, cls in parts.items():
        mod = getattr(net_g, name, None)
        if not isinstance(mod, cls):
            raise TypeError(f"net_g.{name} is {type(mod).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    # (models.py:1329 asserts on self.n_speakers, which SynthesizerTrn.__init__ does not store: without the attribute, the speaker count
    # is emb_g's - a model built with n_speakers <= 1 has no emb_g)
    emb_g = getattr(net_g, "emb_g", None)
    n_speakers = getattr(net_g, "n_speakers", emb_g.num_embeddings if emb_g is not None else 0)
    assert n_speakers > 0, "n_speakers have to be larger than 0."
    enc_q, flow, dec = net_g.enc_q, net_g.flow, net_g.dec
    if not y.is_cuda:
        raise NotImplementedError("vits2.voice_conversion runs on a ROCm device only: move the model and the spectrogram there")
    g_src = net_g.emb_g(sid_src).unsqueeze(-1)
    g_tgt = net_g.emb_g(sid_tgt).unsqueeze(-1)
    dev = y.device
    lengths = y_lengths.to(device=dev, dtype=torch.int32).contiguous()
    z, _, _ = enc_q.forward_cl(y, lengths, g=g_src, noise=noise)
    z_p = flow.forward_cl(z, lengths, g_src)
    z_hat = flow.reverse_cl(z_p, lengths, g_tgt)
    T = y.shape[2]
    y_mask = (torch.arange(T, device=dev)[None, :] < lengths[:, None]).unsqueeze(1).to(torch.float32)
    o_hat = dec.forward_cl(z_hat * y_mask.transpose(1, 2), g_tgt).unsqueeze(1)
    return o_hat, y_mask, (z.transpose(1, 2), z_p.transpose(1, 2), z_hat.transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# Monotonic alignment search (models.py:1224-1254, monotonic_align/) through ttsvits_neg_cent / ttsvits_maximum_path, forced alignment
# ---------------------------------------------------------------------------------------------------------------------------
_ALIGN_ENGINES = EngineCache(VitsEngine)  # weightless handles of the stand-alone calls, one per device
_ALIGN_DIMS = dict(n_vocab=1, inter_channels=8, hidden_channels=4, filter_channels=4, n_heads=1, n_layers=0, kernel_size=1, window_size=0,
                   **_DEFAULT_FLOW)  # (any valid dims)


def _align_engine(device: torch.device, eng: Optional[VitsEngine] = None) -> VitsEngine:
    return eng if eng is not None else _ALIGN_ENGINES.get(_ALIGN_DIMS, device)


def _mask_lengths(mask: torch.Tensor):
    """t_y, t_x [B] int32 of a [B, T_y, T_x] mask, as the reference's wrapper takes them (monotonic_align/__init__.py:16-17)."""
    return (mask.sum(1)[:, 0].to(torch.int32).contiguous(), mask.sum(2)[:, 0].to(torch.int32).contiguous())


def maximum_path(neg_cent, mask):
    """monotonic_align.maximum_path (monotonic_align/__init__.py:6-19) on the device: neg_cent, mask [b, t_t, t_s] -> path [b, t_t, t_s]
    in neg_cent's dtype and on its device, equal to the reference's.  The lengths are mask.sum(1)[:, 0] / mask.sum(2)[:, 0], computed
    on the device; the one host read is the status word (ValueError where the reference would read out of bounds: an utterance
    with t_t < t_s, or an empty one)."""
    if not neg_cent.is_cuda or not mask.is_cuda:
        raise NotImplementedError("vits2.maximum_path runs on a ROCm device only: there is no CPU fallback")
    if neg_cent.dim() != 3 or tuple(mask.shape) != tuple(neg_cent.shape):
        raise ValueError(f"neg_cent and mask must both be [b, t_t, t_s], got {tuple(neg_cent.shape)} and {tuple(mask.shape)}")
    t_y, t_x = _mask_lengths(mask)
    eng = _align_engine(neg_cent.device)
    return eng.maximum_path(neg_cent.detach().to(torch.float32).contiguous(), t_y, t_x, neg_cent.dtype)[0]


def _align_cl(eng: VitsEngine, z_cl, m_cl, logs_cl, t_y, t_x, mas_noise_scale=None, noise=None, also=None):
    """neg_cent and the search on channel-last operands -> (path [B, T_y, T_x] fp32, frame_token, dur, neg_cent).  also: see
    VitsEngine.maximum_path."""
    z_cl, m_cl, logs_cl = (t.detach().to(torch.float32).contiguous() for t in (z_cl, m_cl, logs_cl))
    if mas_noise_scale is None:
        B, T_y, _ = z_cl.shape
        nc = torch.empty(B, T_y, m_cl.shape[1], device=z_cl.device)
        path, ft, dur = eng.maximum_path(nc, t_y, t_x, torch.float32, z_cl, m_cl, logs_cl, also=also)
        return path, ft, dur, nc
    # models.py:1241-1247 on the unmasked cost matrix, as the reference computes it
    nc = eng.neg_cent(z_cl, m_cl, logs_cl, None, None)
    if noise is None:
        noise = torch.randn_like(nc)
    if tuple(noise.shape) != tuple(nc.shape):
        raise ValueError(f"noise must be [B, T_y, T_x] = {tuple(nc.shape)}, got {tuple(noise.shape)}")
    nc = (nc + torch.std(nc) * noise.to(device=nc.device, dtype=torch.float32) * mas_noise_scale).contiguous()
    path, ft, dur = eng.maximum_path(nc, t_y, t_x, torch.float32, also=also)
    return path, ft, dur, nc


def align(z_p, m_p, logs_p, x_mask, y_mask, mas_noise_scale=None, *, noise=None):
    """The ``with torch.no_grad():`` block of SynthesizerTrn.forward (models.py:1224-1254): z_p [B, C, T_y], m_p / logs_p [B, C, T_x],
    x_mask [B, 1, T_x], y_mask [B, 1, T_y] -> attn [B, 1, T_y, T_x].  neg_cent and the search run in the HIP library; with
    ``mas_noise_scale`` the std(neg_cent) * randn * scale term is added by torch ops between the two (``noise`` [B, T_y, T_x], test
    hook, replaces the draw).  The one host read is the status word."""
    for name, t in dict(z_p=z_p, m_p=m_p, logs_p=logs_p, x_mask=x_mask, y_mask=y_mask).items():
        if not t.is_cuda:
            raise NotImplementedError(f"vits2.align runs on a ROCm device only ({name} is on {t.device}): there is no CPU fallback")
    if z_p.dim() != 3 or m_p.shape != logs_p.shape or m_p.shape[:2] != z_p.shape[:2] or z_p.shape[1] % 4:
        raise ValueError(f"z_p [B, C, T_y] and m_p / logs_p [B, C, T_x] with C a multiple of 4 expected, got {tuple(z_p.shape)}, "
                         f"{tuple(m_p.shape)}, {tuple(logs_p.shape)}")
    t_x = x_mask[:, 0, :].sum(1).to(torch.int32).contiguous()
    t_y = y_mask[:, 0, :].sum(1).to(torch.int32).contiguous()
    cl = _DurationBase._channel_last
    path, _, _, _ = _align_cl(_align_engine(z_p.device), cl(z_p), cl(m_p), cl(logs_p), t_y, t_x, mas_noise_scale, noise)
    return path.unsqueeze(1)


def forced_alignment(net_g, x, x_lengths, y, y_lengths, sid=None, *, mas_noise_scale=None, noise=None):
    """Token durations of a given utterance: SynthesizerTrn.forward up to ``logw_`` (models.py:1214-1263) for a model whose enc_p /
    enc_q / flow are this module's drop-ins - x [B, T_x] ids and y [B, spec, T_y] -> (attn [B, 1, T_y, T_x], w = attn.sum(2)
    [B, 1, T_x], logw_ = log(w + 1e-6) * x_mask [B, 1, T_x], (z, z_p, m_p, logs_p) as the reference's [B, inter, T]).  Channel-last
    from the encoders to the search; the one host read is the search's status word.  ``noise`` (test hook): the posterior's draw
    [B, inter, >= T_y], or a pair (posterior draw, MAS draw [B, T_y, T_x]) with ``mas_noise_scale``."""
    return _forced_alignment(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, {}, "vits2.forced_alignment")[:4]


def _forced_alignment(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, more_parts, caller):
    """forced_alignment's body -> its four results, then what ``duration_discriminator_scores`` goes on with: the text encoder's
    x channel-last [B, T_x, H], t_x [B] int32, x_mask [B, 1, T_x] and g.  more_parts: further drop-ins of net_g the caller needs."""
    p = _alignment_parts(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, more_parts, caller)
    zs = (p.z_cl.transpose(1, 2), p.zp_cl.transpose(1, 2), p.m_cl.transpose(1, 2), p.logs_cl.transpose(1, 2))
    return p.attn, p.w, p.logw_, zs, p.xs, p.t_x, p.x_mask, p.g


def _alignment_parts(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, more_parts, caller, also=None):
    """The encoders, the flow and the search, channel-last -> a namespace of everything they computed: attn [B, 1, T_y, T_x], w,
    logw_, x_mask, g, t_x, t_y, frame_token ``ft`` [B, T_y] int32, the weightless engine ``eng``, and channel-last xs [B, T_x, H],
    m_cl / logs_cl [B, T_x, inter] (the unexpanded prior), z_cl / zp_cl / mq_cl / logsq_cl [B, T_y, inter].  also: see
    VitsEngine.maximum_path."""
    from types import SimpleNamespace

    parts = {"enc_p": TextEncoder, "enc_q": PosteriorEncoder, "flow": ResidualCouplingTransformersBlock, **more_parts}
    for name, cls in parts.items():
        mod = getattr(net_g, name, None)
        if not isinstance(mod, cls):
            raise TypeError(f"net_g.{name} is {type(mod).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    if not x.is_cuda or not y.is_cuda:
        raise NotImplementedError(f"{caller} runs on a ROCm device only: move the model, the ids and the spectrogram there")
    enc_p, enc_q, flow = net_g.enc_p, net_g.enc_q, net_g.flow
    e_q, e_mas = noise if isinstance(noise, (tuple, list)) else (noise, None)
    g = None if sid is None else net_g.emb_g(sid).unsqueeze(-1)  # [b, h, 1]
    dev = x.device
    t_x = x_lengths.to(device=dev, dtype=torch.int32).contiguous()
    t_y = y_lengths.to(device=dev, dtype=torch.int32).contiguous()
    xs, m_cl, logs_cl = enc_p.forward_cl(x, t_x, g=g if enc_p.gin_channels else None)
    z_cl, mq_cl, logsq_cl = enc_q.forward_cl(y, t_y, g=g, noise=e_q)
    zp_cl = flow.forward_cl(z_cl, t_y, g)
    eng = flow._engines.get(flow._dims(), dev)  # (the flow's own handle: the calls are weightless)
    path, ft, dur, _ = _align_cl(eng, zp_cl, m_cl, logs_cl, t_y, t_x, mas_noise_scale, e_mas, also)
    w = dur.to(torch.float32).unsqueeze(1)
    x_mask = (torch.arange(x.shape[1], device=dev)[None, :] < t_x[:, None]).unsqueeze(1).to(torch.float32)
    logw_ = torch.log(w + 1e-6) * x_mask
    return SimpleNamespace(attn=path.unsqueeze(1), w=w, logw_=logw_, xs=xs, t_x=t_x, t_y=t_y, x_mask=x_mask, g=g, ft=ft, eng=eng, m_cl=m_cl,
                           logs_cl=logs_cl, z_cl=z_cl, zp_cl=zp_cl, mq_cl=mq_cl, logsq_cl=logsq_cl)


def duration_discriminator_scores(net_g, net_dur_disc, x, x_lengths, y, y_lengths, sid=None, *, noise_scale_w=1.0, mas_noise_scale=None,
                                  noise=None):
    """What the reference's trainer feeds and gets from its duration discriminator, ``net_dur_disc(hidden_x, x_mask, logw_, logw)``
    (train.py:385 / 414), in eval mode: SynthesizerTrn.forward up to ``(x, logw, logw_)`` (models.py:1214-1264) - the text encoder
    once, ``forced_alignment``'s body for logw_, and the duration predictor for logw: ``dp(x, x_mask, g=g, reverse=True,
    noise_scale=noise_scale_w)`` for a StochasticDurationPredictor, ``dp(x, x_mask, g=g)`` for a DurationPredictor - then the
    discriminator.  -> (y_dur_hat_r, y_dur_hat_g, (hidden_x [B, H, T_x], x_mask [B, 1, T_x], logw_, logw [B, 1, T_x])); the two
    outputs are what ``discriminator_loss`` / ``generator_loss`` take ([p] lists for V2, the tensors wrapped by the caller for
    V1, as train.py does).  ``noise`` (test hook): the pair (forced_alignment's ``noise``, the SDP's draw [B, 2, T_x] or None)."""
    if not isinstance(net_dur_disc, _DurationDiscriminatorBase):
        raise TypeError(f"net_dur_disc is {type(net_dur_disc).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    if noise is not None and not (isinstance(noise, (tuple, list)) and len(noise) == 2):
        raise ValueError("noise must be a pair: (forced_alignment's noise, the stochastic duration predictor's draw [B, 2, T_x] or None)")
    e_fa, e_w = noise if noise is not None else (None, None)
    _, _, logw_, _, xs, t_x, x_mask, g = _forced_alignment(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, e_fa,
                                                           {"dp": (StochasticDurationPredictor, DurationPredictor)},
                                                           "vits2.duration_discriminator_scores")
    logw = net_g.dp.logw_cl(xs, t_x, g, noise_scale_w, e_w).unsqueeze(1)
    hidden_x = xs.transpose(1, 2)
    y_dur_hat_r, y_dur_hat_g = net_dur_disc(hidden_x, x_mask, logw_, logw)
    return y_dur_hat_r, y_dur_hat_g, (hidden_x, x_mask, logw_, logw)


def duration_loss(net_g, x, x_lengths, y, y_lengths, sid=None, *, mas_noise_scale=None, noise=None):
    """The duration loss of a given utterance, SynthesizerTrn.forward up to models.py:1267 in eval mode, on ``forced_alignment``'s
    body -> (l_length [B], attn [B, 1, T_y, T_x], x_mask [B, 1, T_x], (hidden_x [B, H, T_x], logw, logw_ [B, 1, T_x])).  With a
    StochasticDurationPredictor l_length = dp.nll(x, x_mask, w, g=g) / sum(x_mask) and logw is its reverse pass at noise_scale
    1.0; with a DurationPredictor logw = dp(x, x_mask, g=g) and l_length = sum((logw - logw_)^2) / sum(x_mask).  The divisor is
    the whole batch's token count, as in the reference; ``l_length.sum()`` is the reference's VL/dur.  The one host read is the
    alignment's status word.  ``noise`` (test hook): the triple (forced_alignment's noise, the likelihood's draw e_q [B, 2, T_x]
    or None, the reverse pass's draw [B, 2, T_x] or None)."""
    if noise is not None and not (isinstance(noise, (tuple, list)) and len(noise) == 3):
        raise ValueError("noise must be a triple: (forced_alignment's noise, the likelihood's draw [B, 2, T_x] or None, the reverse pass's "
                         "draw [B, 2, T_x] or None)")
    e_fa, e_q, e_w = noise if noise is not None else (None, None, None)
    attn, w, logw_, _, xs, t_x, x_mask, g = _forced_alignment(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, e_fa,
                                                              {"dp": (StochasticDurationPredictor, DurationPredictor)}, "vits2.duration_loss")
    l_length, logw = _duration_terms(net_g.dp, xs, t_x, x_mask, w, logw_, g, e_q, e_w)
    return l_length, attn, x_mask, (xs.transpose(1, 2), logw, logw_)


def _duration_terms(dp, xs, t_x, x_mask, w, logw_, g, e_q, e_w):
    """models.py:1257-1267 on the alignment's w and logw_ -> (l_length [B], logw [B, 1, T_x])."""
    n_tokens = torch.sum(x_mask)
    if isinstance(dp, StochasticDurationPredictor):
        l_length = dp.nll_cl(xs, t_x, w[:, 0], g, noise=e_q) / n_tokens
        logw = dp.logw_cl(xs, t_x, g, 1.0, e_w).unsqueeze(1)
    else:
        logw = dp.logw_cl(xs, t_x, g).unsqueeze(1)
        l_length = torch.sum((logw - logw_) ** 2, [1, 2]) / n_tokens
    return l_length, logw


# ---------------------------------------------------------------------------------------------------------------------------
# Audio front-end (mel_processing.py, csrc/spec.hip) in front of voice conversion and forced alignment
# ---------------------------------------------------------------------------------------------------------------------------
from .mel_processing import mel_spectrogram_torch, spec_to_mel_torch, spectrogram_torch  # noqa: E402  (re-exported)


def _spec_from_audio(net_g, wav, wav_lengths, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin, fmax, mel_basis):
    """What net_g.enc_q reads, from waveforms: the linear spectrogram when enc_q.in_channels is n_fft / 2 + 1, the log-mel when it is
    n_mels (the reference's use_mel_posterior_encoder, the ModelConfig default) -> (y [B, in_channels, T], y_lengths [B])."""
    enc_q = getattr(net_g, "enc_q", None)
    if not isinstance(enc_q, PosteriorEncoder):
        raise TypeError(f"net_g.enc_q is {type(enc_q).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    if n_mels is None and mel_basis is not None:
        n_mels = int(mel_basis.shape[0])
    if enc_q.in_channels == n_fft // 2 + 1:
        return spectrogram_torch(wav, n_fft, sampling_rate, hop_size, win_size, lengths=wav_lengths)
    if n_mels is not None and enc_q.in_channels == n_mels:
        return mel_spectrogram_torch(wav, n_fft, n_mels, sampling_rate, hop_size, win_size, fmin, fmax, mel_basis=mel_basis, lengths=wav_lengths)
    raise ValueError(f"net_g.enc_q reads {enc_q.in_channels} channels: neither the linear spectrogram's n_fft / 2 + 1 = {n_fft // 2 + 1} nor "
                     f"n_mels = {n_mels}")


def voice_conversion_from_audio(net_g, wav, wav_lengths, sid_src, sid_tgt, *, n_fft, hop_size, win_size, sampling_rate, n_mels=None, fmin=0.0,
                                fmax=None, mel_basis=None, noise=None):
    """``voice_conversion`` from waveforms: wav [B, samples] fp32, wav_lengths [B] samples -> what voice_conversion returns for the
    spectrogram the reference's data loader would have made of each utterance (mel_processing.py); no host round trip between."""
    y, y_lengths = _spec_from_audio(net_g, wav, wav_lengths, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin, fmax, mel_basis)
    return voice_conversion(net_g, y, y_lengths, sid_src, sid_tgt, noise=noise)


def forced_alignment_from_audio(net_g, x, x_lengths, wav, wav_lengths, sid=None, *, n_fft, hop_size, win_size, sampling_rate, n_mels=None,
                                fmin=0.0, fmax=None, mel_basis=None, mas_noise_scale=None, noise=None):
    """``forced_alignment`` from waveforms (see voice_conversion_from_audio)."""
    y, y_lengths = _spec_from_audio(net_g, wav, wav_lengths, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin, fmax, mel_basis)
    return forced_alignment(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale=mas_noise_scale, noise=noise)


def duration_loss_from_audio(net_g, x, x_lengths, wav, wav_lengths, sid=None, *, n_fft, hop_size, win_size, sampling_rate, n_mels=None,
                             fmin=0.0, fmax=None, mel_basis=None, mas_noise_scale=None, noise=None):
    """``duration_loss`` from waveforms (see voice_conversion_from_audio)."""
    y, y_lengths = _spec_from_audio(net_g, wav, wav_lengths, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin, fmax, mel_basis)
    return duration_loss(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale=mas_noise_scale, noise=noise)


# ---------------------------------------------------------------------------------------------------------------------------
# The validation step (SynthesizerTrn.forward as a whole, models.py:1214-1286, and the forward half of train.py:341-425): the prior
# expanded along the alignment, kl_loss, slice_segments and the mel L1 through ttsvits_kl_loss / ttsvits_slice_segments /
# ttsvits_sliced_l1 (csrc/evalstep.hip)
# ---------------------------------------------------------------------------------------------------------------------------
_WEIGHTLESS = nn.Module()  # inference_only's rules for the functions that hold no parameters


def _fp32_operands(owner: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{owner}: {name} must be a tensor, got {type(t).__name__}")
        inference_only(_WEIGHTLESS, owner, t, fp32=True)


def _prefix_lengths(mask: torch.Tensor, B: int, T: int, owner: str) -> torch.Tensor:
    """t [B] int32 of a [B, 1, T] mask of ones up to each utterance's length and zeros from there; ValueError for any other mask (the
    kernels take lengths).  One host read."""
    if mask.dim() != 3 or tuple(mask.shape) != (B, 1, T):
        raise ValueError(f"{owner}: the mask must be [B, 1, T] = [{B}, 1, {T}], got {tuple(mask.shape)}")
    m = mask[:, 0, :]
    t = (m != 0).sum(1)
    prefix = (torch.arange(T, device=mask.device)[None, :] < t[:, None]).to(m.dtype)
    if not bool(torch.equal(m, prefix)):
        raise ValueError(f"{owner}: the mask is not a prefix mask (ones up to each utterance's length, zeros from there)")
    return t.to(torch.int32).contiguous()


def kl_loss(z_p, logs_q, m_p, logs_p, z_mask):
    """losses.kl_loss (losses.py:37-46): z_p, logs_q, m_p, logs_p [B, C, T] fp32 on a ROCm device, z_mask [B, 1, T] a prefix mask ->
    sum((logs_p - logs_q - 0.5 + 0.5 (z_p - m_p)^2 exp(-2 logs_p)) * z_mask) / sum(z_mask), a 0-dim tensor, in one pass of
    ttsvits_kl_loss.  C a multiple of 4.  The one host read checks the mask."""
    _fp32_operands("kl_loss", z_p=z_p, logs_q=logs_q, m_p=m_p, logs_p=logs_p, z_mask=z_mask)
    if z_p.dim() != 3 or not (z_p.shape == logs_q.shape == m_p.shape == logs_p.shape) or z_p.shape[1] % 4:
        raise ValueError(f"z_p, logs_q, m_p and logs_p must be [B, C, T] of one shape with C a multiple of 4, got {tuple(z_p.shape)}, "
                         f"{tuple(logs_q.shape)}, {tuple(m_p.shape)}, {tuple(logs_p.shape)}")
    B, _, T = z_p.shape
    t_y = _prefix_lengths(z_mask, B, T, "kl_loss")
    cl = _DurationBase._channel_last
    kl, _, _, _ = _align_engine(z_p.device).kl_loss(cl(z_p.detach()), cl(logs_q.detach()), cl(m_p.detach()), cl(logs_p.detach()), None, t_y)
    return kl[1]


def _check_slice(x, segment_size: int, owner: str) -> None:
    _fp32_operands(owner, x=x)
    if x.dim() != 3:
        raise ValueError(f"{owner}: x must be [B, C, T], got {tuple(x.shape)}")
    if not 1 <= int(segment_size) <= x.shape[2]:
        raise ValueError(f"{owner}: segment_size = {segment_size} outside [1, T] = [1, {x.shape[2]}]")


def _ids_on(ids, B: int, device, owner: str) -> torch.Tensor:
    ids = torch.as_tensor(ids).to(device)
    if tuple(ids.shape) != (B,) or ids.dtype.is_floating_point:
        raise ValueError(f"{owner}: ids_str must be [B] = [{B}] integers, got {tuple(ids.shape)} {ids.dtype}")
    return (ids if ids.dtype in (torch.int64, torch.int32) else ids.to(torch.int64)).contiguous()


def slice_segments(x, ids_str, segment_size=4):
    """commons.slice_segments (commons.py:50-56): x [B, C, T] fp32 on a ROCm device, ids_str [B] integers -> x[b, :, ids_str[b] :
    ids_str[b] + segment_size] as [B, C, segment_size], in one launch of ttsvits_slice_segments.  A start below 0 or beyond
    T - segment_size, where the reference raises a shape error, is a ValueError here: the one host read is that status word."""
    _check_slice(x, segment_size, "slice_segments")
    B, Cc, T = x.shape
    ids = _ids_on(ids_str, B, x.device, "slice_segments")
    out, status = _align_engine(x.device).slice_segments(x.detach().contiguous(), ids, Cc, T, 1, int(segment_size))
    if int(status.item()):
        raise ValueError(f"slice_segments: a start in ids_str lies outside [0, T - segment_size] = [0, {T - int(segment_size)}]")
    return out.view(B, Cc, int(segment_size))


def rand_slice_segments(x, x_lengths=None, segment_size=4, *, u=None):
    """commons.rand_slice_segments (commons.py:59-66) -> (slices [B, C, segment_size], ids_str [B] int64): ids_str = (u * (x_lengths -
    segment_size + 1)).long() with u = torch.rand([B]), the reference's draw; ``u`` (keyword, test hook) replaces it.  An utterance
    shorter than segment_size - 1 can draw a negative start: ValueError (see slice_segments)."""
    _check_slice(x, segment_size, "rand_slice_segments")
    B, _, T = x.shape
    ids_str = _draw_ids(B, T if x_lengths is None else x_lengths, int(segment_size), x.device, u)
    return slice_segments(x, ids_str, segment_size), ids_str


def _draw_ids(B: int, lengths, seg: int, device, u=None) -> torch.Tensor:
    """commons.py:63-64: the start of every utterance's segment, [B] int64 on the device."""
    if u is None:
        u = torch.rand([B])
    u = torch.as_tensor(u, dtype=torch.float32).to(device)
    if tuple(u.shape) != (B,):
        raise ValueError(f"u must be [B] = [{B}], got {tuple(u.shape)}")
    ids_str_max = (lengths.to(device) if isinstance(lengths, torch.Tensor) else lengths) - seg + 1
    return (u * ids_str_max).to(dtype=torch.long)


def _synthesizer_parts(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, ids_slice, expand, caller, wav_limit=None):
    """SynthesizerTrn.forward on the drop-ins, channel-last from the encoders to the generator -> (the alignment's namespace with
    l_length, logw, ids_slice, o [B, 1, seg * hop], kl [2] / m_exp / logs_exp of ttsvits_kl_loss added).  expand: write the
    expanded prior.  wav_limit: (samples of the waveform tensor, hop, samples of a segment) - the waveform's slice is checked
    with the latent's.  The start of every slice is checked on the device and read with the alignment's status word."""
    if noise is not None and not (isinstance(noise, (tuple, list)) and len(noise) == 3):
        raise ValueError("noise must be a triple: (forced_alignment's noise, the likelihood's draw [B, 2, T_x] or None, the reverse pass's "
                         "draw [B, 2, T_x] or None)")
    e_fa, e_q, e_w = noise if noise is not None else (None, None, None)
    for name, cls in {"dp": (StochasticDurationPredictor, DurationPredictor), "dec": Generator}.items():  # (before any device work)
        if not isinstance(getattr(net_g, name, None), cls):
            raise TypeError(f"net_g.{name} is {type(getattr(net_g, name, None)).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - "
                            "there is no fallback")
    if not x.is_cuda or not y.is_cuda:
        raise NotImplementedError(f"{caller} runs on a ROCm device only: move the model, the ids and the spectrogram there")
    seg = int(net_g.segment_size)
    B, _, T_y = y.shape
    if not 1 <= seg <= T_y:
        raise ValueError(f"{caller}: net_g.segment_size = {seg} frames outside [1, T_y] = [1, {T_y}]")
    dev = y.device
    ids = _draw_ids(B, y_lengths, seg, dev) if ids_slice is None else _ids_on(ids_slice, B, dev, caller).to(torch.int64)
    bad = (ids < 0) | (ids > T_y - seg)
    if wav_limit is not None:
        n_wav, hop, seg_wav = wav_limit
        bad = bad | (ids * hop > n_wav - seg_wav)
    also = (bad.any().to(torch.int32).reshape(1),
            f"{caller}: a segment starts outside its tensor (start < 0 - an utterance shorter than the segment - or start + segment beyond "
            "the frames or the samples)")
    p = _alignment_parts(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, e_fa,
                         {"dp": (StochasticDurationPredictor, DurationPredictor), "dec": Generator}, caller, also)
    p.l_length, p.logw = _duration_terms(net_g.dp, p.xs, p.t_x, p.x_mask, p.w, p.logw_, p.g, e_q, e_w)
    p.kl, _, p.m_exp, p.logs_exp = p.eng.kl_loss(p.zp_cl, p.logsq_cl, p.m_cl, p.logs_cl, p.ft, p.t_y, expand)
    Cc = p.z_cl.shape[2]
    z_slice, _ = p.eng.slice_segments(p.z_cl, ids, 1, T_y, Cc, seg)
    p.o = net_g.dec.forward_cl(z_slice.view(B, seg, Cc), p.g).unsqueeze(1)
    p.ids_slice = ids
    p.y_mask = (torch.arange(T_y, device=dev)[None, :] < p.t_y[:, None]).unsqueeze(1).to(torch.float32)
    return p


def synthesizer_forward(net_g, x, x_lengths, y, y_lengths, sid=None, *, mas_noise_scale=None, noise=None, ids_slice=None):
    """SynthesizerTrn.forward (models.py:1214-1286) in eval mode for a model whose enc_p / enc_q / flow / dp / dec are this module's
    drop-ins: x [B, T_x] ids, y [B, spec, T_y] -> the reference's eight results (o [B, 1, segment_size * hop], l_length [B], attn
    [B, 1, T_y, T_x], ids_slice [B] int64, x_mask, y_mask, (z, z_p, m_p, logs_p, m_q, logs_q) [B, inter, T_y] with the prior
    expanded along the alignment, (x [B, H, T_x], logw, logw_ [B, 1, T_x])).  ``net_g.segment_size`` is in frames.  Channel-last
    from the encoders to the generator; the prior is gathered through the search's frame_token (ttsvits_kl_loss), the latent's
    segment is one launch (ttsvits_slice_segments).  The one host read is the alignment's status word, which also carries the
    check of the segment starts (ValueError).  ``noise`` (test hook): duration_loss's triple; ``ids_slice`` (test hook)
    replaces the draw (torch.rand([B]) * (y_lengths - segment_size + 1)).long()."""
    p = _synthesizer_parts(net_g, x, x_lengths, y, y_lengths, sid, mas_noise_scale, noise, ids_slice, True, "vits2.synthesizer_forward")
    tr = lambda t: t.transpose(1, 2)  # noqa: E731
    return (p.o, p.l_length, p.attn, p.ids_slice, p.x_mask, p.y_mask,
            (tr(p.z_cl), tr(p.zp_cl), tr(p.m_exp), tr(p.logs_exp), tr(p.mq_cl), tr(p.logsq_cl)), (tr(p.xs), p.logw, p.logw_))


def validation_losses(net_g, net_d, x, x_lengths, spec, spec_lengths, wav, *, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin=0.0,
                      fmax=None, mel_basis=None, segment_size, c_mel=10.0, c_kl=0.2, net_dur_disc=None, sid=None, mas_noise_scale=None,
                      noise=None, ids_slice=None):
    """The loss terms of one batch, train.py:341-425 forward only, in eval mode and without gradients: x [B, T_x] ids, spec
    [B, spec, T_y] what net_g.enc_q reads, wav [B, 1, N] -> a dict of 0-dim device tensors ``loss_disc``, ``loss_gen``, ``loss_fm``,
    ``loss_mel`` (x c_mel), ``loss_dur``, ``loss_kl`` (x c_kl), ``loss_gen_all`` = loss_gen + loss_fm + loss_mel + loss_dur +
    loss_kl (+ loss_dur_gen), with ``net_dur_disc`` also ``loss_dur_disc`` and ``loss_dur_gen``, and ``ids_slice`` [B].
    ``segment_size`` is in samples and must be net_g.segment_size * hop_size; c_mel / c_kl default to the reference's ModelConfig
    (cli.py: 10.0, 0.2).  mel is spec when net_g.enc_q reads n_mels channels, else spec_to_mel_torch(spec); loss_mel is the L1 of
    its segment against mel_spectrogram_torch(o) without the segment in memory (ttsvits_sliced_l1); loss_kl comes from the
    unexpanded prior and the search's frame_token (ttsvits_kl_loss); the waveform's segment is one launch.  The one host read is
    the alignment's status word.  ``noise`` / ``ids_slice``: see synthesizer_forward."""
    if not isinstance(net_d, MultiPeriodDiscriminator):
        raise TypeError(f"net_d is {type(net_d).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    if net_dur_disc is not None and not isinstance(net_dur_disc, _DurationDiscriminatorBase):
        raise TypeError(f"net_dur_disc is {type(net_dur_disc).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    enc_q = getattr(net_g, "enc_q", None)
    if not isinstance(enc_q, PosteriorEncoder):
        raise TypeError(f"net_g.enc_q is {type(enc_q).__name__}, not the HIP drop-in: swap it in (INTEGRATION.md) - there is no fallback")
    _fp32_operands("vits2.validation_losses", spec=spec, wav=wav)
    if wav.dim() != 3 or wav.shape[1] != 1 or wav.shape[0] != spec.shape[0]:
        raise ValueError(f"wav must be [B, 1, N] = [{spec.shape[0]}, 1, N], got {tuple(wav.shape)}")
    seg_frames = int(getattr(net_g, "segment_size", 0))
    if int(segment_size) != seg_frames * int(hop_size):
        raise ValueError(f"segment_size = {segment_size} samples is not net_g.segment_size * hop_size = {seg_frames} * {hop_size}")
    B, _, N = wav.shape
    if not 1 <= int(segment_size) <= N:
        raise ValueError(f"segment_size = {segment_size} samples outside [1, N] = [1, {N}]")
    mel = spec if enc_q.in_channels == n_mels else spec_to_mel_torch(spec, n_fft, n_mels, sampling_rate, fmin, fmax, mel_basis=mel_basis)
    p = _synthesizer_parts(net_g, x, x_lengths, spec, spec_lengths, sid, mas_noise_scale, noise, ids_slice, False, "vits2.validation_losses",
                           (N, int(hop_size), int(segment_size)))
    y_hat_mel = mel_spectrogram_torch(p.o.squeeze(1), n_fft, n_mels, sampling_rate, hop_size, win_size, fmin, fmax, mel_basis=mel_basis)
    if y_hat_mel.shape[2] != seg_frames:
        raise ValueError(f"the mel of a generated segment has {y_hat_mel.shape[2]} frames, the segment {seg_frames}: n_fft, hop_size and "
                         "segment_size do not fit (the reference's F.l1_loss fails there too)")
    l1, _, _ = p.eng.sliced_l1(mel.detach().contiguous(), y_hat_mel.contiguous(), p.ids_slice)
    y, _ = p.eng.slice_segments(wav.detach().contiguous(), p.ids_slice, 1, N, 1, int(segment_size), int(hop_size))
    y_d_hat_r, y_d_hat_g, fmap_r, fmap_g = net_d(y.view(B, 1, int(segment_size)), p.o)
    r_losses, g_losses = discriminator_loss(y_d_hat_r, y_d_hat_g)
    out = {"loss_disc": r_losses.sum() + g_losses.sum(), "loss_gen": generator_loss(y_d_hat_g).sum(), "loss_fm": feature_loss(fmap_r, fmap_g),
           "loss_mel": l1[1] * c_mel, "loss_dur": torch.sum(p.l_length.float()), "loss_kl": p.kl[1] * c_kl}
    out["loss_gen_all"] = out["loss_gen"] + out["loss_fm"] + out["loss_mel"] + out["loss_dur"] + out["loss_kl"]
    if net_dur_disc is not None:
        as_list = lambda v: [v] if isinstance(v, torch.Tensor) else v  # noqa: E731  (V1 returns tensors, V2 lists: train.py wraps them)
        y_dur_hat_r, y_dur_hat_g = net_dur_disc(p.xs.transpose(1, 2), p.x_mask, p.logw_, p.logw)
        dr, dg = discriminator_loss(as_list(y_dur_hat_r), as_list(y_dur_hat_g))
        out["loss_dur_disc"] = dr.sum() + dg.sum()
        out["loss_dur_gen"] = generator_loss(as_list(y_dur_hat_g)).sum()
        out["loss_gen_all"] = out["loss_gen_all"] + out["loss_dur_gen"]
    out["ids_slice"] = p.ids_slice
    return out


def validation_losses_from_audio(net_g, net_d, x, x_lengths, wav, wav_lengths, *, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin=0.0,
                                 fmax=None, mel_basis=None, segment_size, **kwargs):
    """``validation_losses`` with the spectrogram made from wav [B, 1, N] (or [B, N]) and wav_lengths [B] samples, as the
    reference's data loader would have (see voice_conversion_from_audio); the keywords are validation_losses'."""
    wav2 = wav[:, 0] if wav.dim() == 3 else wav
    spec, spec_lengths = _spec_from_audio(net_g, wav2, wav_lengths, n_fft, hop_size, win_size, sampling_rate, n_mels, fmin, fmax, mel_basis)
    return validation_losses(net_g, net_d, x, x_lengths, spec, spec_lengths, wav2.unsqueeze(1), n_fft=n_fft, hop_size=hop_size, win_size=win_size,
                             sampling_rate=sampling_rate, n_mels=n_mels, fmin=fmin, fmax=fmax, mel_basis=mel_basis, segment_size=segment_size,
                             **kwargs)
