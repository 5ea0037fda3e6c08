"""Host-side owner of one ttsdec handle: packs an nn.Module's parameters into the
kernel blob, holds workspaces (PyTorch caching allocator memory) and issues the
C-ABI calls on torch's current HIP stream."""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

Tensor = torch.Tensor


@dataclass(frozen=True)
class EngineDims:
    d_mel: int = 80
    r: int = 1
    d_pre: int = 256
    d_ctx: int = 512
    h_att: int = 1024
    h_dec: int = 1024
    p_zoneout: float = 0.1
    p_dropout: float = 0.5
    postnet_layers: int = 0
    postnet_hidden: int = 512
    postnet_kernel: int = 5
    bn_eps: float = 1e-5
    cell_type: int = 0      # _lib.CELL_*
    d_pre_hidden: int = 0   # 0 = d_pre
    postnet_type: int = 0   # _lib.POSTNET_TYPE_*

    def to_c(self) -> _lib.Dims:
        return _lib.Dims(
            self.d_mel, self.r, self.d_pre, self.d_ctx, self.h_att, self.h_dec, self.p_zoneout, self.p_dropout,
            self.postnet_layers, self.postnet_hidden, self.postnet_kernel, self.bn_eps,
            self.cell_type, self.d_pre_hidden, self.postnet_type,
        )

    @property
    def pre_hidden(self) -> int:
        return self.d_pre_hidden or self.d_pre

    @property
    def cell_output(self) -> int:
        return self.h_att + self.h_dec + self.d_ctx if self.cell_type == _lib.CELL_TACO2 else self.h_dec + self.d_ctx


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_device(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} must live on a ROCm device (got {t.device}): this package runs the decoder hot path "
            "only through its HIP kernels and has no CPU fallback"
        )


STREAM = object()  # in Handle.call's arguments: the current stream of the handle's device


class WS:
    """In Handle.call's arguments: a workspace tensor, passed as its (pointer, bytes) pair; None: (NULL, 0)."""

    __slots__ = ("t",)

    def __init__(self, t: Optional[Tensor]):
        self.t = t


_EPOCH = [0]


def invalidate_packed_weights() -> None:
    """Forces every engine to repack its weight blob on next use.  Needed after edits that autograd's
    version counter does not see: ``param.data.copy_(...)`` / ``param.data.mul_(...)`` leave
    ``param._version`` unchanged (the reference's checkpoint loader does exactly that,
    tacotron/train_util.py:43; so do EMA swaps).  ``load_state_dict`` calls this by itself (hook)."""
    _EPOCH[0] += 1


def _invalidate_hook(module, incompatible_keys) -> None:  # module-level: stays picklable
    invalidate_packed_weights()


class PackedWeightsMixin:
    """For the nn.Modules whose parameters are mirrored in a packed device blob."""

    def invalidate(self) -> None:
        """Call after modifying parameters through ``.data`` (see invalidate_packed_weights)."""
        invalidate_packed_weights()

    def _watch_state_dict_loads(self) -> None:
        self.register_load_state_dict_post_hook(_invalidate_hook)


def weights_fingerprint(tensors: Sequence[Optional[Tensor]]) -> Tuple:
    """Key of a packed blob: changes when a parameter is replaced, moved, or modified in place through
    autograd-visible ops (``_version``), and when invalidate_packed_weights() was called.  In-place edits
    through ``.data`` are NOT visible here - call ``module.invalidate()`` after them."""
    return (_EPOCH[0],) + tuple((None if t is None else (t.data_ptr(), t._version, tuple(t.shape))) for t in tensors)


class Handle:
    """One handle of a C-ABI family (include/ttsdec.h ``<prefix>_*``) bound to one device: create / close, the family's own
    HIP error text, weight packing and grow-only workspaces.  Subclasses add the family's compute calls.  Not thread-safe
    (the C ABI asks the caller to serialise calls per handle)."""

    PREFIX = ""  # the family: "ttsdec", "ttsenc", ...

    def __init__(self, dims, c_dims, device: Optional[torch.device]):
        """dims: the family's dims as the module holds them, c_dims: the same as the C struct; device None: a handle for
        host-only queries (sizes, counts), which work without a GPU."""
        self.dims = dims
        self.device = device
        self._lib = _lib.load()
        h = C.c_void_p()
        create = self._fn("create")
        if device is not None:
            with torch.cuda.device(device):  # the handle binds to the device current at create
                rc = create(C.byref(c_dims), C.byref(h))
        else:
            rc = create(C.byref(c_dims), C.byref(h))
        if rc == _lib.ERR_DIMS:
            raise _lib.DimsNotBuilt(rc, f"{self.PREFIX}_create", f"not built in the HIP library (include/ttsdec.h {self.PREFIX}_dims): {dims}")
        _lib.check(rc, f"{self.PREFIX}_create")
        self._h = h
        self.blob: Optional[Tensor] = None
        self._fingerprint = None
        self._ws: Optional[Dict[str, Tensor]] = None  # kind -> workspace; None: none held

    def _fn(self, name: str):
        return getattr(self._lib, f"{self.PREFIX}_{name}")

    def _err(self, rc: int, what: str) -> None:
        if rc != _lib.OK:
            raise _lib.TtsdecError(rc, what, self._fn("last_hip_error")(self._h).decode() if rc == _lib.ERR_HIP else "")

    def call(self, name: str, *args, dims: Optional[str] = None) -> None:
        """The C function ``name`` (its full name: engines call across prefixes) on this handle, under the handle's device.  args:
        what include/ttsdec.h declares after the handle, in that order - a tensor stands for its data pointer, WS(t) for a
        workspace's pointer and byte count, STREAM for the device's current stream; None, numbers and ctypes objects pass as they
        are.  Raises for a code other than OK; dims: the message of the DimsNotBuilt that ERR_DIMS becomes."""
        with torch.cuda.device(self.device) if self.device is not None else contextlib.nullcontext():
            flat = [self._h]
            for a in args:
                if isinstance(a, Tensor):
                    flat.append(a.data_ptr())
                elif isinstance(a, WS):
                    flat += (None, 0) if a.t is None else (a.t.data_ptr(), a.t.numel())
                else:
                    flat.append(_stream(self.device) if a is STREAM else a)
            rc = getattr(self._lib, name)(*flat)
        if rc == _lib.ERR_DIMS and dims is not None:
            raise _lib.DimsNotBuilt(rc, name, dims)
        self._err(rc, name)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- host-only queries (work without a GPU) ----
    def num_weight_tensors(self) -> int:
        return int(self._fn("num_weight_tensors")(self._h))

    def packed_bytes(self) -> int:
        return int(self._fn("packed_bytes")(self._h))

    # ---- arithmetic of the GEMMs (the families that have the switch) ----
    def set_precision(self, mode: str) -> None:
        """"f32" (exact fp32 matrix instruction, default) or "split_f16" (hi/lo fp16 planes, 3 products)."""
        code = {"f32": _lib.PREC_F32, "split_f16": _lib.PREC_SPLIT_F16}[mode]
        self.call(f"{self.PREFIX}_set_precision", code)

    def precision(self) -> str:
        return {_lib.PREC_F32: "f32", _lib.PREC_SPLIT_F16: "split_f16"}[int(self._fn("get_precision")(self._h))]

    # ---- weights ----
    def pack(self, tensors: Sequence[Optional[Tensor]]) -> Tensor:
        """tensors: in the family's pack order; None = not owned by the calling module (the library leaves that region zero
        where the family allows it - ttsdec_, ttsvits_ - and refuses it elsewhere)."""
        n = self.num_weight_tensors()
        if len(tensors) != n:
            raise ValueError(f"expected {n} weight tensors, got {len(tensors)}")
        keep: List[Tensor] = []
        arr = (C.c_void_p * n)()
        for i, t in enumerate(tensors):
            if t is None:
                continue
            _require_device(t, "weights")
            tc = t.detach().to(torch.float32).contiguous()
            keep.append(tc)
            arr[i] = tc.data_ptr()
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=self.device)
        self.call(f"{self.PREFIX}_pack_weights", arr, n, blob, STREAM)
        torch.cuda.current_stream(self.device).synchronize()  # `keep` must outlive the packing kernels
        self.blob, self._fingerprint = blob, weights_fingerprint(tensors)
        return blob

    def ensure_packed(self, tensors, key_tensors: Optional[Sequence[Optional[Tensor]]] = None) -> None:
        """Packs unless the blob is current.  tensors: pack's list, or a callable producing it (called only when a repack is
        needed); key_tensors: the parameters whose identity / version decide that (default: the list itself - derived tensors
        such as weight-normed weights are new objects on every call and must not be the key)."""
        fp = weights_fingerprint(key_tensors if key_tensors is not None else tensors)
        if self.blob is not None and fp == self._fingerprint:
            return
        self.pack(tensors() if callable(tensors) else tensors)
        self._fingerprint = fp

    # ---- workspaces (caching-allocator memory, one grow-only buffer per kind) ----
    def workspace(self, kind: str, nbytes: int) -> Tensor:
        if self._ws is None:
            self._ws = {}
        ws = self._ws.get(kind)
        if ws is None or ws.numel() < nbytes:
            self._ws.pop(kind, None)  # (the old buffer goes back to the allocator first)
            ws = self._ws[kind] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def sized_workspace(self, kind: str, fn: str, *args, refusal: Optional[Exception] = None) -> Tensor:
        """The workspace of ``kind``, at least as large as the library's size query ``fn`` (full name; args: after the handle)
        reports.  refusal: what to raise where the query answers 0, its way of refusing the sizes."""
        nbytes = int(getattr(self._lib, fn)(self._h, *args))
        if not nbytes and refusal is not None:
            raise refusal
        return self.workspace(kind, nbytes)

    def release_workspaces(self) -> None:
        """Drops every workspace (the next call allocates afresh); assigning None to ``_ws`` does the same."""
        self._ws = None


def _raise_frame_flags(flags: int, T: int) -> None:
    """The status word of ttsdec_mel_to_magnitude / ttsdec_griffinlim (include/ttsdec.h)."""
    if flags & 4:
        raise ValueError(f"an utterance's length exceeds the tensor's {T} frames")
    if flags & 1:
        raise ValueError("an utterance has fewer than 2 frames: it has no samples (hop_length * (frames - 1))")


class Engine(Handle):
    """One ttsdec handle bound to one device."""

    PREFIX = "ttsdec"

    def __init__(self, dims: EngineDims, device: Optional[torch.device]):
        super().__init__(dims, dims.to_c(), device)
        # exact-shape workspaces of the decode steps and the postnet, keyed by (B, L) / (B, T) (a captured graph holds the pointer)
        self._step_ws: Dict[Tuple[int, int], Tensor] = {}
        self._pws: Dict[Tuple[int, int], Tensor] = {}

    def workspace_bytes(self, B: int, L: int) -> int:
        return self._lib.ttsdec_workspace_bytes(self._h, B, L)

    def postnet_workspace_bytes(self, B: int, T: int) -> int:
        return self._lib.ttsdec_postnet_workspace_bytes(self._h, B, T)

    # ---- tuning / measurement options (include/ttsdec.h TTSDEC_OPT_*; -1 = library default) ----
    def set_option(self, name: str, value: int) -> None:
        _lib.check(self._lib.ttsdec_set_option(self._h, _lib.option_ids()[name], int(value)), f"ttsdec_set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        _lib.check(self._lib.ttsdec_get_option(self._h, _lib.option_ids()[name], C.byref(v)), f"ttsdec_get_option({name})")
        return int(v.value)

    # ---- weights ----
    def bind(self, blob: Tensor) -> None:
        """Adopt a packed blob produced elsewhere (e.g. broadcast from rank 0)."""
        _require_device(blob, "blob")
        if blob.numel() * blob.element_size() != self.packed_bytes():
            raise ValueError("blob size does not match this engine's dims")
        with torch.cuda.device(self.device):
            torch.cuda.current_stream(self.device).synchronize()  # the blob must be complete: its header is read back
        self.call("ttsdec_bind_weights", blob)
        self.blob = blob
        self._fingerprint = None

    # ---- mel -> waveform (weightless: a handle of any dims serves, bound or not; audio.py holds the entry points) ----
    def mel_to_magnitude(self, y: Tensor, P: Tensor, frames: Optional[Tensor], n_fft: int, *, check: bool = False) -> Tensor:
        """y [B, T, n_mels], P [n_fft / 2 + 1, n_mels] contiguous fp32, frames [B] int32 (device) or None -> mag [B, bins, T]
        (ttsdec_mel_to_magnitude).  check: read the status word back (one host sync) and raise for a refused utterance."""
        B, T, n_mels = y.shape
        mag = torch.empty(B, n_fft // 2 + 1, T, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device) if check else None
        self.call("ttsdec_mel_to_magnitude", y, P, frames, B, T, n_mels, n_fft, mag, status, STREAM)
        if check:
            _raise_frame_flags(int(status.item()), T)
        return mag

    def griffinlim(self, mag: Tensor, frames: Optional[Tensor], window: Tensor, n_fft: int, hop_length: int, angles: Optional[Tensor],
                   tprev: Optional[Tensor], n_iter: int, momentum: float, normalize: bool, return_state: bool, *, check: bool = False):
        """mag [B, n_fft / 2 + 1, T] contiguous fp32, angles / tprev [B, bins, T] contiguous complex64 or None -> wave
        [B, hop_length * (T - 1)], and with return_state (n_iter >= 1) the last rebuilt spectrum and the final phase factors
        (ttsdec_griffinlim)."""
        B, bins, T = mag.shape
        ws = self.sized_workspace("griffinlim", "ttsdec_griffinlim_workspace_bytes", B, T, n_fft, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsdec_griffinlim", f"B = {B}, T = {T}, n_fft = {n_fft}: built for n_fft 256 / 512 / 1024 / 2048, T >= 2, B <= 65535"))
        wave = torch.empty(B, hop_length * (T - 1), device=self.device)
        state = [torch.empty(B, bins, T, dtype=torch.complex64, device=self.device) for _ in range(2)] if return_state else [None, None]
        status = torch.empty(1, dtype=torch.int32, device=self.device) if check else None
        self.call("ttsdec_griffinlim", mag, frames, B, T, window, n_fft, hop_length, angles, tprev, n_iter, momentum, int(normalize), wave,
                  state[0], state[1], status, WS(ws), STREAM, dims=f"n_fft = {n_fft}, hop_length = {hop_length}: needs hop_length <= n_fft / 2")
        if check:
            _raise_frame_flags(int(status.item()), T)
        return (wave, state[0], state[1]) if return_state else wave

    # ---- waveform -> dB spectrogram and mel (weightless; audio.py holds the entry point) ----
    def mel_analysis(self, wave: Tensor, lengths: Optional[Tensor], window: Tensor, fb: Tensor, hop_length: int, spectrogram: bool):
        """wave [B, N] contiguous fp32, lengths [B] int32 (device) or None, window [n_fft], fb [n_fft / 2 + 1, n_mels] contiguous fp32
        -> (spec_db [B, T, bins] or None, mel_db [B, T, n_mels], frames [B] int32), T = 1 + N // hop_length (ttsdec_mel_analysis).
        The status word is always read back (one host sync): a silent utterance is only known on the device."""
        B, N = wave.shape
        n_fft, (bins, n_mels) = window.numel(), fb.shape
        T = 1 + N // hop_length
        ws = self.sized_workspace("mel_analysis", "ttsdec_mel_analysis_workspace_bytes", B, n_fft, n_mels, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsdec_mel_analysis", f"B = {B}, n_fft = {n_fft}, n_mels = {n_mels}: built for n_fft 256 / 512 / 1024 / 2048, "
            "n_mels <= 256, B <= 65535"))
        spec = torch.empty(B, T, bins, device=self.device) if spectrogram else None
        mel = torch.empty(B, T, n_mels, device=self.device)
        frames = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.call("ttsdec_mel_analysis", wave, lengths, B, N, window, fb, n_mels, n_fft, hop_length, T, spec, mel, frames, status, WS(ws), STREAM,
                  dims=f"n_fft = {n_fft}, hop_length = {hop_length}, {N} samples: needs 1 <= hop_length <= n_fft / 2, at most 2^30 samples and "
                  "2^22 frames")
        flags = int(status.item())
        if flags & 4:
            raise ValueError(f"an utterance's length exceeds the row's {N} samples")
        if flags & 1:
            raise ValueError(f"an utterance has no more than n_fft / 2 = {n_fft // 2} samples: it cannot be reflect-padded")
        if flags & 2:
            raise ValueError("an utterance is all zeros: it has no peak to normalise by")
        return spec, mel, frames

    # ---- sample-rate conversion (weightless; audio.py holds the entry point) ----
    def resample(self, wave: Tensor, lengths: Optional[Tensor], orig_freq: int, new_freq: int, lowpass_filter_width: int, rolloff: float,
                 n_out: int, *, check: bool = False):
        """wave [B, N] contiguous fp32, lengths [B] int32 (device) or None -> (out [B, n_out], lengths_out [B] int32)
        (ttsdec_resample).  Enqueues only; check: read the status word back (one host sync) and raise for a length beyond the row."""
        B, N = wave.shape
        ws = self.sized_workspace("resample", "ttsdec_resample_workspace_bytes", orig_freq, new_freq, lowpass_filter_width, rolloff, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsdec_resample", f"{orig_freq} -> {new_freq} Hz, lowpass_filter_width = {lowpass_filter_width}, rolloff = {rolloff}: "
            "built for reduced rates <= 1024 and <= 16384 taps"))
        out = torch.empty(B, n_out, device=self.device)
        lengths_out = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device) if check else None
        self.call("ttsdec_resample", wave, lengths, B, N, orig_freq, new_freq, lowpass_filter_width, rolloff, out, n_out, lengths_out, status,
                  WS(ws), STREAM, dims=f"B = {B}, {N} -> {n_out} samples: needs B <= 65535 and at most 2^30 samples")
        if check and int(status.item()) & 4:
            raise ValueError(f"an utterance's length exceeds the row's {N} samples")
        return out, lengths_out

    # ---- workspaces ----
    def step_workspace(self, B: int, L: int) -> Tensor:
        key = (B, L)
        ws = self._step_ws.get(key)
        if ws is None:
            self._step_ws.clear()
            ws = torch.empty(self.workspace_bytes(B, L), dtype=torch.uint8, device=self.device)
            self._step_ws[key] = ws
        return ws

    def postnet_workspace(self, B: int, T: int) -> Tensor:
        key = (B, T)
        ws = self._pws.get(key)
        if ws is None:
            self._pws.clear()
            ws = torch.empty(self.postnet_workspace_bytes(B, T), dtype=torch.uint8, device=self.device)
            self._pws[key] = ws
        return ws

    # ---- compute ----
    def decode(
        self,
        memory: Tensor,
        *,
        t_begin: int,
        n_steps: int,
        stop_threshold: float,
        check_stop: bool,
        dropout_mode: int,
        masks: Optional[Tensor],
        seed: int,
        teacher: Optional[Tensor],
        teacher_flags: Optional[Tensor],
        y: Tensor,
        s: Tensor,
        w: Tensor,
        t_out: Tensor,
    ) -> None:
        """Enqueues n_steps decode steps; outputs land in y/s/w rows [0, n_steps)."""
        _require_device(memory, "memory")
        B, L, _ = memory.shape
        t_stride = w.shape[1]
        ws = self.step_workspace(B, L)
        self.call(
            "ttsdec_decode", memory, B, L, t_begin, n_steps, t_stride,
            float(stop_threshold), int(check_stop), dropout_mode, masks, seed & 0xFFFFFFFFFFFFFFFF,
            teacher, 0 if teacher is None else teacher.shape[1], teacher_flags,
            y, s, w, t_out, WS(ws), STREAM,
        )

    def decode_each(self, memory: Tensor, *, t_begin: int, n_steps: int, stop_threshold: float, dropout_mode: int,
                    masks: Optional[Tensor], seed: int, y: Tensor, s: Tensor, w: Tensor, stop_steps: Tensor, t_out: Tensor) -> None:
        """decode under the per-utterance stop rule (ttsdec_decode_each); stop_steps: int32 [B] on the device, the same tensor
        for every chunk of one decode."""
        _require_device(memory, "memory")
        B, L, _ = memory.shape
        if stop_steps.dtype != torch.int32 or stop_steps.numel() != B or not stop_steps.is_contiguous():
            raise ValueError("stop_steps must be a contiguous int32 [B] tensor")
        _require_device(stop_steps, "stop_steps")
        ws = self.step_workspace(B, L)
        self.call(
            "ttsdec_decode_each", memory, B, L, t_begin, n_steps, w.shape[1],
            float(stop_threshold), dropout_mode, masks, seed & 0xFFFFFFFFFFFFFFFF, None, 0, None,
            y, s, w, stop_steps, t_out, WS(ws), STREAM,
        )

    def zero_tail(self, x: Tensor, lengths: Tensor, len_div: int = 1) -> None:
        """Zeroes x[b, lengths[b] // len_div :] in place (ttsdec_zero_tail).  x: fp32 [B, T] or [B, T, C] whose entries x[b] are
        contiguous (a slice along T of a contiguous tensor is fine); lengths: int32 [B] on the device."""
        _require_device(x, "x")
        B, T = x.shape[:2]
        Cc = x.shape[2] if x.dim() == 3 else 1
        if x.dtype != torch.float32 or x.dim() not in (2, 3) or not x[0].is_contiguous():
            raise ValueError("zero_tail: x must be fp32 [B, T] or [B, T, C] with contiguous entries")
        if T == 0:
            return
        self.call("ttsdec_zero_tail", x, lengths, B, T, x.stride(0) if B > 1 else T * Cc, Cc, len_div, STREAM)

    # ---- the validation step's loss terms (weightless; tacotron.py holds the entry points) ----
    def val_losses(self, y: Optional[Tensor], y_post: Optional[Tensor], x: Optional[Tensor], s: Optional[Tensor], w: Optional[Tensor],
                   lengths: Optional[Tensor], pos_weight: float = 0.1, shape: Optional[Tuple[int, int, int]] = None):
        """y / y_post [B, T, D], x [B, T_x >= T, D], s [B, T], w [B, S, L] contiguous fp32 or None, lengths [B] int32 (device) or None ->
        (rows [B, 9], terms [16]) (ttsdec_val_losses).  shape: (B, T, D) where y is None.  Enqueues only."""
        B, T, D = y.shape if y is not None else shape
        S, L = (w.shape[1], w.shape[2]) if w is not None else (0, 0)
        ws = self.sized_workspace("val_losses", "ttsdec_val_losses_workspace_bytes", B, T, S, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsdec_val_losses", f"B = {B}, T = {T}, S = {S}: needs B <= 65535 and at most 2^31 frames"))
        rows = torch.empty(B, 9, device=self.device)
        terms = torch.empty(16, device=self.device)
        self.call("ttsdec_val_losses", y, y_post, x, T if x is None else x.shape[1], s, w, lengths, B, T, D, S, L, float(pos_weight), rows, terms,
                  WS(ws), STREAM, dims=f"B = {B}, D = {D}: needs B <= 65535, D <= 1024 and tensors of at most 2^31 elements")
        return rows, terms

    def mel_loss(self, y: Tensor, x: Tensor, lengths: Optional[Tensor], order: int):
        """y [B, T, D], x [B, T_x >= T, D] contiguous fp32, lengths [B] int32 (device) or None -> (rows [B], out [1]) (ttsdec_mel_loss)."""
        B, T, D = y.shape
        ws = self.sized_workspace("val_losses", "ttsdec_val_losses_workspace_bytes", B, T, 0, refusal=_lib.DimsNotBuilt(
            _lib.ERR_DIMS, "ttsdec_mel_loss", f"B = {B}, T = {T}: needs B <= 65535 and at most 2^31 frames"))
        rows = torch.empty(B, device=self.device)
        out = torch.empty(1, device=self.device)
        self.call("ttsdec_mel_loss", y, x, x.shape[1], lengths, B, T, D, int(order), rows, out, WS(ws), STREAM,
                  dims=f"B = {B}, D = {D}: needs B <= 65535, D <= 1024 and tensors of at most 2^31 elements")
        return rows, out

    def postnet(self, y: Tensor, precision: int = _lib.POSTNET_F32, lengths: Optional[Tensor] = None) -> Tensor:
        _require_device(y, "y")
        B, T, _ = y.shape
        out = torch.empty_like(y)
        ws = self.postnet_workspace(B, T)
        if lengths is None:
            self.call("ttsdec_postnet", y, B, T, precision, out, WS(ws), STREAM)
        else:  # int32 [B] on the device, frames
            self.call("ttsdec_postnet_ragged", y, lengths, B, T, precision, out, WS(ws), STREAM)
        return out

    def cell_step(self, x, memory, w, ctx, h_att, c_att, h_dec, c_dec, dropout_mode, masks, seed, step) -> Tensor:
        _require_device(memory, "memory")
        B, L, _ = memory.shape
        x_dec = torch.empty(B, self.dims.cell_output, dtype=torch.float32, device=self.device)
        ws = self.step_workspace(B, L)
        self.call("ttsdec_cell_step", x, memory, B, L, w, ctx, h_att, c_att, h_dec, c_dec, dropout_mode, masks, seed & 0xFFFFFFFFFFFFFFFF, step,
                  x_dec, WS(ws), STREAM)
        return x_dec

    def profile_step(self, memory: Tensor, iters: int, dropout_mode: int, masks: Optional[Tensor], seed: int):
        """Mean per-kernel duration (ms) of one decode step; see ttsdec_profile_step."""
        B, L, _ = memory.shape
        d = self.dims
        y = torch.empty(B, 2 * d.r, d.d_mel, device=self.device)  # (the profiled step is step 1 of 2)
        s = torch.empty(B, 2 * d.r, device=self.device)
        w = torch.empty(B, 2, L, device=self.device)
        ws = self.step_workspace(B, L)
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        nk = C.c_int(0)
        self.call("ttsdec_profile_step", memory, B, L, iters, dropout_mode, masks, seed & 0xFFFFFFFFFFFFFFFF, y, s, w, WS(ws), STREAM,
                  ms, names, 16, C.byref(nk))
        return {names[i].decode(): float(ms[i]) for i in range(nk.value)}


    def profile_loop(self, memory: Tensor, n_steps: int, dropout_mode: int, masks: Optional[Tensor], seed: int):
        """Per-launch time (ms) INSIDE the replayed graph of the step loop and the loop's time per step; see
        ttsdec_profile_loop (n_steps: a multiple of 30, at least 60)."""
        B, L, _ = memory.shape
        d = self.dims
        y = torch.empty(B, n_steps * d.r, d.d_mel, device=self.device)
        s = torch.empty(B, n_steps * d.r, device=self.device)
        w = torch.empty(B, n_steps, L, device=self.device)
        t_out = torch.zeros(2, dtype=torch.int32, device=self.device)
        ws = self.step_workspace(B, L)
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        nk = C.c_int(0)
        step = C.c_float(0.0)
        self.call("ttsdec_profile_loop", memory, B, L, n_steps, dropout_mode, masks, seed & 0xFFFFFFFFFFFFFFFF, y, s, w, t_out, WS(ws), STREAM,
                  ms, names, 16, C.byref(nk), C.byref(step))
        return {names[i].decode(): float(ms[i]) for i in range(nk.value)}, float(step.value)


class EngineCache:
    """Per-device engines of one module, made by ``engine_cls(dims, device)`` and rebuilt when the dims change.  Lives in the
    module's __dict__ but is dropped on pickling / deepcopy, and shared (keyed by device) by the replicas nn.DataParallel
    makes (train_util.py:215 in the reference)."""

    def __init__(self, engine_cls=Engine):
        self.engine_cls = engine_cls
        self._by_dev: Dict[int, Tuple[object, Handle]] = {}  # device index -> (dims it was built for, engine)

    def get(self, dims, device: torch.device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        built = self._by_dev.get(idx)
        if built is None or built[0] != dims:
            built = self._by_dev[idx] = (copy.deepcopy(dims), self.engine_cls(dims, torch.device("cuda", idx)))
        return built[1]

    def engines(self) -> List[Handle]:
        return [e for _, e in self._by_dev.values()]

    def clear(self) -> None:
        for e in self.engines():
            e.close()
        self._by_dev.clear()

    def __getstate__(self):
        return {"engine_cls": self.engine_cls}

    def __setstate__(self, state):
        self.engine_cls, self._by_dev = state["engine_cls"], {}

    def __deepcopy__(self, memo):
        return EngineCache(self.engine_cls)
