"""ctypes binding of libttsdec.so (include/ttsdec.h).  No torch types cross this
boundary: only raw device pointers, sizes and the stream handle."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, NamedTuple, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
# (TTSDEC_LIB: another build of the same library, for same-box A/B measurements of two source states - tools/ only)
LIB_PATH = os.environ.get("TTSDEC_LIB") or os.path.join(HERE, "lib", "libttsdec.so")

# error codes / enums (mirrors include/ttsdec.h)
OK = 0
ERR_INVALID_ARG, ERR_DIMS, ERR_HIP, ERR_NOT_BOUND, ERR_WORKSPACE, ERR_DEVICE = -1, -2, -3, -4, -5, -6
DROPOUT_OFF, DROPOUT_MASKS, DROPOUT_PHILOX = 0, 1, 2
POSTNET_F32, POSTNET_BF16, POSTNET_SPLIT_F16 = 0, 1, 2
PREC_F32, PREC_SPLIT_F16 = 0, 1
ABI_VERSION = 2  # include/ttsdec.h TTSDEC_VERSION these bindings were written for
CELL_TACO2PROD, CELL_TACO2 = 0, 1
POSTNET_TYPE_MEL, POSTNET_TYPE_MEL2 = 0, 1
W_DECODER_COUNT = 21
W_POSTNET_PER_LAYER = 5
W_POSTNET2_PER_LAYER = 11


def option_ids():
    """name -> TTSDEC_OPT_* of the tuning / measurement options (include/ttsdec.h), as the library itself names them."""
    lib, out, i = load(), {}, 0
    while True:
        n = lib.ttsdec_option_name(i)
        if n is None:
            return out
        out[n.decode()] = i
        i += 1

ENC_W_COUNT = 20


class Dims(C.Structure):
    _fields_ = [
        ("d_mel", C.c_int32),
        ("r", C.c_int32),
        ("d_pre", C.c_int32),
        ("d_ctx", C.c_int32),
        ("h_att", C.c_int32),
        ("h_dec", C.c_int32),
        ("p_zoneout", C.c_float),
        ("p_dropout", C.c_float),
        ("postnet_layers", C.c_int32),
        ("postnet_hidden", C.c_int32),
        ("postnet_kernel", C.c_int32),
        ("bn_eps", C.c_float),
        ("cell_type", C.c_int32),
        ("d_pre_hidden", C.c_int32),
        ("postnet_type", C.c_int32),
    ]


class EncDims(C.Structure):
    _fields_ = [
        ("alphabet_size", C.c_int32),
        ("d_emb", C.c_int32),
        ("d_out", C.c_int32),
        ("conv_kernel", C.c_int32),
        ("bn_eps", C.c_float),
    ]


STYLE_MAX_CONVS = 8  # include/ttsdec.h TTSENC_STYLE_MAX_CONVS
STYLE_ENCODER, STYLE_VAE, STYLE_GST, STYLE_GST_VAE = 0, 1, 2, 3  # ttsenc_style_dims.kind
STYLE_W_STAGES, STYLE_W_PER_STAGE = 13, 6  # TTSENC_STYLE_W_STAGES / _PER_STAGE


class StyleDims(C.Structure):  # include/ttsdec.h ttsenc_style_dims
    _fields_ = [("n_mels", C.c_int32), ("n_convs", C.c_int32), ("filters", C.c_int32 * STYLE_MAX_CONVS), ("d_enc", C.c_int32),
                ("kind", C.c_int32), ("d_emb", C.c_int32), ("d_vae", C.c_int32), ("n_tokens", C.c_int32), ("n_heads", C.c_int32),
                ("bn_eps", C.c_float)]


class VitsDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_vocab", "inter_channels", "hidden_channels", "filter_channels", "n_heads", "n_layers", "kernel_size", "window_size",
        "flow_hidden", "flow_kernel", "flow_wn_layers", "n_flows", "flow_tf_layers", "flow_tf_heads", "flow_tf_kernel", "gin_channels", "cond_layer_idx")]


GEN_MAX_UP, GEN_MAX_RES = 8, 4  # include/ttsdec.h TTSGEN_MAX_UP / TTSGEN_MAX_RES


class GenDims(C.Structure):  # include/ttsdec.h ttsgen_dims
    _fields_ = [("initial_channel", C.c_int32), ("upsample_initial_channel", C.c_int32), ("n_up", C.c_int32),
                ("up_rates", C.c_int32 * GEN_MAX_UP), ("up_kernels", C.c_int32 * GEN_MAX_UP), ("n_res", C.c_int32),
                ("res_kernels", C.c_int32 * GEN_MAX_RES), ("res_dilations", (C.c_int32 * 3) * GEN_MAX_RES), ("n_dil", C.c_int32),
                ("resblock", C.c_int32), ("gin_channels", C.c_int32)]


class DiscDims(C.Structure):  # include/ttsdec.h ttsvits_disc_dims
    _fields_ = [(n, C.c_int32) for n in ("period", "kernel_size", "stride")]


class DurDiscDims(C.Structure):  # include/ttsdec.h ttsvits_durdisc_dims
    _fields_ = [(n, C.c_int32) for n in ("version", "in_channels", "filter_channels", "kernel_size")]


class DurNllDims(C.Structure):  # include/ttsdec.h ttsvits_durnll_dims
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "kernel_size", "n_flows", "gin_channels")]


DUR_SDP, DUR_DP = 0, 1  # include/ttsdec.h ttsdur_dims.kind
PATH_F32, PATH_F16, PATH_BF16 = 0, 1, 2  # include/ttsdec.h TTSVITS_PATH_*
ALIGN_MAX_TX = 1024  # tokens per utterance ttsvits_maximum_path is built for
VITS_MAX_HEAD_WIDTH = 256  # channels per attention head ttsvits_create accepts (csrc/vits2.hip dims_ok)


class DurDims(C.Structure):  # include/ttsdec.h ttsdur_dims
    _fields_ = [(n, C.c_int32) for n in ("kind", "in_channels", "filter_channels", "kernel_size", "n_flows", "gin_channels")]


class PostDims(C.Structure):  # include/ttsdec.h ttspost_dims
    _fields_ = [(n, C.c_int32) for n in ("spec_channels", "inter_channels", "hidden_channels", "kernel_size", "n_layers", "gin_channels")]


# One row per C-ABI family (include/ttsdec.h): its prefix, its dims struct, whether it has <prefix>_set_precision /
# _get_precision, and (restype, argtypes) of its own entry points.  Every family also has the shared ones of SHARED below.
vp, i32, u64, sz, f32 = C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_float
_ws_bytes = (sz, [vp, i32, i32])  # <prefix>_*workspace_bytes(h, B, T)


# entry points every handle has besides its create
_SHARED_SIGS = {
    "destroy": (i32, [vp]),
    "last_hip_error": (C.c_char_p, [vp]),
    "num_weight_tensors": (i32, [vp]),
    "packed_bytes": (sz, [vp]),
    "pack_weights": (i32, [vp, C.POINTER(vp), i32, vp, vp]),
    "bind_weights": (i32, [vp, vp]),
}


class Family(NamedTuple):
    prefix: str
    dims: type
    has_precision: bool
    own: Dict[str, Tuple[type, list]]


FAMILIES = (
    Family("ttsdec", Dims, True, {
        "version": (i32, []),
        "strerror": (C.c_char_p, [i32]),
        "set_option": (i32, [vp, i32, i32]),
        "get_option": (i32, [vp, i32, C.POINTER(i32)]),
        "option_name": (C.c_char_p, [i32]),
        "workspace_bytes": _ws_bytes,
        "decode": (i32, [
            vp, vp, i32, i32, i32, i32, i32,  # h, memory, B, L, t_begin, n_steps, t_stride
            f32, i32, i32, vp, u64,           # stop_threshold, check_stop, dropout_mode, masks, seed
            vp, i32, vp,                      # teacher, teacher_T, teacher_flags
            vp, vp, vp, vp,                   # y, s, w, T_out
            vp, sz, vp,                       # workspace, workspace_bytes, stream
        ]),
        "decode_each": (i32, [
            vp, vp, i32, i32, i32, i32, i32,  # h, memory, B, L, t_begin, n_steps, t_stride
            f32, i32, vp, u64,                # stop_threshold, dropout_mode, masks, seed
            vp, i32, vp,                      # teacher (NULL), teacher_T, teacher_flags
            vp, vp, vp, vp, vp,               # y, s, w, stop_steps, T_out
            vp, sz, vp,                       # workspace, workspace_bytes, stream
        ]),
        "zero_tail": (i32, [vp, vp, vp, i32, i32, C.c_int64, i32, i32, vp]),  # h, x, lengths, B, T, batch_stride, C, len_div, stream
        # the Tacotron validation step's loss terms (csrc/valstep.hip)
        "val_losses_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (h, B, T, S)
        "val_losses": (i32, [
            vp, vp, vp, vp, i32, vp, vp, vp,      # h, y, y_post, x, T_x, s, w, lengths
            i32, i32, i32, i32, i32, f32,         # B, T, D, S, L, pos_weight
            vp, vp, vp, sz, vp,                   # rows, terms, workspace, workspace_bytes, stream
        ]),
        "mel_loss": (i32, [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),  # h, y, x, T_x, lengths, B, T, D, order, rows, out, ws, bytes, stream
        "postnet_workspace_bytes": _ws_bytes,
        "postnet": (i32, [vp, vp, i32, i32, i32, vp, vp, sz, vp]),
        "postnet_ragged": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]),  # h, y, lengths, B, T, precision, y_post, ws, bytes, stream
        "cell_step": (i32, [
            vp, vp, vp, i32, i32,             # h, x, memory, B, L
            vp, vp, vp, vp, vp, vp,           # w, ctx, h_att, c_att, h_dec, c_dec
            i32, vp, u64, i32,                # dropout_mode, masks, seed, step
            vp, vp, sz, vp,                   # x_dec, workspace, workspace_bytes, stream
        ]),
        "profile_step": (i32, [
            vp, vp, i32, i32, i32, i32, vp, u64,  # h, memory, B, L, iters, dropout_mode, masks, seed
            vp, vp, vp, vp, sz, vp,               # y, s, w, workspace, workspace_bytes, stream
            C.POINTER(f32), C.POINTER(C.c_char_p), i32, C.POINTER(i32),
        ]),
        "profile_loop": (i32, [
            vp, vp, i32, i32, i32, i32, vp, u64,       # h, memory, B, L, n_steps, dropout_mode, masks, seed
            vp, vp, vp, vp, vp, sz, vp,                 # y, s, w, T_out, workspace, workspace_bytes, stream
            C.POINTER(f32), C.POINTER(C.c_char_p), i32, C.POINTER(i32), C.POINTER(f32),
        ]),
        "griffinlim_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (h, B, T, n_fft)
        "mel_to_magnitude": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
        "griffinlim": (i32, [
            vp, vp, vp, i32, i32, vp, i32, i32,  # h, mag, frames, B, T, window, n_fft, hop_length
            vp, vp, i32, f32, i32,               # angles, tprev, n_iter, momentum, normalize
            vp, vp, vp, vp, vp, sz, vp,          # wave, rebuilt_out, angles_out, status, workspace, workspace_bytes, stream
        ]),
        "mel_analysis_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (h, B, n_fft, n_mels)
        "mel_analysis": (i32, [
            vp, vp, vp, i32, i32, vp, vp,        # h, wave, lengths, B, n_samples, window, fb
            i32, i32, i32, i32,                  # n_mels, n_fft, hop_length, T
            vp, vp, vp, vp, vp, sz, vp,          # spec_db, mel_db, frames_out, status, workspace, workspace_bytes, stream
        ]),
        "resample_workspace_bytes": (sz, [vp, i32, i32, i32, f32]),  # (h, orig_freq, new_freq, lowpass_filter_width, rolloff)
        "resample": (i32, [
            vp, vp, vp, i32, i32, i32, i32, i32, f32,  # h, wave, lengths, B, n_samples, orig_freq, new_freq, lowpass_filter_width, rolloff
            vp, i32, vp, vp, vp, sz, vp,               # out, n_out, lengths_out, status, workspace, workspace_bytes, stream
        ]),
    }),
    Family("ttsenc", EncDims, True, {
        "workspace_bytes": _ws_bytes,
        "forward": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, sz, vp, vp]),
        # the style encoder: a second handle of this family (engine.Handle builds its names with PREFIX = "ttsenc_style")
        "style_create": (i32, [C.POINTER(StyleDims), C.POINTER(vp)]),
        **{f"style_{n}": sig for n, sig in _SHARED_SIGS.items()},
        "style_workspace_bytes": _ws_bytes,
        "style_forward": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),  # h, x, ldx, lengths, eps, B, T, enc_out, x_out, kl_out, ws, bytes, stream
    }),
    Family("ttsvits", VitsDims, True, {
        "text_encoder_workspace_bytes": _ws_bytes,
        "text_encoder": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp, vp]),
        "flow_workspace_bytes": _ws_bytes,
        "flow_reverse": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "flow_forward": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "align_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (h, B, T_y, T_x)
        "neg_cent": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
        "maximum_path": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, vp, sz, vp]),
        "align": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
        "spec_workspace_bytes": (sz, [vp, i32, i32]),  # (h, n_fft, n_mels)
        "spectrogram": (i32, [vp, vp, vp, i32, i32, vp, i32, i32, i32, vp, i32, vp, vp, sz, vp]),
        "spec_to_mel": (i32, [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, sz, vp]),
        "mel_spectrogram": (i32, [vp, vp, vp, i32, i32, vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, sz, vp]),
        # the validation step's glue (csrc/evalstep.hip)
        "kl_loss_workspace_bytes": _ws_bytes,  # (h, B, T_y)
        "kl_loss": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),  # h, z_p, logs_q, m_p, logs_p, frame_token, t_y, B, T_y, T_x, C, m_p_exp, logs_p_exp, kl_rows, kl, ws, bytes, stream
        "slice_segments": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),  # h, x, ids, ids_int64, B, outer, T, inner, seg, scale, out, status, stream
        "sliced_l1": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),  # h, a, y, ids, ids_int64, B, C, T_a, seg, l1_rows, l1, status, stream
        # the generator with its arithmetic as a call argument: these take a ttsgen handle (vits2.GenEngine)
        "generator_planes_bytes": (sz, [vp]),
        "generator_pack_planes": (i32, [vp, vp, vp]),  # gen, planes, stream
        "generator_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (gen, precision, B, T)
        "generator_forward": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]),  # gen, precision, planes, z, g, B, T, n_stages, out, ws, bytes, stream
        # the waveform discriminators: a second handle of this family (vits2.DiscEngine builds its names with PREFIX = "ttsvits_disc")
        "disc_create": (i32, [C.POINTER(DiscDims), C.POINTER(vp)]),
        **{f"disc_{n}": sig for n, sig in _SHARED_SIGS.items()},
        "disc_workspace_bytes": _ws_bytes,
        "disc_forward": (i32, [vp, vp, i32, i32, vp, C.POINTER(vp), vp, sz, vp]),  # h, y, B, T, scores, fmaps, ws, bytes, stream
        # the duration discriminators: a third handle of this family (vits2.DurDiscEngine, PREFIX = "ttsvits_durdisc")
        "durdisc_create": (i32, [C.POINTER(DurDiscDims), C.POINTER(vp)]),
        **{f"durdisc_{n}": sig for n, sig in _SHARED_SIGS.items()},
        "durdisc_workspace_bytes": (sz, [vp, i32, i32, i32]),  # (h, B, T, n_dur)
        "durdisc_trunk": (i32, [vp, vp, vp, i32, i32, vp, vp, sz, vp]),  # h, x, lengths, B, T, hidden_out, ws, bytes, stream
        "durdisc_prob": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]),  # h, hidden, lengths, dur, n_dur, B, T, prob, logit, ws, bytes, stream
        # the stochastic duration predictor's likelihood: a fourth handle of this family (vits2.DurNllEngine, PREFIX = "ttsvits_durnll")
        "durnll_create": (i32, [C.POINTER(DurNllDims), C.POINTER(vp)]),
        **{f"durnll_{n}": sig for n, sig in _SHARED_SIGS.items()},
        "durnll_workspace_bytes": _ws_bytes,
        "durnll_forward": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]),  # h, x, lengths, g, w, noise, B, T, nll, terms, z, ws, bytes, stream
    }),
    Family("ttsgen", GenDims, False, {
        "workspace_bytes": _ws_bytes,
        "forward": (i32, [vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "forward_stages": (i32, [vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    }),
    Family("ttsdur", DurDims, False, {
        "workspace_bytes": _ws_bytes,
        "sdp_reverse": (i32, [vp, vp, vp, vp, vp, f32, i32, i32, vp, vp, sz, vp]),
        "dp_forward": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "lengths": (i32, [vp, vp, vp, f32, i32, i32, vp, vp, vp, vp]),
        "expand": (i32, [vp, vp, vp, vp, vp, i32, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    }),
    Family("ttspost", PostDims, True, {
        "workspace_bytes": _ws_bytes,
        "forward": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    }),
)
SHARED = _SHARED_SIGS
PRECISION = {"set_precision": (i32, [vp, i32]), "get_precision": (i32, [vp])}


def _entry_points(fam: Family) -> Dict[str, Tuple[type, list]]:
    eps = {"create": (i32, [C.POINTER(fam.dims), C.POINTER(vp)]), **SHARED, **(PRECISION if fam.has_precision else {}), **fam.own}
    return {f"{fam.prefix}_{n}": sig for n, sig in eps.items()}


FAMILY_SYMBOLS = {fam.prefix: tuple(_entry_points(fam)) for fam in FAMILIES}
ALL_SYMBOLS = tuple(s for syms in FAMILY_SYMBOLS.values() for s in syms)  # every symbol include/ttsdec.h declares
# the same, under the names callers know: the decoder / encoder / VITS2 text-encoder-and-flow families, then one list per later family
SYMBOLS = FAMILY_SYMBOLS["ttsdec"] + FAMILY_SYMBOLS["ttsenc"] + FAMILY_SYMBOLS["ttsvits"]
GEN_SYMBOLS, DUR_SYMBOLS, POST_SYMBOLS = (FAMILY_SYMBOLS[p] for p in ("ttsgen", "ttsdur", "ttspost"))


class TtsdecError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str = ""):
        self.code = code
        msg = f"{what}: {_strerror(code)} (code {code})"
        if detail:
            msg += f" [{detail}]"
        super().__init__(msg)


class DimsNotBuilt(TtsdecError, NotImplementedError):
    """ERR_DIMS from a family's create: dimensions the library has no kernels for."""


_lib = None
_lock = threading.Lock()


def _strerror(code: int) -> str:
    try:
        return load().ttsdec_strerror(code).decode()
    except Exception:  # pragma: no cover
        return "?"


def load() -> C.CDLL:
    """Loads libttsdec.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python torch-tts_amd/build.py, or __graft_entry__.build()). "
                "There is no CPU fallback for this path."
            )
        lib = C.CDLL(LIB_PATH)
        lib.ttsdec_version.restype = i32
        lib.ttsdec_version.argtypes = []
        got = lib.ttsdec_version()
        if got != ABI_VERSION:  # (an older or newer build, e.g. through TTSDEC_LIB: its entry points take other argument lists)
            raise RuntimeError(f"{LIB_PATH} has ABI version {got}, these bindings are for version {ABI_VERSION}: rebuild it "
                               "(python torch-tts_amd/build.py --force)")
        for fam in FAMILIES:
            for name, (restype, argtypes) in _entry_points(fam).items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return _lib


def check(code: int, what: str) -> None:
    if code != OK:
        raise TtsdecError(code, what)
