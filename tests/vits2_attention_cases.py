"""Inputs that drive each VITS2 attention kernel (torch-tts_amd/csrc/vits2.hip: mha_kernel, mha_mfma_kernel<DKH>,
mha_flash_kernel<DK>) to its own edges, and the tools that prove on the CPU that they do.

TEST INFRASTRUCTURE ONLY.  Nothing here needs a GPU or the native library: tests/test_vits2_attention_host.py checks the cases
themselves (which kernel run_stack picks, where the flash kernel's lazy maximum moves, how well conditioned the inputs are, what a
planted fault would cost), tests/test_vits2_attention_hip.py runs them through the library.

The attention kernels are reachable only through TextEncoder and ResidualCouplingTransformersBlock, so a case is a whole module
input: weights in the oracle's state-dict layout plus ids or z.  The flow's attention width is inter_channels / 2 with 2 heads
(dk = channels / 4), the text encoder's hidden_channels with n_heads."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from oracle import vits2_oracle as V

RTOL, ATOL = 1e-4, 1e-5  # the project's bar (tests/test_vits2_hip.py)
LOG2E = 1.4426950408889634
MASKED2 = -1e4 * LOG2E  # masked_fill(mask == 0, -1e4) in the flash kernel's base-2 domain
FLASH_TILE, FLASH_LAZY = 32, 8.0  # keys per tile; how far a tile's maximum must exceed the running one before it moves
FAULTS = ("skip_lsum", "skip_y", "rescale_after_p", "wave_uniform_alpha")


# --------------------------------------------------------------------------
# run_stack's choice of kernel, restated
# --------------------------------------------------------------------------
def mha_mfma_lds_bytes(T: int, dk: int, window: int) -> int:
    """size_t mha_mfma_lds_bytes(int T, int dk, int window) {
         const size_t rel = (window >= 0 ? 32 * 33 : 0) + 32;  // relative-key logits, 1 / row sums
         const size_t s = (size_t)kMhaMRows * (T | 1) + rel;
         const size_t red = (size_t)4 * 32 * (dk + 1) + (size_t)(window >= 0 ? 2 * window + 1 : 0) * dk;  // partial tiles, E_v
         return (s > red ? s : red) * sizeof(float);
       }                                                       (kMhaMRows = 32)"""
    rel = (32 * 33 if window >= 0 else 0) + 32
    s = 32 * (T | 1) + rel
    red = 4 * 32 * (dk + 1) + (2 * window + 1 if window >= 0 else 0) * dk
    return max(s, red) * 4


def mha_lds_bytes(T: int, dk: int, window: int) -> int:
    """size_t mha_lds_bytes(int T, int dk, int window) {
         const int nrel = window >= 0 ? 2 * window + 1 : 0;
         return ((size_t)kMhaRows * dk + (size_t)kMhaChunk * (dk + 1) + 2 * (size_t)nrel * dk + (size_t)kMhaRows * T) * sizeof(float);
       }                                                       (kMhaRows = 16, kMhaChunk = 64)"""
    nrel = 2 * window + 1 if window >= 0 else 0
    return (16 * dk + 64 * (dk + 1) + 2 * nrel * dk + 16 * T) * 4


MHA_MAX_LDS = 150 * 1024  # constexpr size_t kMhaMaxLds = 150 * 1024;


def mha_choice(T: int, dk: int, window: Optional[int], precision: str, C: int) -> str:
    """The attention kernel run_stack launches for T frames, head width dk, relative window `window` (None or -1: none),
    precision "f32" / "split_f16" and attention width C: "scalar", "mfma<DKH>" or "flash<DK>".  ValueError where run_stack
    returns TTSDEC_ERR_DIMS.  A restatement - the source it mirrors:

        const size_t lds_m = mha_mfma_lds_bytes(T, dk, sd.window);
        const bool use_mfma = lds_m <= kMhaMaxLds && sd.window <= 15 && (dk == 96 || dk == 48 || dk == 16 || dk == 8);
        const size_t lds = use_mfma ? lds_m : mha_lds_bytes(T, dk, sd.window);
        if (lds > kMhaMaxLds || dk > 256) return TTSDEC_ERR_DIMS;
        const bool use_flash = sd.window < 0 && h->precision == TTSDEC_PREC_SPLIT_F16 && (dk == 48 || dk == 32 || dk == 64 || dk == 16) && !(C & 3);
        MhaLaunch mha{mha_kernel, ...};
        if (use_flash) {
          mha = dk == 48 ? flash_launch<48>(nb) : dk == 32 ? flash_launch<32>(nb) : dk == 64 ? flash_launch<64>(nb) : flash_launch<16>(nb);
        } else if (use_mfma) {
          mha.fn = dk == 96 ? mha_mfma_kernel<48> : dk == 48 ? mha_mfma_kernel<24> : dk == 16 ? mha_mfma_kernel<8> : mha_mfma_kernel<4>;
        }
    """
    assert precision in ("f32", "split_f16"), precision
    w = -1 if window is None else int(window)
    lds_m = mha_mfma_lds_bytes(T, dk, w)
    use_mfma = lds_m <= MHA_MAX_LDS and w <= 15 and dk in (96, 48, 16, 8)
    lds = lds_m if use_mfma else mha_lds_bytes(T, dk, w)
    if lds > MHA_MAX_LDS or dk > 256:
        raise ValueError(f"TTSDEC_ERR_DIMS: T={T} dk={dk} window={w} needs {lds} bytes of LDS")
    if w < 0 and precision == "split_f16" and dk in (48, 32, 64, 16) and not C & 3:
        return f"flash<{dk}>"
    if use_mfma:
        return f"mfma<{dk // 2}>"
    return "scalar"


def flash_grid_order(B: int, heads: int) -> str:
    """mha_flash_kernel:  const int npair = gridDim.x / nqb;  if (npair % 8 == 0) { (the XCD remap) } else { (plain order) }"""
    return "remap" if (B * heads) % 8 == 0 else "plain"


# --------------------------------------------------------------------------
# the flash kernel's online softmax, restated in fp64
# --------------------------------------------------------------------------
def lazy_max_moves(scores: torch.Tensor, n_valid: int) -> torch.Tensor:
    """Where mha_flash_kernel's lazy running maximum moves.  scores [..., query, key]: base-2 scores after the mask fill
    (MASKED2 where mask_q * mask_k == 0); keys >= n_valid do not exist.  Returns bool [tile, ..., query]; row 0 (the first tile,
    where m_run leaves -3e38 and alpha = 0 multiplies zeros) is excluded: all False.  The rule it mirrors:

        const bool move = tmax > m_run + 8.0f;  // (first tile: m_run = -3e38)
        ... const float m_new = move ? tmax : m_run;
    """
    nt = (n_valid + FLASH_TILE - 1) // FLASH_TILE
    out = torch.zeros((nt,) + tuple(scores.shape[:-1]), dtype=torch.bool)
    m_run = scores[..., :min(FLASH_TILE, n_valid)].amax(-1)
    for t in range(1, nt):
        tmax = scores[..., t * FLASH_TILE:min((t + 1) * FLASH_TILE, n_valid)].amax(-1)
        move = tmax > m_run + FLASH_LAZY
        out[t] = move
        m_run = torch.where(move, tmax, m_run)
    return out


def _group_alpha(alpha: torch.Tensor, move: torch.Tensor) -> torch.Tensor:
    """The alpha of the first moving query of every aligned 32-query group, for the whole group (1 where none moves)."""
    T = alpha.shape[-1]
    pad = (-T) % 32
    a = torch.nn.functional.pad(alpha, (0, pad), value=1.0).unflatten(-1, (-1, 32))
    m = torch.nn.functional.pad(move, (0, pad), value=False).unflatten(-1, (-1, 32))
    first = m.int().argmax(-1, keepdim=True)
    ga = torch.where(m.any(-1, keepdim=True), a.gather(-1, first), torch.ones_like(a[..., :1]))
    return ga.expand_as(a).flatten(-2)[..., :T]


def flash_emulation(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, fault: Optional[str] = None) -> torch.Tensor:
    """mha_flash_kernel's algorithm in the dtype of its inputs (fp64 here): q (already divided by sqrt(dk)), k, v [..., T, dk],
    mask [..., T] of 0 / 1 -> out [..., T, dk].  Keys in tiles of 32, the last one ragged (keys >= T excluded), scores in the base-2
    domain, MASKED2 where mask_q * mask_k == 0, the lazy running maximum with threshold 8, every quantity on the old scale
    rescaled by alpha = 2^(m_run - m_new) BEFORE the tile's p are formed, out = y / lsum.

    fault plants one of the mistakes the rescale invites (from the second tile on; on the first the sums are zero):
      "skip_lsum"           lsum is not rescaled
      "skip_y"              the accumulators are not rescaled
      "rescale_after_p"     the tile's p and P V are added first, then everything is multiplied by alpha
      "wave_uniform_alpha"  the alpha of the first moving query of a 32-query group (one wave's queries) is used by the whole group"""
    assert fault is None or fault in FAULTS, fault
    T = q.shape[-2]
    q2 = q * LOG2E
    m_run = torch.full(q.shape[:-1], -3.0e38, dtype=q.dtype)
    lsum = torch.zeros(q.shape[:-1], dtype=q.dtype)
    y = torch.zeros_like(q)
    for t in range((T + FLASH_TILE - 1) // FLASH_TILE):
        j0, j1 = t * FLASH_TILE, min((t + 1) * FLASH_TILE, T)
        s = q2 @ k[..., j0:j1, :].transpose(-1, -2)
        s = torch.where(mask[..., :, None] * mask[..., None, j0:j1] == 0, torch.full_like(s, MASKED2), s)
        tmax = s.amax(-1)
        move = tmax > m_run + FLASH_LAZY
        m_new = torch.where(move, tmax, m_run)
        alpha = torch.exp2(m_run - m_new)
        planted = fault if t > 0 else None
        if planted == "wave_uniform_alpha":
            alpha = _group_alpha(alpha, move)
        m_run = m_new
        p = torch.exp2(s - m_run[..., None])
        ps, pv = p.sum(-1), p @ v[..., j0:j1, :]
        if planted == "rescale_after_p":
            lsum = (lsum + ps) * alpha
            y = (y + pv) * alpha[..., None]
            continue
        lsum = (lsum if planted == "skip_lsum" else lsum * alpha) + ps
        y = (y if planted == "skip_y" else y * alpha[..., None]) + pv
    return y / lsum[..., None]


def exact_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """softmax(masked scores) @ v as attentions.py states it (natural-log domain, masked_fill -1e4), same shapes as above."""
    s = q @ k.transpose(-1, -2)
    s = s.masked_fill(mask[..., :, None] * mask[..., None, :] == 0, -1e4)
    return torch.softmax(s, -1) @ v


def base2_scores(q: torch.Tensor, k: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    s = (q * LOG2E) @ k.transpose(-1, -2)
    return torch.where(mask[..., :, None] * mask[..., None, :] == 0, torch.full_like(s, MASKED2), s)


def bar_units(out: torch.Tensor, ref: torch.Tensor, rtol: float = RTOL, atol: float = ATOL) -> float:
    """max over elements of err / (atol + rtol * |ref|): <= 1 is inside the bar."""
    out, ref = out.detach().cpu().double(), ref.detach().cpu().double()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    return float(((out - ref).abs() / (atol + rtol * ref.abs())).max())


# --------------------------------------------------------------------------
# flow cases: ResidualCouplingTransformersBlock, reverse, n_flows = 1, flow_hidden = 64
# --------------------------------------------------------------------------
_SMALL_TEXT = dict(n_vocab=8, hidden_channels=16, filter_channels=16, n_layers=1)  # (the flow cases never run the text encoder)
_ATT = "flow.flows.0.pre_transformer.attn_layers"
RAMP_STEP = 1.0 / 256.0  # the ramp channel's step per frame: j / 256 is exact in fp32 and in one fp16 plane


def ramp_qt(dk: int) -> float:
    """The ramp cases' q / sqrt(dk) in every channel: the power of two that gives a slope of at least 0.5 nats per key."""
    return 2.0 ** math.ceil(math.log2(0.5 / (dk * RAMP_STEP)))


def ramp_slope(dk: int) -> float:
    """nats per key of the ramp cases' scores"""
    return dk * ramp_qt(dk) * RAMP_STEP


@dataclass(frozen=True)
class FlowCase:
    name: str
    dims: V.Vits2Dims
    wts: dict
    z: torch.Tensor  # [B, channels, T]
    lengths: Tuple[int, ...]

    @property
    def T(self) -> int:
        return self.z.shape[2]

    @property
    def ymask(self) -> torch.Tensor:
        return V.sequence_mask(torch.tensor(self.lengths), self.T).unsqueeze(1).float()

    @property
    def C(self) -> int:  # the attention's width
        return self.dims.inter_channels // 2

    @property
    def dk(self) -> int:
        return self.C // self.dims.flow_tf_heads

    def choice(self, precision: str) -> str:
        return mha_choice(self.T, self.dk, None, precision, self.C)

    def reference(self, dtype=torch.float64) -> torch.Tensor:
        """The oracle's flow_reverse in `dtype`, returned as fp32 (computed once per case and dtype; do not modify)."""
        key = (self.name, dtype)
        if key not in _REFS:
            wts = {k: v.to(dtype) for k, v in self.wts.items()}
            _REFS[key] = V.flow_reverse(self.z.to(dtype), self.ymask.to(dtype), wts, self.dims).float()
        return _REFS[key]

    def reference_with_fault(self, fault: Optional[str]) -> torch.Tensor:
        """The fp64 oracle with the first attention layer's softmax(Q K^T) V replaced by flash_emulation(fault): what a flash kernel
        with that fault would hand the rest of the flow, carried through to the flow's output."""
        orig = V.mha

        def mha(x, attn_mask, wts, prefix, n_heads, window):
            if not prefix.endswith("attn_layers.0"):
                return orig(x, attn_mask, wts, prefix, n_heads, window)
            B, C, T = x.shape
            conv = torch.nn.functional.conv1d
            q, k, v = (conv(x, wts[f"{prefix}.{nm}.weight"], wts[f"{prefix}.{nm}.bias"]).view(B, n_heads, C // n_heads, T).transpose(2, 3)
                       for nm in ("conv_q", "conv_k", "conv_v"))
            out = flash_emulation(q / math.sqrt(C // n_heads), k, v, attn_mask.amax(-1), fault)
            return conv(out.transpose(2, 3).contiguous().view(B, C, T), wts[prefix + ".conv_o.weight"], wts[prefix + ".conv_o.bias"])

        V.mha = mha
        try:
            wts = {k: v.double() for k, v in self.wts.items()}
            return V.flow_reverse(self.z.double(), self.ymask.double(), wts, self.dims).float()
        finally:
            V.mha = orig

    def layer0_qkv(self):
        """fp64 q / sqrt(dk), k, v [B, heads, T, dk] of the first attention layer and the frame mask [B, 1, T] (broadcasts over
        the heads): what mha_* is launched on for layer 0 (coupling_reverse: Flip, first half, times the mask)."""
        w = {k: v.double() for k, v in self.wts.items() if k.startswith(_ATT + ".0.")}
        mask = self.ymask.double()
        x0 = torch.flip(self.z.double(), [1])[:, :self.C] * mask
        B, h, dk = x0.shape[0], self.dims.flow_tf_heads, self.dk
        out = []
        for nm in ("conv_q", "conv_k", "conv_v"):
            t = torch.nn.functional.conv1d(x0, w[f"{_ATT}.0.{nm}.weight"], w[f"{_ATT}.0.{nm}.bias"])
            out.append(t.view(B, h, dk, self.T).transpose(2, 3))
        return out[0] / math.sqrt(dk), out[1], out[2], mask


_REFS: dict = {}


def _flow_dims(channels: int) -> V.Vits2Dims:
    return V.Vits2Dims(inter_channels=channels, n_flows=1, flow_hidden=64, **_SMALL_TEXT)


def _z(channels: int, B: int, T: int, seed: int) -> torch.Tensor:
    return torch.randn(B, channels, T, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def scaled(channels: int, s: float = 6.0, B: int = 2, T: int = 300, lengths: Tuple[int, ...] = (300, 223), wseed: int = 17,
           zseed: int = 5) -> FlowCase:
    """random_vits2_weights with conv_q.weight and conv_q.bias of both pre_transformer layers times s: scores with a standard
    deviation of about s nats instead of 1, so the lazy maximum moves at some tiles for some queries (alpha strictly inside
    (0, 1)) and not for their neighbours."""
    d = _flow_dims(channels)
    wts = V.random_vits2_weights(d, seed=wseed)
    for i in range(d.flow_tf_layers):
        for t in ("weight", "bias"):
            wts[f"{_ATT}.{i}.conv_q.{t}"] = wts[f"{_ATT}.{i}.conv_q.{t}"] * s
    return FlowCase(f"scaled-{channels}-s{s:g}-B{B}-T{T}-{'.'.join(map(str, lengths))}-w{wseed}-z{zseed}", d, wts, _z(channels, B, T, zseed),
                    tuple(lengths))


@functools.lru_cache(maxsize=None)
def ramp(channels: int, direction: str, B: int = 2, T: int = 300, lengths: Tuple[int, ...] = (300, 223), wseed: int = 17,
         zseed: int = 5) -> FlowCase:
    """Layer-0 attention with planted weights: every valid query sees score_j = +-ramp_slope(dk) * j nats.
      conv_q.weight = 0, conv_q.bias = +-a in every channel;  conv_k.weight copies channel 0 of x0 into every channel, conv_k.bias = 0;
      channel 0 of x0 (after the Flip: the LAST channel of z) is the ramp j * RAMP_STEP = j / 256
      => score_j = sum_d (a / sqrt(dk)) (j / 256) = dk qt j / 256 with qt = a / sqrt(dk).
    qt is a power of two (a = qt * float32(sqrt(dk)), which the kernels' division by sqrtf(dk) takes back to qt exactly), so
    every product and partial sum of a score is an integer multiple of 2^-8 below 2^16: exact in fp32 in any order, and what is
    left of the comparison is the softmax and P V.  The slope dk qt / 256 is 0.5 nats per key, 0.75 at dk = 48 and 96: 23 (35) in
    base 2 per full tile, and 8.66 (13) across the 12 keys of the ragged last tile at T = 300 - above the threshold of 8 there
    too (0.25 per key would move at every full tile but not at that one).  "ascending": the maximum moves at every tile that holds
    a valid key; "descending": never after the first.  Everything else is random, layer 1 included."""
    assert direction in ("ascending", "descending"), direction
    d = _flow_dims(channels)
    wts = V.random_vits2_weights(d, seed=wseed)
    C = channels // 2
    dk = C // d.flow_tf_heads
    a = ramp_qt(dk) * float(torch.tensor(float(dk)).sqrt()) * (1.0 if direction == "ascending" else -1.0)
    wts[f"{_ATT}.0.conv_q.weight"] = torch.zeros(C, C, 1)
    wts[f"{_ATT}.0.conv_q.bias"] = torch.full((C,), a)
    wk = torch.zeros(C, C, 1)
    wk[:, 0, 0] = 1.0
    wts[f"{_ATT}.0.conv_k.weight"] = wk
    wts[f"{_ATT}.0.conv_k.bias"] = torch.zeros(C)
    z = _z(channels, B, T, zseed)
    z[:, channels - 1, :] = torch.arange(T, dtype=torch.float32) * RAMP_STEP
    return FlowCase(f"ramp-{channels}-{direction}-B{B}-T{T}-{'.'.join(map(str, lengths))}-w{wseed}-z{zseed}", d, wts, z, tuple(lengths))


# --------------------------------------------------------------------------
# text-encoder cases: the relative-position window
# --------------------------------------------------------------------------
@dataclass(frozen=True)
class TextCase:
    name: str
    dims: V.Vits2Dims
    wts: dict
    ids: torch.Tensor  # [B, T]
    lengths: Tuple[int, ...]

    @property
    def T(self) -> int:
        return self.ids.shape[1]

    @property
    def dk(self) -> int:
        return self.dims.hidden_channels // self.dims.n_heads

    def choice(self, precision: str) -> str:
        return mha_choice(self.T, self.dk, self.dims.window_size, precision, self.dims.hidden_channels)

    def reference(self, dtype=torch.float64):
        """The oracle's (x, m, logs) in `dtype`, returned as fp32 (computed once per case and dtype; do not modify)."""
        key = (self.name, dtype)
        if key not in _REFS:
            wts = {k: v.to(dtype) for k, v in self.wts.items()}
            x, m, logs, _ = V.text_encoder(self.ids, torch.tensor(self.lengths), wts, self.dims)
            _REFS[key] = tuple(t.float() for t in (x, m, logs))
        return _REFS[key]


@functools.lru_cache(maxsize=None)
def text(hidden: int, window: int = 4, n_layers: int = 2, B: int = 3, T: int = 300, lengths: Tuple[int, ...] = (300, 161, 5), q_scale: float = 1.0,
         wseed: int = 13, idseed: int = 7) -> TextCase:
    """TextEncoder(hidden, 2 heads, window) on random_vits2_weights; q_scale multiplies conv_q.weight / .bias of every layer."""
    d = V.Vits2Dims(n_vocab=40, inter_channels=max(8, hidden // 2), hidden_channels=hidden, filter_channels=2 * hidden, n_heads=2, n_layers=n_layers,
                    window_size=window, n_flows=0)
    wts = V.random_vits2_weights(d, seed=wseed)
    if q_scale != 1.0:
        for i in range(n_layers):
            for t in ("weight", "bias"):
                wts[f"enc_p.encoder.attn_layers.{i}.conv_q.{t}"] = wts[f"enc_p.encoder.attn_layers.{i}.conv_q.{t}"] * q_scale
    ids = torch.randint(0, d.n_vocab, (B, T), generator=torch.Generator().manual_seed(idseed))
    return TextCase(f"text-{hidden}-w{window}-L{n_layers}-B{B}-T{T}-{'.'.join(map(str, lengths))}-q{q_scale:g}-w{wseed}-i{idseed}", d, wts, ids,
                    tuple(lengths))


# --------------------------------------------------------------------------
# the cases both test files run: (kind, channels, B, T, lengths) for the flow, text()'s arguments for the text encoder
# --------------------------------------------------------------------------
SCALE = 6.0  # the `scaled` cases' factor on conv_q
_BTL = (2, 300, (300, 223))


def flow_case(kind: str, channels: int, B: int = 2, T: int = 300, lengths: Tuple[int, ...] = (300, 223)) -> FlowCase:
    """kind "scaled", "ascending" or "descending"."""
    if kind == "scaled":
        return scaled(channels, SCALE, B, T, tuple(lengths))
    return ramp(channels, kind, B, T, tuple(lengths))


def spec_id(spec) -> str:
    return "-".join(".".join(map(str, s)) if isinstance(s, tuple) else f"{s:g}" if isinstance(s, float) else str(s) for s in spec)


FLASH_CHANNELS = (64, 128, 192, 256)
# split_f16: 4 (utterance, head) pairs -> the plain grid order
FLASH_MAIN = [(kind, ch) + _BTL for ch in FLASH_CHANNELS for kind in ("scaled", "ascending", "descending")]
# 8 pairs -> the XCD remap; lengths 97 and 1: whole workgroups of masked queries
FLASH_REMAP = [("scaled", 192, 4, 300, (300, 223, 97, 1))]
# one tile (T = 1, 32), a second tile of one key (33), a second workgroup with three idle staging waves (129)
FLASH_SHORT = [("scaled", 64, 3, T, (T, (T + 1) // 2, 1)) for T in (1, 32, 33, 129)]
# exact fp32 under large scores: mfma<4>, mfma<8> (T = 600: 19 key tiles, the 4-tile ring of each wave refills), scalar dk 32 / 64,
# mfma<24>, mfma<48> without window
EXACT_F32 = [(kind, ch) + btl for ch, btl in ((32, _BTL), (64, _BTL), (64, (2, 600, (600, 411))), (128, _BTL), (256, _BTL), (192, _BTL), (384, _BTL))
             for kind in ("scaled", "ascending")]
# split_f16 at head widths the flash kernel is not built for: the mfma kernel writes the out_p planes the output GEMM reads
EXACT_SPLIT = [(kind, ch) + _BTL for ch in (32, 384) for kind in ("scaled", "ascending")]
FLOW_SPECS = list(dict.fromkeys(FLASH_MAIN + FLASH_REMAP + FLASH_SHORT + EXACT_F32 + EXACT_SPLIT))

# (hidden, window, n_layers, B, T, lengths, q_scale)
_TEXT_BTL = (3, 300, (300, 161, 5))
TEXT_WIDTHS = [(h, 4, 2) + _TEXT_BTL + (1.0,) for h in (16, 32, 64, 96, 192)]  # mfma<4>, mfma<8>, scalar, mfma<24>, mfma<48>
TEXT_SCALE = 4.0  # conv_q x 6 leaves the fp32 oracle at 0.93 of the bar against its fp64 run, x 5 at 0.70 - 0.76, x 4 at 0.41
TEXT_SCALED = [(192, 4, 2) + _TEXT_BTL + (TEXT_SCALE,)]
TEXT_LDS_EDGE = [(192, 4, 1, 1, T, (T,), 1.0) for T in (1165, 1166)]  # the last mfma length, the first scalar length
TEXT_WINDOWS = [(32, w, 2, 3, 100, (100, 61, 5), 1.0) for w in (0, 15, 16)]  # finish<9> with one row, finish<31>, scalar
TEXT_SPECS = TEXT_WIDTHS + TEXT_SCALED + TEXT_LDS_EDGE + TEXT_WINDOWS
