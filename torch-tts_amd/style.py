"""Drop-ins for the reference's style encoders (tacotron/modules/style.py, modules/attention.py:129-186): ``ReferenceEncoder``,
``STL``, ``GST``, ``VAE``, ``GST_VAE`` and ``MultiHeadAttention`` with the reference's constructor signatures and state-dict keys.

In eval mode on a ROCm device, in fp32 and with no gradient wanted, the forward runs through ``ttsenc_style_forward``
(csrc/style.hip: a direct first conv, implicit-GEMM convs, one input-projection GEMM, packed-sequence LSTM steps and one tail
kernel); everything else - training, other dtypes, the CPU - takes ``_stock_forward`` on plain torch ops, which is differentiable
and uses batch statistics in training, as the reference does.  The model trains through these modules, hence Encoder2's dispatch
rule rather than the inference-only one of the VITS2 modules.

Differences from the reference, all on purpose:
  * ``forward(inputs, input_lengths=None, eps=None)``: the standard-normal draw of VAE / GST_VAE may be passed in (tests do);
    ``None`` draws it with ``torch.randn`` on the input's device, as ``randn_like`` would.
  * nothing is printed in eval mode (the reference prints three statistics from VAE and one from MultiHeadAttention, each a
    host synchronisation).
  * lengths may be a list, a host tensor or a device tensor.  A host-side length above the padded T raises ValueError (the
    reference raises from pack_padded_sequence); a DEVICE-side length is never read back by the HIP path - it is clamped to the
    T' steps there are - so that the call does not synchronise.
The convs are not masked: like the reference's they see whatever the padded frames hold."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib
from .engine import STREAM, WS, EngineCache, Handle, PackedWeightsMixin, _require_device

_HEAD_NAMES = ("encoder.gru.weight_ih_l0", "encoder.gru.weight_hh_l0", "encoder.gru.bias_ih_l0", "encoder.gru.bias_hh_l0",
               "mean_linear.weight", "mean_linear.bias", "logvar_linear.weight", "logvar_linear.bias", "fc_out.weight",
               "stl.embed", "stl.attention.W_query.weight", "stl.attention.W_key.weight", "stl.attention.W_value.weight")
_STAGE_NAMES = ("encoder.convs.{i}.weight", "encoder.convs.{i}.bias", "encoder.bns.{i}.weight", "encoder.bns.{i}.bias",
                "encoder.bns.{i}.running_mean", "encoder.bns.{i}.running_var")


class StyleEngine(Handle):
    """One ttsenc_style handle on one device; dims: the fields of _lib.StyleDims (filters as a tuple)."""

    PREFIX = "ttsenc_style"

    def __init__(self, dims: Dict, device: Optional[torch.device]):
        f = tuple(dims["filters"])
        if len(f) > _lib.STYLE_MAX_CONVS:
            raise _lib.DimsNotBuilt(_lib.ERR_DIMS, "ttsenc_style_create", f"more than {_lib.STYLE_MAX_CONVS} conv stages: {dims}")
        c = _lib.StyleDims(**{**dims, "n_convs": len(f), "filters": (_lib.C.c_int32 * _lib.STYLE_MAX_CONVS)(*f)})
        super().__init__(dims, c, device)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self._lib.ttsenc_style_workspace_bytes(self._h, B, T))

    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor], eps: Optional[torch.Tensor]):
        """x [B, T, n_mels] fp32 (rows may be a slice of a wider tensor), lengths [B] int32 on the device or None,
        eps [B, d_vae] or None -> (enc_out [B, d_enc], x_out [B, d_emb] or None, kl [B, d_vae] or None).  No host sync."""
        _require_device(x, "inputs")
        B, T, n_mels = x.shape
        if x.stride(2) != 1 or x.stride(0) != T * x.stride(1) or x.stride(1) < n_mels:
            x = x.contiguous()
        d = self.dims
        kind = d["kind"]
        new = lambda n: torch.empty(B, n, dtype=torch.float32, device=self.device)  # noqa: E731
        enc_out = new(d["d_enc"])
        x_out = new(d["d_emb"]) if kind != _lib.STYLE_ENCODER else None
        kl = new(d["d_vae"]) if kind in (_lib.STYLE_VAE, _lib.STYLE_GST_VAE) else None
        ws = self.workspace("forward", self.workspace_bytes(B, T))
        self.call("ttsenc_style_forward", x, x.stride(1), lengths, eps, B, T, enc_out, x_out, kl, WS(ws), STREAM)
        return enc_out, x_out, kl


def _host_lengths_check(lengths, T: int) -> None:
    """ValueError for a host-side length beyond the padded T; device tensors are not read (that would synchronise)."""
    if lengths is None or (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
        return
    top = int(max(lengths)) if not isinstance(lengths, torch.Tensor) else int(lengths.max())
    if top > T:
        raise ValueError(f"an utterance's length ({top}) exceeds the padded input's {T} frames")


def _device_lengths(lengths, device) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    return torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()


class MultiHeadAttention(nn.Module):
    """attention.py:129-186 without its eval-mode print: query [N, T_q, query_dim], key [N, T_k, key_dim] -> [N, T_q, num_units]."""

    def __init__(self, query_dim, key_dim, num_units, num_heads):
        super().__init__()
        self.num_units, self.num_heads = num_units, num_heads
        self.d_gain = 1 / (key_dim ** 0.5)
        self.W_query = nn.Linear(query_dim, num_units, bias=False)
        self.W_key = nn.Linear(key_dim, num_units, bias=False)
        self.W_value = nn.Linear(key_dim, num_units, bias=False)

    def forward(self, query, key, key_mask=None):
        split = self.num_units // self.num_heads
        heads = lambda t: torch.stack(torch.split(t, split, dim=2), dim=0)  # noqa: E731  [h, N, T, num_units / h]
        querys, keys, values = heads(self.W_query(query)), heads(self.W_key(key)), heads(self.W_value(key))
        scores = self.d_gain * torch.matmul(querys, keys.transpose(2, 3))
        if key_mask is not None:
            scores = scores.masked_fill(~(key_mask.unsqueeze(0).unsqueeze(2)), -1e6)
        scores = nn.functional.softmax(scores, dim=3)
        out = torch.matmul(scores, values)
        return torch.cat(torch.split(out, 1, dim=0), dim=3).squeeze(0)


class _StyleBase(PackedWeightsMixin, nn.Module):
    """What the four modules share: the weight list in the library's pack order, the dispatch rule and the engine cache."""

    KIND = _lib.STYLE_ENCODER

    def _init_engine(self):
        self._watch_state_dict_loads()
        self.use_hip = True  # eval-mode forwards on a ROCm device go through libttsdec
        self._engines = EngineCache(StyleEngine)

    def _ref_encoder(self) -> "ReferenceEncoder":
        return self.encoder

    def _prefix(self) -> str:
        return ""  # state-dict prefix of this module's own names inside weight_names()

    def weight_names(self) -> List[str]:
        """State-dict keys in the order of include/ttsdec.h TTSENC_STYLE_W_* (names this kind of module does not have included)."""
        K = len(self._ref_encoder().convs)
        return list(_HEAD_NAMES) + [n.format(i=i) for i in range(K) for n in _STAGE_NAMES]

    def weight_tensors(self):
        """The tensors of weight_names(); None where this module has no such tensor."""
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        strip = "encoder." if isinstance(self, ReferenceEncoder) else None
        out = []
        for n in self.weight_names():
            if strip is not None:
                n = n[len(strip):] if n.startswith(strip) else "\0"
            out.append(sd.get(n))
        return out

    def style_dims(self) -> Dict:
        enc = self._ref_encoder()
        d = dict(n_mels=enc.num_mels, filters=tuple(c.out_channels for c in enc.convs), d_enc=enc.gru.hidden_size, kind=self.KIND,
                 d_emb=0, d_vae=0, n_tokens=0, n_heads=0, bn_eps=float(enc.bns[0].eps))
        if hasattr(self, "fc_out"):
            d.update(d_emb=self.fc_out.out_features, d_vae=self.fc_out.in_features)
        if hasattr(self, "stl"):
            d.update(d_emb=self.stl.attention.num_units, n_tokens=self.stl.embed.shape[0], n_heads=self.stl.attention.num_heads)
        return d

    def _hip_ok(self, inputs) -> bool:
        return (self.use_hip and inputs.is_cuda and inputs.dtype == torch.float32 and not self.training
                and not (torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters())))
                and all(p.dtype == torch.float32 for p in self.parameters()) and self._dims_built())

    def _dims_built(self) -> bool:
        """ttsenc_style_create's rule (csrc/style.hip), so that a module it would refuse takes the stock path instead of raising."""
        d = self.style_dims()
        f, kind = d["filters"], d["kind"]
        ok = d["n_mels"] > 0 and 1 <= len(f) <= _lib.STYLE_MAX_CONVS and all(0 < c <= 1024 and c % 4 == 0 for c in f)
        ok = ok and 0 < d["d_enc"] <= 1024 and d["d_enc"] % 4 == 0
        if kind != _lib.STYLE_ENCODER:
            ok = ok and 0 < d["d_emb"] <= 1024
        if kind in (_lib.STYLE_VAE, _lib.STYLE_GST_VAE):
            ok = ok and 0 < d["d_vae"] <= 256
        if kind in (_lib.STYLE_GST, _lib.STYLE_GST_VAE):
            ok = ok and 0 < d["n_tokens"] <= 64 and 0 < d["n_heads"] <= 16 and d["d_emb"] % d["n_heads"] == 0
        return ok

    def _hip_forward(self, inputs, input_lengths, eps):
        _host_lengths_check(input_lengths, inputs.shape[1])
        eng = self._engines.get(self.style_dims(), inputs.device)
        eng.ensure_packed(self.weight_tensors())
        return eng.forward(inputs, _device_lengths(input_lengths, inputs.device), eps)

    def _draw(self, like_rows: int, inputs, eps):
        if eps is not None:
            return eps.to(device=inputs.device, dtype=inputs.dtype)
        return torch.randn(like_rows, self.fc_out.in_features, device=inputs.device, dtype=inputs.dtype)


class ReferenceEncoder(_StyleBase):
    """inputs [N, T, num_mels] -> [N, dim_out]: the last LSTM state over the conv stack's output (style.py:7-76)."""

    def __init__(self, num_mels=80, dim_out=128, ref_enc_filters=[32, 32, 64, 64, 128, 128]):
        super().__init__()
        self._init_engine()
        K = len(ref_enc_filters)
        filters = [1] + list(ref_enc_filters)
        self.convs = nn.ModuleList([nn.Conv2d(filters[i], filters[i + 1], kernel_size=(3, 3), stride=(2, 2), padding=(1, 1)) for i in range(K)])
        self.bns = nn.ModuleList([nn.BatchNorm2d(num_features=ref_enc_filters[i]) for i in range(K)])
        self.num_mels = num_mels
        self.gru = nn.LSTM(input_size=ref_enc_filters[-1] * self.calculate_channels(num_mels, 3, 2, 1, K), hidden_size=dim_out, batch_first=True)

    def _ref_encoder(self):
        return self

    @staticmethod
    def calculate_channels(L, kernel_size, stride, pad, n_convs):
        for _ in range(n_convs):
            L = (L - kernel_size + 2 * pad) // stride + 1
        return L

    def _stock_forward(self, inputs, input_lengths=None):
        out = inputs.unsqueeze(1)
        for conv, bn in zip(self.convs, self.bns):
            out = nn.functional.relu(bn(conv(out)))
        out = out.transpose(1, 2)
        N, T = out.size(0), out.size(1)
        out = out.contiguous().view(N, T, -1)
        if input_lengths is not None:
            _host_lengths_check(input_lengths, inputs.shape[1])
            lens = torch.as_tensor(input_lengths)
            lens = torch.clip((lens / 2 ** len(self.convs)).long(), min=1)
            if lens.is_cuda:  # (a device-side length is clamped like the HIP path clamps it)
                lens = torch.clip(lens, max=T)
            out = nn.utils.rnn.pack_padded_sequence(out, lens.cpu(), batch_first=True, enforce_sorted=False)
        _, out = self.gru(out)
        return out[0].squeeze(0)

    def forward(self, inputs, input_lengths=None):
        if not self._hip_ok(inputs):
            return self._stock_forward(inputs, input_lengths)
        return self._hip_forward(inputs, input_lengths, None)[0]


class STL(nn.Module):
    """inputs [N, dim_query] -> [N, 1, dim_emb]: attention of the reference embedding over tanh(token embeddings) (style.py:79-109)."""

    def __init__(self, dim_query=128, num_tokens=10, dim_emb=256, num_heads=4):
        super().__init__()
        self.embed = nn.Parameter(torch.empty(num_tokens, dim_emb // num_heads))
        self.attention = MultiHeadAttention(query_dim=dim_query, key_dim=dim_emb // num_heads, num_units=dim_emb, num_heads=num_heads)
        nn.init.normal_(self.embed, mean=0, std=0.5)

    def forward(self, inputs):
        N = inputs.size(0)
        keys = torch.tanh(self.embed).unsqueeze(0).expand(N, -1, -1)
        return self.attention(inputs.unsqueeze(1), keys)


def _vae_head(m, h, eps):
    """mean / logvar / z / kl of VAE and GST_VAE (style.py:137-142)."""
    z_mean, z_logvar = m.mean_linear(h), m.logvar_linear(h)
    z = eps.view_as(z_mean) * torch.exp(0.5 * z_logvar) + z_mean
    kl = -(1 + z_logvar - z_mean * z_mean - z_logvar.exp()) / 2
    return z, kl


class GST(_StyleBase):
    KIND = _lib.STYLE_GST

    def __init__(self, num_mels=80, dim_emb=256, dim_enc=128, num_tokens=10, num_heads=4):
        super().__init__()
        self._init_engine()
        self.encoder = ReferenceEncoder(num_mels=num_mels, dim_out=dim_enc)
        self.stl = STL(dim_query=dim_enc, num_tokens=num_tokens, dim_emb=dim_emb, num_heads=num_heads)

    def _stock_forward(self, inputs, input_lengths=None, eps=None):
        return self.stl(self.encoder._stock_forward(inputs, input_lengths)), {}

    def forward(self, inputs, input_lengths=None, eps=None):
        if not self._hip_ok(inputs):
            return self._stock_forward(inputs, input_lengths)
        _, x, _ = self._hip_forward(inputs, input_lengths, None)
        return x.unsqueeze(1), {}


class VAE(_StyleBase):
    KIND = _lib.STYLE_VAE

    def __init__(self, num_mels=80, dim_emb=256, dim_enc=128, dim_vae=16):
        super().__init__()
        self._init_engine()
        self.encoder = ReferenceEncoder(num_mels=num_mels, dim_out=dim_enc)
        self.mean_linear = nn.Linear(dim_enc, dim_vae)
        self.logvar_linear = nn.Linear(dim_enc, dim_vae)
        self.fc_out = nn.Linear(dim_vae, dim_emb, bias=False)

    def _stock_forward(self, inputs, input_lengths=None, eps=None):
        enc_out = self.encoder._stock_forward(inputs, input_lengths)
        z, kl = _vae_head(self, enc_out, self._draw(enc_out.shape[0], inputs, eps))
        return torch.tanh(self.fc_out(z).unsqueeze(1)), {"kl": kl}

    def forward(self, inputs, input_lengths=None, eps=None):
        if not self._hip_ok(inputs):
            return self._stock_forward(inputs, input_lengths, eps)
        eps = self._draw(inputs.shape[0], inputs, eps).reshape(inputs.shape[0], -1).contiguous()
        _, x, kl = self._hip_forward(inputs, input_lengths, eps)
        return x.unsqueeze(1), {"kl": kl}


class GST_VAE(_StyleBase):
    KIND = _lib.STYLE_GST_VAE

    def __init__(self, num_mels=80, dim_emb=256, dim_enc=128, num_tokens=10, num_heads=4, dim_vae=32):
        super().__init__()
        self._init_engine()
        self.encoder = ReferenceEncoder(num_mels=num_mels, dim_out=dim_enc)
        self.stl = STL(dim_query=dim_enc, num_tokens=num_tokens, dim_emb=dim_emb, num_heads=num_heads)
        self.mean_linear = nn.Linear(dim_emb, dim_vae)
        self.logvar_linear = nn.Linear(dim_emb, dim_vae)
        self.fc_out = nn.Linear(dim_vae, dim_emb, bias=False)

    def _stock_forward(self, inputs, input_lengths=None, eps=None):
        style = self.stl(self.encoder._stock_forward(inputs, input_lengths))  # [N, 1, dim_emb]
        z, kl = _vae_head(self, style, self._draw(style.shape[0], inputs, eps))
        return self.fc_out(z), {"kl": kl}  # x [N, 1, dim_emb], kl [N, 1, dim_vae]

    def forward(self, inputs, input_lengths=None, eps=None):
        if not self._hip_ok(inputs):
            return self._stock_forward(inputs, input_lengths, eps)
        eps = self._draw(inputs.shape[0], inputs, eps).reshape(inputs.shape[0], -1).contiguous()
        _, x, kl = self._hip_forward(inputs, input_lengths, eps)
        return x.unsqueeze(1), {"kl": kl.unsqueeze(1)}
