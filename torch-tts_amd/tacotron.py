"""Model assembly with the reference's API (tacotron/tacotron.py:20-56,165-224):
``Tacotron(encoder, decoder, postnet, refencoder).forward(...) -> (y, y_post, s,
{"w", "kl_loss"})`` and ``build_tacotron(config)``.  The decoder and postnet are the
HIP-backed drop-ins of this package; so are the encoder (torch-tts_amd/encoder.py) and the style
encoder (torch-tts_amd/style.py) in eval mode; both run once per batch, before the hot path.
``fast_inference()`` leaves the style encoder in exact fp32: it has no other arithmetic."""
from __future__ import annotations

import torch
import torch.nn as nn

from .decoder import Decoder
from .engine import PackedWeightsMixin
from .decoder_cell import Taco2DecoderCell, Taco2ProdDecoderCell
from .encoder import Encoder2
from .postnet import MelPostnet, MelPostnet2
from .style import VAE


def lengths_to_mask(lengths):
    """Boolean [B, max(lengths)] mask (tacotron/data/util.py:4-7)."""
    idx = torch.arange(int(lengths.max()), device=lengths.device)
    return idx.unsqueeze(0) < lengths.unsqueeze(1)


def weights_init(m):
    # tacotron.py:12-17
    if isinstance(m, (nn.Conv1d, nn.Linear)):
        if m.weight is not None:
            nn.init.xavier_normal_(m.weight, gain=1.5)
        if m.bias is not None:
            nn.init.zeros_(m.bias)


class Tacotron(PackedWeightsMixin, nn.Module):
    def __init__(self, encoder, decoder, postnet=None, refencoder=None):
        super().__init__()
        self.refencoder = refencoder
        self.encoder = encoder
        self.decoder = decoder
        self.postnet = postnet
        self.apply(weights_init)

    def fast_inference(self, seed: int = 0):
        """One switch for the fast configuration of the HIP path (inference only):
          * PreNet dropout drawn on the device (Philox, keyed by `seed`) instead of replaying the reference's CPU generator -
            the default `dropout_source = "reference_rng"` draws ~80 MB of masks on the host and uploads them per 256 x 600
            batch, which exists for bit-compatibility with the reference's RNG stream, not for speed;
          * split-fp16 arithmetic (fp32-class accuracy: 22 significand bits per operand, fp32 accumulate) for the decoder's
            the Postnet's and the text encoder's GEMMs instead of exact fp32 matrix instructions (about 0.6 of the step time at
            256 utterances).
        Returns self; `reference_compatible()` switches back."""
        self.decoder.dropout_source, self.decoder.dropout_seed, self.decoder.precision = "philox", int(seed), "split_f16"
        for m in (self.postnet, self.encoder):
            if m is not None and hasattr(m, "precision"):
                m.precision = "split_f16"
        return self

    def reference_compatible(self):
        """The defaults: the reference's RNG stream for the always-on PreNet dropout, exact fp32 arithmetic."""
        self.decoder.dropout_source, self.decoder.precision = "reference_rng", "f32"
        for m in (self.postnet, self.encoder):
            if m is not None and hasattr(m, "precision"):
                m.precision = "f32"
        return self

    def forward(self, cond, cond_lengths, x=None, x_lengths=None, xref=None, xref_lengths=None, max_steps: int = 0):
        defer = isinstance(self.encoder, Encoder2) and not self.training
        if defer:  # the encoder's id range check rides on the decoder's sync below instead of a sync of its own
            prev, self.encoder.defer_id_check = self.encoder.defer_id_check, True
        try:
            memory = self.encoder(cond, cond_lengths)
        finally:
            if defer:
                self.encoder.defer_id_check = prev
        kl_loss = torch.scalar_tensor(0)
        if xref is not None and self.refencoder is not None:
            style_embed, style_loss_dict = self.refencoder(xref, xref_lengths)
            memory = memory + style_embed
            if "kl" in style_loss_dict:
                kl_loss = style_loss_dict["kl"].mean()
        mmask = lengths_to_mask(cond_lengths)
        y, s, w = self.decoder(memory, mmask, x, max_steps, p_no_forcing=0.1)
        if defer:
            self.encoder.check_ids()  # (the decoder has just synchronised: the status word is there)
        y_post = self.postnet(y) if self.postnet else y
        return y, y_post, s, {"w": w, "kl_loss": kl_loss}

    def synthesize(self, cond, cond_lengths, xref=None, xref_lengths=None, max_steps: int = 0):
        """Batched synthesis: a batch of texts in, a ragged batch of spectrograms out, each utterance ending at its OWN stop
        token (``Decoder.forward_each``) and post-processed as if alone (the Postnet with lengths).  Inference only.
        Returns ``(y, y_post, s, {"w", "kl_loss", "lengths", "stopped"})``: y / y_post [B, T, D_mel], s [B, T, 1], w [B, T / r, L],
        all zero past each utterance's ``lengths[b]`` frames (int64 [B], on the device); ``stopped[b]`` is False for an
        utterance that reached the step cap without firing.  ``lengths`` is what ``synth_audio_native(y_post, frontend,
        lengths=lengths)`` takes."""
        defer = isinstance(self.encoder, Encoder2) and not self.training
        if defer:  # (as in forward: the id range check rides on the decoder's sync)
            prev, self.encoder.defer_id_check = self.encoder.defer_id_check, True
        try:
            memory = self.encoder(cond, cond_lengths)
        finally:
            if defer:
                self.encoder.defer_id_check = prev
        kl_loss = torch.scalar_tensor(0)
        if xref is not None and self.refencoder is not None:
            style_embed, style_loss_dict = self.refencoder(xref, xref_lengths)
            memory = memory + style_embed
            if "kl" in style_loss_dict:
                kl_loss = style_loss_dict["kl"].mean()
        mmask = lengths_to_mask(cond_lengths)
        y, s, w, lengths, stopped = self.decoder.forward_each(memory, mmask, max_steps)
        if defer:
            self.encoder.check_ids()
        y_post = self.postnet(y, lengths=lengths) if self.postnet else y
        return y, y_post, s.unsqueeze(2), {"w": w, "kl_loss": kl_loss, "lengths": lengths, "stopped": stopped}


# ---- the validation step: the loss terms of tacotron.py:59-138 and tacotron_lightning.py:50-99 on the HIP path ----
TERM_NAMES = ("mel", "mel_post", "dmel_all", "dmel_post_all", "dmel", "dmel_post", "stop", "w_std", "w_max", "N", "N1")  # terms[i] of ttsdec_val_losses
_INFERENCE_ONLY = "{} is inference only: call module.eval() and run it under torch.no_grad()"


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _fp32(owner: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{owner}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise NotImplementedError(f"the HIP {owner} is exact fp32: {name} must be torch.float32, got {t.dtype}")


def _on_device(owner: str, **tensors) -> torch.device:
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{owner}: {name} must live on a ROCm device (got {t.device}): this package has no CPU path")
    return next(iter(tensors.values())).device


def _mask_lengths(mask: torch.Tensor, B: int, T: int, owner: str) -> torch.Tensor:
    """lengths [B] int32 of the reference's [B, T, 1] mask of ones up to each utterance's length and zeros from there; ValueError for
    any other mask (the kernels take lengths).  One host read."""
    if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (B, T, 1):
        raise ValueError(f"{owner}: the mask must be [B, T, 1] = [{B}, {T}, 1], got {tuple(getattr(mask, 'shape', ()))}")
    m = mask[:, :, 0]
    t = (m != 0).sum(1)
    prefix = (torch.arange(T, device=mask.device)[None, :] < t[:, None]).to(m.dtype)
    if not bool(torch.equal(m, prefix)):
        raise ValueError(f"{owner}: the mask is not a prefix mask (ones up to each utterance's length, zeros from there)")
    return t.to(torch.int32).contiguous()


def _check_lengths(lengths, B: int, owner: str) -> torch.Tensor:
    lengths = torch.as_tensor(lengths)
    if tuple(lengths.shape) != (B,) or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
        raise ValueError(f"{owner}: lengths must be [B] = [{B}] integers, got {tuple(lengths.shape)} {lengths.dtype}")
    return lengths


def _lengths_on(lengths, B: int, device, owner: str) -> torch.Tensor:
    return _check_lengths(lengths, B, owner).to(device=device, dtype=torch.int32).contiguous()


def _engine(device):
    from .audio import _engine as weightless  # the weightless ttsdec handle of the stand-alone calls, one per device

    return weightless(device)


def mel_loss_fn(y, x, mask=None, order=1, *, lengths=None):
    """mel_loss_fn of the reference (tacotron.py:59-84): y [B, T, D], x [B, T_x >= T, D] (its first T frames count) fp32 on a ROCm
    device, mask None or the reference's [B, T, 1] prefix mask, order 0 / 1 / 2 -> a 0-dim tensor, in one pass of ttsdec_mel_loss.
    The one host read checks the mask; ``lengths=`` ([B] integers) in its place skips it.  An operand that requires grad (with grad
    enabled) takes the torch-op form of autograd_path instead."""
    if order not in (0, 1, 2):
        raise ValueError(f"mel_loss_fn: order must be 0, 1 or 2, got {order!r}")
    if mask is not None and lengths is not None:
        raise ValueError("mel_loss_fn: give mask or lengths, not both")
    if _wants_grad(y, x):
        from . import autograd_path

        if lengths is not None:
            mask = (torch.arange(y.shape[1], device=y.device)[None, :] < torch.as_tensor(lengths).to(y.device)[:, None]).unsqueeze(2).to(y.dtype)
        return autograd_path.mel_loss_fn(y, x[:, : y.shape[1]], mask, order)
    _fp32("mel_loss_fn", y=y, x=x)
    if y.dim() != 3 or x.dim() != 3 or y.shape[0] != x.shape[0] or y.shape[2] != x.shape[2] or x.shape[1] < y.shape[1] or not y.numel():
        raise ValueError(f"mel_loss_fn: y must be [B, T, D] and x [B, T_x >= T, D], got {tuple(y.shape)} and {tuple(x.shape)}")
    B, T, _ = y.shape
    if mask is not None:
        lengths = _mask_lengths(mask, B, T, "mel_loss_fn")
    elif lengths is not None:
        lengths = _check_lengths(lengths, B, "mel_loss_fn")
    dev = _on_device("mel_loss_fn", y=y, x=x)
    if lengths is not None:
        lengths = _lengths_on(lengths, B, dev, "mel_loss_fn")
    _, out = _engine(dev).mel_loss(y.detach().contiguous(), x.detach().contiguous(), lengths, order)
    return out[0]


def _alignment_terms(w, owner: str) -> torch.Tensor:
    _fp32(owner, w=w)
    if w.dim() != 3 or not w.numel():
        raise ValueError(f"{owner}: w must be [B, steps, L], got {tuple(w.shape)}")
    dev = _on_device(owner, w=w)
    return _engine(dev).val_losses(None, None, None, None, w.detach().contiguous(), None, shape=(w.shape[0], 1, 1))[1]


def alignment_max_loss(w):
    """alignment_max_loss of the reference (tacotron.py:87-89): w [B, steps, L] fp32 on a ROCm device -> mean(1 - max_l w)."""
    if _wants_grad(w):
        from . import autograd_path

        return autograd_path.alignment_max_loss(w)
    return _alignment_terms(w, "alignment_max_loss")[8]


def alignment_std_loss(w):
    """alignment_std_loss of the reference (tacotron.py:92-97): sqrt(mean(clip(var_l w, 0))) with var = sum w l^2 - (sum w l)^2,
    evaluated as sum w (l - m1)^2 + m1^2 (1 - sum w): the same quantity without that form's cancellation in fp32."""
    if _wants_grad(w):
        from . import autograd_path

        return autograd_path.alignment_std_loss(w)
    return _alignment_terms(w, "alignment_std_loss")[7]


def stop_loss(s, lengths, pos_weight=0.1):
    """The stop-token line of the reference (tacotron.py:120-123): binary_cross_entropy_with_logits(s, xmask, pos_weight) with
    s [B, T] or [B, T, 1] fp32 on a ROCm device and xmask the prefix mask of lengths [B]."""
    if _wants_grad(s):
        from . import autograd_path

        return autograd_path.stop_loss(s, torch.as_tensor(lengths), pos_weight)
    _fp32("stop_loss", s=s)
    if s.dim() not in (2, 3) or (s.dim() == 3 and s.shape[2] != 1) or not s.numel():
        raise ValueError(f"stop_loss: s must be [B, T] or [B, T, 1], got {tuple(s.shape)}")
    B, T = s.shape[:2]
    lengths = _check_lengths(lengths, B, "stop_loss")
    dev = _on_device("stop_loss", s=s)
    lengths = _lengths_on(lengths, B, dev, "stop_loss")
    return _engine(dev).val_losses(None, None, None, s.detach().reshape(B, T).contiguous(), None, lengths, pos_weight, shape=(B, T, 1))[1][6]


def validation_terms(model, c, c_lengths, x, x_lengths, xref=None, xref_lengths=None):
    """The forward of a validation step and every loss term the reference's loops log, in one call of ttsdec_val_losses on the
    forward's outputs: ``model(c, c_lengths, x, x_lengths, xref=..., xref_lengths=...)`` in eval mode under no_grad, then the terms
    from y, y_post, s and out["w"] against the first T = y.shape[1] frames of x (by index: no x[:, :T] copy) and x_lengths.
    Returns (terms, y, y_post, s, out): terms [16] fp32 on the device, named by TERM_NAMES (include/ttsdec.h ttsdec_val_losses).
    Enqueues only beyond what the forward itself reads back."""
    if model.training:
        raise RuntimeError(_INFERENCE_ONLY.format("validation_terms"))
    _fp32("validation_terms", x=x)
    if x.dim() != 3:
        raise ValueError(f"validation_terms: x must be [B, T_x, num_mels], got {tuple(x.shape)}")
    dev = _on_device("validation_terms", x=x, c=c)
    with torch.no_grad():
        lengths = _lengths_on(x_lengths, x.shape[0], dev, "validation_terms")
        y, y_post, s, out = model(c, c_lengths, x, x_lengths, xref=xref, xref_lengths=xref_lengths)
        B, T, _ = y.shape
        _, terms = _engine(dev).val_losses(y.contiguous(), y_post.contiguous(), x.contiguous(), s.reshape(B, T).contiguous(),
                                           out["w"].contiguous(), lengths, 0.1)
    return terms, y, y_post, s, out


def _step_numbers(terms, kl, loss):
    """One host read: the terms, the KL and the total as Python floats."""
    host = torch.cat([terms, kl.reshape(1).to(device=terms.device, dtype=terms.dtype), loss.reshape(1)]).tolist()
    return host[:-2], host[-2], host[-1]


def run_validation_step(model, batch, device):
    """run_training_step of the reference (tacotron.py:100-138) for a model in eval mode, without autograd: the same batch
    (c, c_lengths, x, x_lengths), the same weights and the same keys -> (loss, dict); loss is a 0-dim tensor on the device, the
    dict's floats come from one host read."""
    c, c_lengths, x, x_lengths = [t.to(device) for t in batch if isinstance(t, torch.Tensor)]
    terms, _, _, _, out = validation_terms(model, c, c_lengths, x, x_lengths, xref=x, xref_lengths=x_lengths)
    kl = out["kl_loss"].to(terms.device)
    loss_mel, loss_mel_post = terms[0] + terms[2], terms[1] + terms[3]
    loss = 0.8 * loss_mel + 0.2 * loss_mel_post + 0.1 * terms[6] + 0.0002 * kl + 0.0001 * terms[7]
    t, kl_f, _ = _step_numbers(torch.cat([terms, loss_mel.reshape(1), loss_mel_post.reshape(1)]), kl, loss)
    return loss, {"loss_mel_db": 100 * t[16], "loss_mel_post_db": 100 * t[17], "loss_stop": t[6], "loss_kl": kl_f, "loss_w": t[7],
                  "w": out["w"].detach().cpu()}


def task_forward(model, batch, extra_loss=False):
    """TacotronTask.train_forward of the reference (tacotron_lightning.py:50-99) for a model in eval mode, without autograd: batch
    is its five-tuple (_, c, c_lengths, x, x_lengths) -> (loss, log_dict, img_dict) with its weights and keys, the masked dmel terms
    and the alignment term included when extra_loss is set."""
    _, c, c_lengths, x, x_lengths = batch
    terms, _, y_post, _, out = validation_terms(model, c, c_lengths, x, x_lengths, xref=x, xref_lengths=x_lengths)
    kl = out["kl_loss"].to(terms.device)
    loss = 0.8 * terms[0] + 0.2 * terms[1] + 0.1 * terms[6] + 0.0002 * kl
    if extra_loss:
        loss = loss + 0.0001 * terms[7] + 0.4 * terms[4] + 0.1 * terms[5]
    t, kl_f, total = _step_numbers(terms, kl, loss)
    return (loss, {"total": total, "mel_db": 100 * t[0], "mel_post_db": 100 * t[1], "stop": t[6], "kl": kl_f, "w": t[7]},
            {"w": out["w"].detach().cpu(), "y_post": y_post.detach().cpu()})


def build_tacotron(config):
    """config dict -> Tacotron, as tacotron.py:165-224 for the LJSpeech-style configs
    (decoder type other than tacotron1/tacotron2 -> Taco2ProdDecoderCell; postnet type
    "tacotron2" -> MelPostnet)."""
    text_config, audio_config = config["text"], config["audio"]
    decoder_config, encoder_config = config["model"]["decoder"], config["model"]["encoder"]
    if decoder_config["type"] == "tacotron1":
        raise NotImplementedError("Taco1DecoderCell is dead code in the reference (SURVEY.md section 2) and is not provided")
    decoder_cell_class = Taco2DecoderCell if decoder_config["type"] == "tacotron2" else Taco2ProdDecoderCell
    decoder_cell = decoder_cell_class(
        encoder_config["dim_out"], audio_config["num_mels"], r=decoder_config["r"], dim_rnn=decoder_config["dim_rnn"],
        dim_pre=decoder_config["dim_pre"], dim_att=decoder_config["dim_att"],
    )
    decoder = Decoder(decoder_cell, decoder_config["r"], audio_config["num_mels"])
    alphabet_size = 1 + len(text_config["alphabet"])
    if "phonemes" in text_config:
        alphabet_size += len(text_config["phonemes"])
    encoder = Encoder2(alphabet_size, dim_out=encoder_config["dim_out"], dim_emb=encoder_config["dim_emb"])
    postnet_config = config["model"].get("postnet")
    postnet = None
    if postnet_config:
        if postnet_config.get("type") == "tacotron2":
            postnet = MelPostnet(audio_config["num_mels"], dim_hidden=postnet_config["dim_hidden"], num_layers=postnet_config["num_layers"])
        else:
            postnet = MelPostnet2(audio_config["num_mels"], dim_hidden=postnet_config["dim_hidden"], num_layers=postnet_config["num_layers"])
    style_encoder_config = config["model"].get("style_encoder")
    refencoder = None
    if style_encoder_config:  # tacotron.py:216-220
        refencoder = VAE(num_mels=audio_config["num_mels"], dim_vae=style_encoder_config["dim_vae"])
    return Tacotron(encoder, decoder, postnet=postnet, refencoder=refencoder)
