"""MI355X-native drop-in for the Tacotron decoder hot path of kgoba/torch-tts.

Import as ``torch_tts_amd`` (the directory name ``torch-tts_amd`` is not a Python
identifier; the sibling ``torch_tts_amd/`` package aliases it)."""
from . import _lib  # noqa: F401
from .decoder import Decoder
from .decoder_cell import LSTMZoneoutCell, PreNet, StepwiseMonotonicAttention, Taco2DecoderCell, Taco2ProdDecoderCell
from .engine import Engine, EngineDims
from .postnet import Conv1dFix, MelPostnet, MelPostnet2
from .style import GST, GST_VAE, STL, VAE, MultiHeadAttention, ReferenceEncoder, StyleEngine
from .tacotron import (Encoder2, Tacotron, alignment_max_loss, alignment_std_loss, build_tacotron, lengths_to_mask, mel_loss_fn,
                       run_validation_step, stop_loss, task_forward, validation_terms)
from . import vits2  # noqa: F401  (TextEncoder, ResidualCouplingTransformersBlock, Generator, StochasticDurationPredictor, DurationPredictor, infer,
#                             PosteriorEncoder, voice_conversion, forced_alignment, duration_loss, synthesizer_forward, validation_losses,
#                             kl_loss, slice_segments, rand_slice_segments)
from .vits2 import (DiscriminatorP, DiscriminatorS, DurationDiscriminatorV1, DurationDiscriminatorV2, DurationPredictor, Generator,
                    MultiPeriodDiscriminator, PosteriorEncoder, StochasticDurationPredictor)
from . import audio  # noqa: F401  (AudioFrontend.mel_inv / decode, m_rev, synth_audio)
from . import mel_processing  # noqa: F401  (spectrogram_torch, spec_to_mel_torch, mel_spectrogram_torch: the VITS2 audio front-end)
from . import train_util  # noqa: F401  (load_state_dict: the reference's partial checkpoint loader + blob invalidation)

__all__ = [
    "Decoder", "Taco2ProdDecoderCell", "Taco2DecoderCell", "PreNet", "LSTMZoneoutCell", "StepwiseMonotonicAttention", "MelPostnet", "MelPostnet2",
    "Tacotron", "Encoder2", "build_tacotron", "lengths_to_mask", "Engine", "EngineDims",
    "Generator", "StochasticDurationPredictor", "DurationPredictor", "PosteriorEncoder",
    "DiscriminatorS", "DiscriminatorP", "MultiPeriodDiscriminator", "DurationDiscriminatorV1", "DurationDiscriminatorV2",
    "ReferenceEncoder", "STL", "GST", "VAE", "GST_VAE", "MultiHeadAttention", "StyleEngine",
    "mel_loss_fn", "alignment_max_loss", "alignment_std_loss", "stop_loss", "validation_terms", "run_validation_step", "task_forward",
]
