"""Host-side checks of the VITS2 spectrogram front-end (vits2/mel_processing.py:58-187): the torch-CPU restatement that the GPU
tests (tests/test_spec_hip.py) lean on is pinned here against the reference's own results (tests/golden/make_golden_spec.py: every
utterance run alone through the reference in fp32 and in fp64); plus the frame-count arithmetic, the C-ABI exports and their
host-only refusals, and the refusals of the Python entry points.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "spec_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "spec_meta.json")))
    return {k: z[k] for k in z.files}, meta


# ---------------------------------------------------------------------------------------------------------------------------
# restatement: the reference's lines on torch ops, one utterance at a time (the reflection is at the utterance's own ends)
# ---------------------------------------------------------------------------------------------------------------------------
def spectrogram_one(y, n_fft, hop, win):
    """mel_processing.py:58-106 on one utterance y [n] (fp32 or fp64, any device) -> [n_fft / 2 + 1, T]."""
    window = torch.hann_window(win).to(dtype=y.dtype, device=y.device)
    pad = int((n_fft - hop) / 2)
    yp = torch.nn.functional.pad(y[None, None], (pad, pad), mode="reflect")[0]
    s = torch.stft(yp, n_fft, hop_length=hop, win_length=win, window=window, center=False, pad_mode="reflect", normalized=False, onesided=True,
                   return_complex=True)
    s = torch.view_as_real(s)
    return torch.sqrt(s.pow(2).sum(-1) + 1e-6)[0]


def spec_to_mel_one(spec, basis):
    """mel_processing.py:109-122 with the basis given: log(clamp(basis @ spec, 1e-5))."""
    return torch.log(torch.clamp(torch.matmul(basis.to(spec.dtype), spec), min=1e-5))


def spectrogram_batch(y, lengths, n_fft, hop, win, basis=None):
    """A padded batch y [B, N] with lengths -> ([B, rows, T] with zeros past each utterance's frames, frame counts), T from N."""
    from torch_tts_amd.mel_processing import frame_count

    B, N = y.shape
    rows = n_fft // 2 + 1 if basis is None else basis.shape[0]
    out = torch.zeros(B, rows, frame_count(N, n_fft, hop), dtype=y.dtype, device=y.device)
    counts = []
    for b in range(B):
        s = spectrogram_one(y[b, : int(lengths[b])], n_fft, hop, win)
        if basis is not None:
            s = spec_to_mel_one(s, basis)
        out[b, :, : s.shape[1]] = s
        counts.append(s.shape[1])
    return out, counts


def frame_err(s, s64):
    """max over frames of max_bins |s - s64| / max_bins s64: [bins, T] each."""
    return float(((s.double() - s64).abs().amax(0) / s64.amax(0)).max())


def golden_batch(sd, c, ci):
    """The three utterances of configuration ci as a zero-padded batch [3, max len] and their lengths."""
    y = torch.zeros(3, max(c["lengths"]))
    for ui, n in enumerate(c["lengths"]):
        y[ui, :n] = torch.from_numpy(sd[f"c{ci}/u{ui}/wav"])
    return y, list(c["lengths"])


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference():
    sd, meta = load_golden()
    assert len(meta["configs"]) == 3
    for ci, c in enumerate(meta["configs"]):
        basis = torch.from_numpy(sd[f"basis/{c['n_fft']}"])
        for ui, n in enumerate(c["lengths"]):
            y = torch.from_numpy(sd[f"c{ci}/u{ui}/wav"])
            assert y.numel() == n and n % c["hop"] != 0
            t = lambda k: torch.from_numpy(sd[f"c{ci}/u{ui}/{k}"])  # noqa: E731
            s32 = spectrogram_one(y, c["n_fft"], c["hop"], c["win"])
            assert s32.shape == t("spec32").shape
            assert torch.allclose(s32, t("spec32"), rtol=1e-6)  # (the same library calls on the same input: equal, or an ulp apart)
            assert torch.allclose(spec_to_mel_one(s32, basis), t("mel32"), rtol=1e-6)
            s64 = spectrogram_one(y.double(), c["n_fft"], c["hop"], c["win"])
            assert float((s64 - t("spec64")).abs().max()) <= 1e-12 * max(1.0, float(t("spec64").max()))
            assert float((spec_to_mel_one(s64, basis) - t("mel64")).abs().max()) <= 1e-12 * 12
        # what fp32 can be expected to give: sets the GPU test's bar
        assert 5e-8 < c["spec_frame_err"] < 1e-6 and c["mel_tol_ratio"] <= 1.0, c


def test_golden_signals_reach_the_floor_and_the_quiet_end_of_the_log():
    sd, meta = load_golden()
    for ci in range(3):
        assert float(sd[f"c{ci}/u2/spec64"].min()) < 1.01e-3  # sqrt(1e-6): the ramp's first frames
        assert float(sd[f"c{ci}/u2/mel64"].min()) < -8.0 and float(sd[f"c{ci}/u1/mel64"].max()) > -2.0


def test_frame_count_arithmetic():
    from torch_tts_amd.mel_processing import frame_count, pad_of

    for n_fft, hop, win in ((1024, 256, 1024), (256, 64, 256), (1024, 256, 800), (512, 127, 512), (256, 255, 200), (256, 256, 256), (256, 1, 256)):
        pad = pad_of(n_fft, hop)
        assert pad == (n_fft - hop) // 2
        for n in (pad + 1, pad + 2, n_fft, n_fft + hop - 1, n_fft + hop, 3 * n_fft + 17):
            want = 0
            if n + 2 * pad >= n_fft:
                want = spectrogram_one(torch.zeros(n), n_fft, hop, win).shape[1]
            assert frame_count(n, n_fft, hop) == want, (n_fft, hop, n)
            assert want == 0 or want == 1 + (n + 2 * pad - n_fft) // hop
        assert frame_count(pad, n_fft, hop) == 0  # the reflection is undefined (torch raises too)
        if pad > 0:
            with pytest.raises(RuntimeError):
                spectrogram_one(torch.zeros(pad), n_fft, hop, win)
    _, meta = load_golden()
    for c in meta["configs"]:
        assert [frame_count(n, c["n_fft"], c["hop"]) for n in c["lengths"]] == [1 + (n + 2 * pad_of(c["n_fft"], c["hop"]) - c["n_fft"]) // c["hop"]
                                                                               for n in c["lengths"]]


def test_new_ttsvits_symbols_are_declared_bound_and_exported():
    import torch_tts_amd as T
    from torch_tts_amd import _lib

    new = ("ttsvits_spec_workspace_bytes", "ttsvits_spectrogram", "ttsvits_spec_to_mel", "ttsvits_mel_spectrogram")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttsdec.h")).read(), flags=re.S)
    lib = _lib.load()
    for sym in new:
        assert re.search(rf"\b{sym}\s*\(", hdr), sym
        assert sym in _lib.FAMILY_SYMBOLS["ttsvits"] and hasattr(lib, sym), sym
    assert lib.ttsdec_version() == 2 and len(_lib.FAMILIES) == 6
    eng = T.vits2.VitsEngine(T.vits2._ALIGN_DIMS, None)
    h = eng._h
    assert lib.ttsvits_spec_workspace_bytes(h, 1024, 0) == 8192 and lib.ttsvits_spec_workspace_bytes(h, 1024, 80) == 8192 + 768
    assert lib.ttsvits_spec_workspace_bytes(h, 1000, 0) == 0 and lib.ttsvits_spec_workspace_bytes(h, 4096, 0) == 0
    assert lib.ttsvits_spec_workspace_bytes(h, 128, 0) == 0 and lib.ttsvits_spec_workspace_bytes(h, 1024, 257) == 0
    one = 256  # (non-null placeholders: the size checks come first)
    big = 1 << 20
    spec = lambda B, N, n_fft, ws=big: lib.ttsvits_spectrogram(h, one, None, B, N, one, n_fft, 256, n_fft, one, 4, None, one, ws, None)  # noqa: E731
    mel = lambda B, N, n_fft, ws=big: lib.ttsvits_mel_spectrogram(h, one, None, B, N, one, n_fft, 256, n_fft, one, 80, one, 4, None, one, ws, None)  # noqa: E731
    for call in (spec, mel):
        assert call(1, 4000, 1000) == _lib.ERR_DIMS and call(1, 4000, 4096) == _lib.ERR_DIMS
        assert call(0, 4000, 1024) == _lib.ERR_INVALID_ARG and call(1, 0, 1024) == _lib.ERR_INVALID_ARG and call(-1, 4000, 1024) == _lib.ERR_INVALID_ARG
        assert call(1, 4000, 1024, 64) == _lib.ERR_WORKSPACE
    assert lib.ttsvits_spectrogram(h, one, None, 1, 4000, one, 1024, 256, 1025, one, 4, None, one, big, None) == _lib.ERR_DIMS  # win_size > n_fft
    assert lib.ttsvits_spectrogram(h, one, None, 1, 4000, one, 1024, 0, 1024, one, 4, None, one, big, None) == _lib.ERR_INVALID_ARG  # hop_size 0
    assert lib.ttsvits_spec_to_mel(h, one, None, 1, 1000, 4, one, 80, one, one, big, None) == _lib.ERR_DIMS
    assert lib.ttsvits_spec_to_mel(h, one, None, 0, 1024, 4, one, 80, one, one, big, None) == _lib.ERR_INVALID_ARG
    assert lib.ttsvits_spec_to_mel(h, one, None, 1, 1024, 4, one, 80, one, one, 8192, None) == _lib.ERR_WORKSPACE
    eng.close()


def test_entry_points_refuse_what_is_not_on_the_path():
    import torch_tts_amd as T
    from torch_tts_amd import mel_processing as MP

    V = T.vits2
    assert V.spectrogram_torch is MP.spectrogram_torch and V.mel_spectrogram_torch is MP.mel_spectrogram_torch
    assert V.spec_to_mel_torch is MP.spec_to_mel_torch
    y = torch.zeros(2, 4000)
    with pytest.raises(NotImplementedError):  # CPU tensors: no fallback
        MP.spectrogram_torch(y, 1024, 22050, 256, 1024)
    with pytest.raises(NotImplementedError):
        MP.mel_spectrogram_torch(y, 1024, 80, 22050, 256, 1024, 0, None)
    with pytest.raises(NotImplementedError):
        MP.spec_to_mel_torch(torch.zeros(1, 513, 4), 1024, 80, 22050, 0, None)
    with pytest.raises(NotImplementedError, match="center"):
        MP.spectrogram_torch(y, 1024, 22050, 256, 1024, center=True)
    with pytest.raises(NotImplementedError, match="center"):
        MP.mel_spectrogram_torch(y, 1024, 80, 22050, 256, 1024, 0, None, True)
    with pytest.raises(NotImplementedError):  # fp64
        MP.spectrogram_torch(y.double(), 1024, 22050, 256, 1024)

    class Net(nn.Module):
        def __init__(self, ch):
            super().__init__()
            self.enc_q = V.PosteriorEncoder(ch, 8, 8, 5, 1, 2, gin_channels=4)

    kw = dict(n_fft=1024, hop_size=256, win_size=1024, sampling_rate=22050)
    with pytest.raises(ValueError, match="77"):
        V.voice_conversion_from_audio(Net(77), y, [4000, 3000], None, None, n_mels=80, **kw)
    with pytest.raises(ValueError, match="80"):
        V.forced_alignment_from_audio(Net(80), None, None, y, [4000, 3000], **kw)  # a mel model and no n_mels
    with pytest.raises(TypeError, match="enc_q"):
        V.voice_conversion_from_audio(nn.Module(), y, [4000, 3000], None, None, **kw)
    with pytest.raises(NotImplementedError):  # the right channels, CPU tensors
        V.voice_conversion_from_audio(Net(513), y, [4000, 3000], None, None, **kw)
    with pytest.raises(NotImplementedError):
        V.forced_alignment_from_audio(Net(80), None, None, y, [4000, 3000], n_mels=80, **kw)
