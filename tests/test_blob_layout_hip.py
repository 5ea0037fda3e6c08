"""The packed decoder blob does not move: ttsdec_pack_weights on fixed weights gives the bytes it gave when
tests/golden/decoder_blob_sha256.json was recorded - every stored form of every matrix (fp32, split-fp16 hi / lo, bf16, frame-order
and chunked planes), the folded BatchNorms and the range-guard header, each at its offset.

The weights are a closed-form integer hash of the element index (no RNG stream to drift), in [-0.5, 0.5) - far inside the fp16
range - with BatchNorm variances in [0.5, 1.5).  The recorded hashes were taken on an MI355X from the library of commit ed25182
("Add audio resampling on HIP"), the parent of the commit that introduced the matrix records of csrc/api.hip:

    TTSDEC_LIB=<that build's libttsdec.so> python tests/test_blob_layout_hip.py      prints the JSON"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ("dec_small_mel", "dec_small_mel2", "dec_chunked")


def case_dims(_lib, name):
    """dec_small_mel: Prod cell + MelPostnet, no frame kernel, no chunked planes; dec_small_mel2: Taco2 cell + MelPostnet2 with
    d_pre_hidden (frame-order planes); dec_chunked: the smallest dims of the chunked planes (csrc/api.hip chunk_ok) - the frame
    kernel's d_mel = 80, r = 1 and PreNet 128 -> 32, every K segment one 32-element chunk - with one Postnet layer of width 8."""
    if name == "dec_chunked":
        return _lib.Dims(80, 1, 32, 32, 32, 32, 0.1, 0.5, 1, 8, 5, 1e-5, _lib.CELL_TACO2PROD, 128, _lib.POSTNET_TYPE_MEL)
    from test_layout_host import family_dims

    return family_dims(_lib)[name][1]


def hashed(n, salt, positive=False):
    """n floats, element i a fixed function of (i, salt): multiples of 2^-16 in [-0.5, 0.5), or in [0.5, 1.5) (variances)."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt + 1) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    v = (x & np.uint64(0xFFFF)).astype(np.float32) / np.float32(65536.0)
    return v + np.float32(0.5) if positive else v - np.float32(0.5)


def weight_sizes(_lib, d):
    """-> [(elements, is a BatchNorm variance, feeds wmax[0] / wmax[1] / neither)] in ttsdec_pack_weights' order (include/ttsdec.h)."""
    taco2 = d.cell_type == _lib.CELL_TACO2
    Mel, R, P, D, Ha, Hd = d.d_mel, d.r, d.d_pre, d.d_ctx, d.h_att, d.h_dec
    Ph = d.d_pre_hidden or P
    q_ld = Ha + Hd + D if taco2 else Ha
    p_ld = Ha + Hd + D if taco2 else Hd + D
    dec = [Ph * Mel, -Ph, P * Ph, -P, D * q_ld, 4 * Ha * (P + D), 4 * Ha * Ha, -4 * Ha, -4 * Ha, 4 * Hd * (Ha + D), 4 * Hd * Hd, -4 * Hd,
           -4 * Hd, -Ha, -Hd, -Ha, -Hd, R * Mel * p_ld, -R * Mel, R * p_ld, -R]  # (negative: a vector - no planes, not in the range guard)
    out = [(abs(n), False, 0 if n > 0 else None) for n in dec]
    Hh, k = d.postnet_hidden, d.postnet_kernel
    bn = [(Hh, False, None)] * 3 + [(Hh, True, None)]  # weight, bias, running_mean, running_var
    if d.postnet_type == _lib.POSTNET_TYPE_MEL2:
        for _ in range(d.postnet_layers):
            out += [(Hh * Mel * k, False, 1)] + bn + [(Hh * Hh * k, False, 1)] + bn + [(Mel * Hh * k, False, 1)]
    else:
        cin = Mel
        for _ in range(d.postnet_layers):
            out += [(Hh * cin * k, False, 1)] + bn
            cin = Hh
        out += [(Mel * Hh, False, 1)]
    return out


def pack(name):
    """-> (blob bytes, the two maxima the range-guard header must hold, ttsdec_get_precision in split-fp16 mode, the dims)"""
    import torch

    from torch_tts_amd import _lib

    lib, d, h = _lib.load(), case_dims(_lib, name), C.c_void_p()
    assert lib.ttsdec_create(C.byref(d), C.byref(h)) == _lib.OK
    try:
        sizes = weight_sizes(_lib, d)
        assert lib.ttsdec_num_weight_tensors(h) == len(sizes)
        host = [hashed(n, i, positive=var) for i, (n, var, _) in enumerate(sizes)]
        wmax = [max(float(np.abs(w).max()) for w, s in zip(host, sizes) if s[2] == g) for g in (0, 1)]
        dev = [torch.from_numpy(w).to("cuda:0") for w in host]
        arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        blob = torch.empty(lib.ttsdec_packed_bytes(h), dtype=torch.uint8, device="cuda:0")
        assert blob.data_ptr() % 256 == 0
        rc = lib.ttsdec_pack_weights(h, arr, len(dev), blob.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.OK, rc
        torch.cuda.synchronize()
        assert lib.ttsdec_set_precision(h, _lib.PREC_SPLIT_F16) == _lib.OK
        return blob.cpu().numpy().tobytes(), wmax, lib.ttsdec_get_precision(h), d
    finally:
        lib.ttsdec_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_packed_blob_is_the_recorded_one(name):
    from torch_tts_amd import _lib

    recorded = json.load(open(os.path.join(HERE, "golden", "decoder_blob_sha256.json")))
    blob, wmax, precision, d = pack(name)
    got = hashlib.sha256(blob).hexdigest()
    print(name, len(blob), got)
    assert len(blob) == recorded[name]["bytes"]
    assert got == recorded[name]["sha256"]
    # the header: max |w| over the decoder's matrices, then over the Postnet's (a maximum has no rounding: exact)
    assert np.frombuffer(blob[:8], dtype=np.float32).tolist() == wmax
    # ... as read back by the pack call: split-fp16 wherever every K segment is whole 8-element columns (the maxima are in range)
    split_ok = not (d.d_pre | d.d_ctx | d.h_att | d.h_dec) & 7
    assert precision == (_lib.PREC_SPLIT_F16 if split_ok else _lib.PREC_F32)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    out = {}
    for name in CASES:
        blob = pack(name)[0]
        out[name] = {"bytes": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}
    print(json.dumps(out, indent=1))
