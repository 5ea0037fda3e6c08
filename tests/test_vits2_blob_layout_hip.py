"""The packed VITS2 blobs do not move: ttsvits_pack_weights (text encoder + flow) and ttspost_pack_weights (posterior encoder) on
fixed weights give the bytes they gave when tests/golden/vits2_blob_sha256.json was recorded - every GEMM weight as fp32 | hi | lo,
q / k / v stacked, conv weights tap-major, the vectors, each at its offset.

Weights are test_blob_layout_hip.hashed (closed form, no RNG stream).  The tensor sizes and their order are written out below from
include/ttsdec.h, independently of the library's own layout walk.  The recorded hashes were taken on an MI355X from the library of
commit cfc45a4 ("Decoder blob: one matrix record ..."), the parent of the commit that introduced the weight records of
csrc/vits2.hip:

    TTSDEC_LIB=<that build's libttsdec.so> python tests/test_vits2_blob_layout_hip.py      prints the JSON"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# name -> (family_dims key, which sources are given: None = all, "text" / "flow" = the others are NULL)
CASES = {"vits_small": ("vits_small", None), "vits_small_g": ("vits_small_g", None), "vits_small_text_only": ("vits_small", "text"),
         "vits_small_flow_only": ("vits_small", "flow"), "post_small": ("post_small", None), "post_small_g": ("post_small_g", None)}


def stack_sizes(C_, F, heads, layers, k, window):
    """one attentions.Encoder: per layer conv_{q,k,v,o}.{weight,bias}, (emb_rel_k, emb_rel_v,) norm 1, the FFN convs, norm 2"""
    rel = [(2 * window + 1) * (C_ // heads)] * 2 if window >= 0 else []
    return (4 * [C_ * C_, C_] + rel + [C_, C_, F * C_ * k, F, C_ * F * k, C_, C_, C_]) * layers


def wn_sizes(H, k, layers, gin):
    """modules.WN: (cond_layer,) per layer in_layers.j, res_skip_layers.j (the last one H rows instead of 2 H)"""
    out = [2 * H * layers * gin, 2 * H * layers] if gin else []
    for j in range(layers):
        cr = 2 * H if j < layers - 1 else H
        out += [2 * H * H * k, 2 * H, cr * H, cr]
    return out


def weight_sizes(fam, d):
    """-> ([elements per source tensor] in the family's pack order (include/ttsdec.h), number of them that are the text encoder's)"""
    if fam == "ttspost":
        S, I, H = d.spec_channels, d.inter_channels, d.hidden_channels
        return [H * S, H] + wn_sizes(H, d.kernel_size, d.n_layers, d.gin_channels) + [2 * I * H, 2 * I], 0
    H, I, gin = d.hidden_channels, d.inter_channels, d.gin_channels
    text = [d.n_vocab * H] + ([H * gin, H] if gin else [])
    text += stack_sizes(H, d.filter_channels, d.n_heads, d.n_layers, d.kernel_size, d.window_size) + [2 * I * H, 2 * I]
    half, Fh = I // 2, d.flow_hidden
    flow = []
    for _ in range(d.n_flows):
        flow += stack_sizes(half, half, d.flow_tf_heads, d.flow_tf_layers, d.flow_tf_kernel, -1) + [Fh * half, Fh]
        flow += wn_sizes(Fh, d.flow_kernel, d.flow_wn_layers, gin) + [half * Fh, half]
    return text + flow, len(text)


def pack(name):
    """-> (blob bytes, the dims)"""
    import torch

    from test_blob_layout_hip import hashed
    from test_layout_host import family_dims
    from torch_tts_amd import _lib

    key, only = CASES[name]
    fam, d = family_dims(_lib)[key]
    lib, h = _lib.load(), C.c_void_p()
    fn = lambda what: getattr(lib, f"{fam}_{what}")
    assert fn("create")(C.byref(d), C.byref(h)) == _lib.OK
    try:
        sizes, n_text = weight_sizes(fam, d)
        assert fn("num_weight_tensors")(h) == len(sizes)
        given = [only is None or (i < n_text) == (only == "text") for i in range(len(sizes))]
        dev = [torch.from_numpy(hashed(n, i)).to("cuda:0") if g else None for i, (n, g) in enumerate(zip(sizes, given))]
        arr = (C.c_void_p * len(dev))(*[t.data_ptr() if t is not None else None for t in dev])
        blob = torch.empty(fn("packed_bytes")(h), dtype=torch.uint8, device="cuda:0")
        assert blob.data_ptr() % 256 == 0
        rc = fn("pack_weights")(h, arr, len(dev), blob.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.OK, rc
        torch.cuda.synchronize()
        return blob.cpu().numpy().tobytes(), d
    finally:
        fn("destroy")(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_packed_blob_is_the_recorded_one(name):
    recorded = json.load(open(os.path.join(HERE, "golden", "vits2_blob_sha256.json")))
    blob, d = pack(name)
    got = hashlib.sha256(blob).hexdigest()
    print(name, len(blob), got)
    assert len(blob) == recorded[name]["bytes"]
    assert got == recorded[name]["sha256"]
    if name.startswith("post"):
        # pre.weight leads the blob as [hidden, spec rounded up to 8] fp32 | hi | lo: the padding columns are zero in all three
        H, S = d.hidden_channels, d.spec_channels
        Sp = (S + 7) // 8 * 8
        w = np.frombuffer(blob[:4 * H * Sp], dtype=np.float32).reshape(H, Sp)
        planes = np.frombuffer(blob[4 * H * Sp:8 * H * Sp], dtype=np.float16).reshape(2, H, Sp)
        assert np.abs(w[:, :S]).max() > 0 and np.abs(planes[0][:, :S]).max() > 0
        assert not w[:, S:].any() and not planes[:, :, S:].any()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    out = {}
    for name in CASES:
        blob = pack(name)[0]
        out[name] = {"bytes": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}
    print(json.dumps(out, indent=1))
