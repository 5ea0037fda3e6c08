"""The packed generator and duration-predictor blobs do not move: ttsgen_pack_weights, ttsdur_pack_weights and
ttsvits_durnll_pack_weights on fixed weights give the bytes they gave when tests/golden/gen_dur_blob_sha256.json was recorded - conv
weights tap-major, the transposed convs as their
polyphase 3-tap weight with the bias once per phase, the duration convs K-major, the vectors, each at its offset - and so do the
split-fp16 weight planes that ttsvits_generator_pack_planes makes from the bound blob, in a buffer zeroed first (the alignment gaps are
never written), also where only some layers have planes.

Weights are test_blob_layout_hip.hashed (closed form, no RNG stream).  The tensor sizes and their order are written out below from
include/ttsdec.h, independently of the library's own layout walk.  The recorded hashes were taken on an MI355X from the library of
commit 293bf2f ("Add the VITS2 duration discriminators on HIP: V1 and V2 probabilities"), the parent of the commit that introduced
the weight records of csrc/generator.hip and csrc/duration.hip; the durnll rows from the library of commit e4aad43 ("Add the VITS2
duration likelihood on HIP: SDP forward, l_length, VL/dur"), where the likelihood handle still had a record struct of its own:

    TTSDEC_LIB=<that build's libttsdec.so> python tests/test_gen_dur_blob_layout_hip.py      prints the JSON"""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PACKED = ("gen_small", "gen_small_g", "sdp_small", "sdp_small_g", "dp_small", "dp_small_g", "durnll_small",
          "durnll_small_g")  # test_layout_host.family_dims keys
# the planes buffer: every layer split; then the two mixed handles of test_generator_split_host (conv_pre and the resblocks exact: only
# ups[0] has planes; one dilation keeps the stage exact: conv_pre and ups[0] have planes)
PLANES = {"planes_gen_small": None, "planes_mixed_12_24": dict(initial=12, c0=24, rates=(2,), dil=(1, 1, 1)),
          "planes_mixed_8_192": dict(initial=8, c0=192, rates=(2,), dil=(1, 3, 1))}


def gen_sizes(d):
    """elements per source tensor of ttsgen_pack_weights, in its order (include/ttsdec.h)"""
    C0 = d.upsample_initial_channel
    chans = [C0 >> (i + 1) for i in range(d.n_up)]
    out = [C0 * d.initial_channel * 7, C0]
    for i, c in enumerate(chans):
        out += [(C0 if i == 0 else chans[i - 1]) * c * d.up_kernels[i], c]
    for c in chans:
        for j in range(d.n_res):
            out += [c * c * d.res_kernels[j], c] * 6
    out += [chans[-1] * 7]
    return out + ([C0 * d.gin_channels, C0] if d.gin_channels else [])


def dur_sizes(_lib, d):
    """elements per source tensor of ttsdur_pack_weights, in its order (include/ttsdec.h)"""
    Cc, F = d.in_channels, d.filter_channels
    dds = [Cc * 3, Cc, Cc * Cc, Cc, Cc, Cc, Cc, Cc] * 3
    if d.kind == _lib.DUR_SDP:
        out = [Cc * Cc, Cc] + dds + [Cc * Cc, Cc, 2, 2]
        for _ in range(d.n_flows - 1):
            out += [Cc, Cc] + dds + [29 * Cc, 29]
    else:
        out = [F * Cc * 3, F, F, F, F * F * 3, F, F, F, F, 1]
    return out + ([Cc * d.gin_channels, Cc] if d.gin_channels else [])


def durnll_sizes(d):
    """elements per source tensor of ttsvits_durnll_pack_weights, in its order (include/ttsdec.h)"""
    Cc = d.in_channels
    dds = [Cc * 3, Cc, Cc * Cc, Cc, Cc, Cc, Cc, Cc] * 3
    flow = [Cc, Cc] + dds + [29 * Cc, 29]
    out = [Cc * Cc, Cc] + dds + [Cc * Cc, Cc] + [2, 2] + flow * d.n_flows  # pre, convs, proj; flows.0; flows.{2k+1}
    out += [Cc, Cc] + dds + [Cc * Cc, Cc] + [2, 2] + flow * 4  # post_pre [C, 1, 1], post_convs, post_proj; post_flows.0; post_flows.{1, 3, 5, 7}
    return out + ([Cc * d.gin_channels, Cc] if d.gin_channels else [])


def _pack(_lib, lib, fam, d, h):
    """-> the packed blob (a device tensor) of hashed weights"""
    import torch

    from test_blob_layout_hip import hashed

    fn = lambda what: getattr(lib, f"{fam}_{what}")
    sizes = {"ttsgen": gen_sizes, "ttsvits_durnll": durnll_sizes, "ttsdur": lambda d: dur_sizes(_lib, d)}[fam](d)
    assert fn("num_weight_tensors")(h) == len(sizes)
    dev = [torch.from_numpy(hashed(n, i)).to("cuda:0") for i, n in enumerate(sizes)]
    arr = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    blob = torch.empty(fn("packed_bytes")(h), dtype=torch.uint8, device="cuda:0")
    assert blob.data_ptr() % 256 == 0
    rc = fn("pack_weights")(h, arr, len(dev), blob.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.OK, rc
    torch.cuda.synchronize()
    return blob


def packed(name):
    """-> the bytes of the packed blob or, for a PLANES name, of the planes buffer"""
    import torch

    from test_layout_host import family_dims
    from torch_tts_amd import _lib

    if name in PLANES:
        from test_generator_split_host import _small_dims

        fam, d = ("ttsgen", _small_dims(**PLANES[name])) if PLANES[name] else family_dims(_lib)["gen_small"]
    else:
        fam, d = family_dims(_lib)[name]
    lib, h = _lib.load(), C.c_void_p()
    assert getattr(lib, fam + "_create")(C.byref(d), C.byref(h)) == _lib.OK
    try:
        blob = _pack(_lib, lib, fam, d, h)
        if name not in PLANES:
            return blob.cpu().numpy().tobytes()
        assert lib.ttsgen_bind_weights(h, blob.data_ptr()) == _lib.OK
        planes = torch.zeros(lib.ttsvits_generator_planes_bytes(h), dtype=torch.uint8, device="cuda:0")
        assert planes.data_ptr() % 256 == 0
        rc = lib.ttsvits_generator_pack_planes(h, planes.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.OK, rc
        torch.cuda.synchronize()
        return planes.cpu().numpy().tobytes()
    finally:
        getattr(lib, fam + "_destroy")(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PACKED) + list(PLANES))
def test_packed_bytes_are_the_recorded_ones(name):
    recorded = json.load(open(os.path.join(HERE, "golden", "gen_dur_blob_sha256.json")))
    data = packed(name)
    got = hashlib.sha256(data).hexdigest()
    print(name, len(data), got)
    assert len(data) == recorded[name]["bytes"]
    assert got == recorded[name]["sha256"]


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    out = {}
    for name in list(PACKED) + list(PLANES):
        data = packed(name)
        out[name] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
    print(json.dumps(out, indent=1))
