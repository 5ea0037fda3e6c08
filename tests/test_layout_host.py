"""The sizes every family of the C ABI reports - workspaces and packed blobs - are the ones recorded below.  The layouts behind
them are walked by one carver (csrc/layout.h) and may be rewritten; what a caller is told to allocate, and where a blob's tensors
lie, may not move.  No GPU needed.

    python tests/test_layout_host.py      prints the table from the library in torch-tts_amd/lib (or TTSDEC_LIB)"""
import ctypes as C
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BT = [(1, 1), (2, 37), (3, 200)]
N_FFT = (256, 512, 1024, 2048)


def _golden(name):
    return json.load(open(os.path.join(HERE, "golden", name)))


def _gen_dims(_lib, dims, gin):
    d = _lib.GenDims()
    d.initial_channel, d.upsample_initial_channel = dims["initial_channel"], dims["upsample_initial_channel"]
    d.n_up, d.n_res, d.n_dil, d.resblock, d.gin_channels = len(dims["upsample_rates"]), len(dims["resblock_kernel_sizes"]), 3, 1, gin
    for i, (u, k) in enumerate(zip(dims["upsample_rates"], dims["upsample_kernel_sizes"])):
        d.up_rates[i], d.up_kernels[i] = u, k
    for j, (k, ds) in enumerate(zip(dims["resblock_kernel_sizes"], dims["resblock_dilation_sizes"])):
        d.res_kernels[j] = k
        for l, dl in enumerate(ds):
            d.res_dilations[j][l] = dl
    return d


def family_dims(_lib):
    """name -> (family prefix, dims struct): the golden fixtures' small dims and the model configuration's, with and without gin."""
    from oracle import vits2_oracle as V

    sm, t2, gm, vm = _golden("meta.json")["small_dims"], _golden("taco2_meta.json")["dims"], _golden("generator_meta.json"), _golden("vits2_meta.json")
    out = {}
    # decoder + postnet: MelPostnet (small_cases.npz / LJSpeech) and MelPostnet2 (taco2_cases.npz / the 512-wide configuration)
    out["dec_small_mel"] = ("ttsdec", _lib.Dims(sm["d_mel"], sm["r"], sm["d_pre"], sm["d_ctx"], sm["h_att"], sm["h_dec"], 0.1, 0.5,
                                                sm["postnet_layers"], sm["postnet_hidden"], 5, 1e-5, _lib.CELL_TACO2PROD, 0, _lib.POSTNET_TYPE_MEL))
    out["dec_small_mel2"] = ("ttsdec", _lib.Dims(t2["d_mel"], t2["r"], t2["d_pre"], t2["d_ctx"], t2["h_att"], t2["h_dec"], 0.1, 0.5,
                                                 t2["postnet_layers"], t2["postnet_hidden"], 5, 1e-5, _lib.CELL_TACO2, t2["d_pre_hidden"],
                                                 _lib.POSTNET_TYPE_MEL2))
    out["dec_model_mel"] = ("ttsdec", _lib.Dims(80, 1, 256, 512, 1024, 1024, 0.1, 0.5, 5, 512, 5, 1e-5, _lib.CELL_TACO2PROD, 0, _lib.POSTNET_TYPE_MEL))
    out["dec_model_mel2"] = ("ttsdec", _lib.Dims(80, 1, 256, 512, 1024, 1024, 0.1, 0.5, 5, 512, 5, 1e-5, _lib.CELL_TACO2, 0, _lib.POSTNET_TYPE_MEL2))
    out["enc_small"] = ("ttsenc", _lib.EncDims(40, 24, 40, 5, 1e-5))
    out["enc_model"] = ("ttsenc", _lib.EncDims(148, 512, 512, 5, 1e-5))
    vits = {"small": vm["dims"], "small_g": vm["dims_g"], "model": dataclasses.asdict(V.Vits2Dims()),
            "model_g": dataclasses.asdict(V.Vits2Dims(gin_channels=256))}
    for name, d in vits.items():
        d = dict(dict(gin_channels=0, cond_layer_idx=0), **d)
        out["vits_" + name] = ("ttsvits", _lib.VitsDims(*[int(d[n]) for n, _ in _lib.VitsDims._fields_]))
    for name, dims, gin in (("small", gm["dims"], 0), ("small_g", gm["dims"], 4), ("model", gm["fulldims"], 0), ("model_g", gm["fulldims"], 256)):
        out["gen_" + name] = ("ttsgen", _gen_dims(_lib, dims, gin))
    for name, C_, F_, gin in (("small", 32, 48, 0), ("small_g", 32, 48, 4), ("model", 192, 256, 0), ("model_g", 192, 256, 256)):
        out["sdp_" + name] = ("ttsdur", _lib.DurDims(_lib.DUR_SDP, C_, 192, 3, 4, gin))
        out["dp_" + name] = ("ttsdur", _lib.DurDims(_lib.DUR_DP, C_, F_, 3, 0, gin))
        out["durnll_" + name] = ("ttsvits_durnll", _lib.DurNllDims(C_, 3, 4, gin))
    out["post_small"] = ("ttspost", _lib.PostDims(13, 8, 16, 5, 3, 0))
    out["post_small_g"] = ("ttspost", _lib.PostDims(16, 8, 16, 5, 3, 8))
    out["post_model"] = ("ttspost", _lib.PostDims(513, 192, 192, 5, 16, 0))
    out["post_model_g"] = ("ttspost", _lib.PostDims(513, 192, 192, 5, 16, 256))
    return out


def reported_sizes(lib, _lib):
    """-> {row name: [numbers]} of the loaded library; workspaces at BT in order."""
    rows, handles = {}, {}
    for name, (fam, d) in family_dims(_lib).items():
        h = C.c_void_p()
        assert getattr(lib, fam + "_create")(C.byref(d), C.byref(h)) == _lib.OK, name
        handles[name] = (fam, h)
        rows[name + "/packed"] = [getattr(lib, fam + "_packed_bytes")(h)]
        if fam == "ttsdec":
            rows[name + "/decode_ws"] = [lib.ttsdec_workspace_bytes(h, B, T) for B, T in BT]
            rows[name + "/postnet_ws"] = [lib.ttsdec_postnet_workspace_bytes(h, B, T) for B, T in BT]
        elif fam == "ttsvits":
            pass  # (text encoder / flow workspaces: tests/test_vc_host.py WORKSPACE_BYTES)
        else:
            rows[name + "/ws"] = [getattr(lib, fam + "_workspace_bytes")(h, B, T) for B, T in BT]
    hd, hv = handles["dec_small_mel"][1], handles["vits_small"][1]
    for n_fft in N_FFT:
        rows[f"griffinlim_ws/{n_fft}"] = [lib.ttsdec_griffinlim_workspace_bytes(hd, B, T, n_fft) for B, T in BT]  # (T < 2: refused)
        rows[f"spec_ws/{n_fft}"] = [lib.ttsvits_spec_workspace_bytes(hv, n_fft, n_mels) for n_mels in (0, 80, 128)]
        rows[f"mel_analysis_ws/{n_fft}"] = [lib.ttsdec_mel_analysis_workspace_bytes(hd, B, n_fft, n_mels) for B in (1, 2, 3) for n_mels in (80, 128)]
    rows["align_ws"] = [lib.ttsvits_align_workspace_bytes(hv, B, T, Tx) for B, T in BT for Tx in (1, 9, 150)]
    os.environ["TTSGEN_GROUP_FORCE"] = "2"  # (read at every call: groups of two utterances, so B = 3 reports what B = 2 needs)
    try:
        for name in ("gen_small_g", "gen_model"):
            rows[name + "/ws_group2"] = [lib.ttsgen_workspace_bytes(handles[name][1], B, T) for B, T in BT]
    finally:
        del os.environ["TTSGEN_GROUP_FORCE"]
    # what is refused reports 0
    zeros = []
    for name, (fam, h) in handles.items():
        fns = {"ttsdec": ["ttsdec_workspace_bytes", "ttsdec_postnet_workspace_bytes"], "ttsvits": ["ttsvits_text_encoder_workspace_bytes",
               "ttsvits_flow_workspace_bytes"]}.get(fam, [fam + "_workspace_bytes"])
        for fn in fns:
            zeros += [getattr(lib, fn)(h, 0, 5), getattr(lib, fn)(h, 2, 0), getattr(lib, fn)(h, -1, -1), getattr(lib, fn)(None, 2, 5)]
        zeros.append(getattr(lib, fam + "_packed_bytes")(None))
    zeros += [lib.ttsdec_griffinlim_workspace_bytes(hd, 2, 37, 300), lib.ttsdec_griffinlim_workspace_bytes(hd, 0, 37, 512),
              lib.ttsdec_griffinlim_workspace_bytes(hd, 2, 1, 512), lib.ttsdec_griffinlim_workspace_bytes(None, 2, 37, 512),
              lib.ttsvits_spec_workspace_bytes(hv, 300, 80), lib.ttsvits_spec_workspace_bytes(hv, 512, -1), lib.ttsvits_spec_workspace_bytes(None, 512, 80),
              lib.ttsvits_align_workspace_bytes(hv, 0, 37, 9), lib.ttsvits_align_workspace_bytes(hv, 2, 37, 0), lib.ttsvits_align_workspace_bytes(hv, 2, 37, 1025),
              lib.ttsvits_align_workspace_bytes(None, 2, 37, 9),
              lib.ttsdec_mel_analysis_workspace_bytes(hd, 2, 300, 80), lib.ttsdec_mel_analysis_workspace_bytes(hd, 2, 512, 257),
              lib.ttsdec_mel_analysis_workspace_bytes(hd, 0, 512, 80), lib.ttsdec_mel_analysis_workspace_bytes(None, 2, 512, 80)]
    rows["refused"] = [sum(1 for z in zeros if z != 0), len(zeros)]
    for fam, h in handles.values():
        getattr(lib, fam + "_destroy")(h)
    return rows


# As the library of commit e178cdf ("VITS2 flow path: one templated kernel per step, one layout per workspace") reported them, before
# the size functions of these families became their carve routines' totals; the mel_analysis_ws rows as the library of commit 3e4a5ff
# ("Add Tacotron audio analysis on HIP") reported them; the durnll rows as the library of commit e4aad43 ("Add the VITS2 duration
# likelihood on HIP") reported them, before the two SDP handles shared their records.  Bytes.
RECORDED = {
    "dec_small_mel/packed": [1472256],
    "dec_small_mel/decode_ws": [112896, 118784, 129280],
    "dec_small_mel/postnet_ws": [768, 44032, 355328],
    "dec_small_mel2/packed": [1867264],
    "dec_small_mel2/decode_ws": [112640, 119040, 130816],
    "dec_small_mel2/postnet_ws": [1536, 66560, 537600],
    "dec_model_mel/packed": [275090176],
    "dec_model_mel/decode_ws": [1320192, 1391872, 1467136],
    "dec_model_mel/postnet_ws": [4608, 326912, 2649600],
    "dec_model_mel2/packed": [313195264],
    "dec_model_mel2/decode_ws": [1320192, 1391872, 1467136],
    "dec_model_mel2/postnet_ws": [6144, 398336, 3225600],
    "enc_small/packed": [149248],
    "enc_small/ws": [3584, 99072, 788736],
    "enc_model/packed": [50651136],
    "enc_model/ws": [28672, 1679360, 13535232],
    "vits_small/packed": [593664],
    "vits_small_g/packed": [726272],
    "vits_model/packed": [112987648],
    "vits_model_g/packed": [125989120],
    "gen_small/packed": [206336],
    "gen_small/ws": [1792, 113920, 922112],
    "gen_small_g/packed": [207104],
    "gen_small_g/ws": [1792, 113920, 922112],
    "gen_model/packed": [62648064],
    "gen_model/ws": [198656, 14553088, 117970944],
    "gen_model_g/packed": [63174400],
    "gen_model_g/ws": [198656, 14553088, 117970944],
    "sdp_small/packed": [96768],
    "sdp_small/ws": [1536, 38912, 312576],
    "dp_small/packed": [48128],
    "dp_small/ws": [512, 14592, 115712],
    "sdp_small_g/packed": [97536],
    "sdp_small_g/ws": [1536, 38912, 312576],
    "dp_small_g/packed": [48896],
    "dp_small_g/ws": [512, 14592, 115712],
    "sdp_model/packed": [2221568],
    "sdp_model/ws": [4096, 229632, 1850368],
    "dp_model/packed": [1383680],
    "dp_model/ws": [1792, 77312, 616704],
    "sdp_model_g/packed": [2418944],
    "sdp_model_g/ws": [4096, 229632, 1850368],
    "dp_model_g/packed": [1581056],
    "dp_model_g/ws": [1792, 77312, 616704],
    "durnll_small/packed": [235776],
    "durnll_small/ws": [2048, 39936, 317696],
    "durnll_small_g/packed": [236544],
    "durnll_small_g/ws": [2048, 39936, 317696],
    "durnll_model/packed": [5270784],
    "durnll_model/ws": [4608, 230656, 1855488],
    "durnll_model_g/packed": [5468160],
    "durnll_model_g/ws": [4608, 230656, 1855488],
    "post_small/packed": [77824],
    "post_small/ws": [3840, 68864, 541440],
    "post_small_g/packed": [84480],
    "post_small_g/ws": [3840, 68864, 541440],
    "post_model/packed": [57767424],
    "post_model/ws": [40960, 1193984, 9349888],
    "post_model_g/packed": [70374912],
    "post_model_g/ws": [40960, 1193984, 9349888],
    "griffinlim_ws/256": [0, 269312, 2164736],
    "spec_ws/256": [2048, 2816, 3072],
    "mel_analysis_ws/256": [3328, 3584, 3328, 3584, 3328, 3584],
    "griffinlim_ws/512": [0, 536576, 4317184],
    "spec_ws/512": [4096, 4864, 5120],
    "mel_analysis_ws/512": [5376, 5632, 5376, 5632, 5376, 5632],
    "griffinlim_ws/1024": [0, 1071104, 8622080],
    "spec_ws/1024": [8192, 8960, 9216],
    "mel_analysis_ws/1024": [9472, 9728, 9472, 9728, 9472, 9728],
    "griffinlim_ws/2048": [0, 2140160, 17231872],
    "spec_ws/2048": [16384, 17152, 17408],
    "mel_analysis_ws/2048": [17664, 17920, 17664, 17920, 17664, 17920],
    "align_ws": [256, 256, 256, 4864, 4864, 4864, 38400, 38400, 38400],
    "gen_small_g/ws_group2": [1792, 113920, 614656],
    "gen_model/ws_group2": [198656, 14553088, 78647296],
    "refused": [0, 197],
}


def test_reported_sizes_are_the_recorded_ones():
    from torch_tts_amd import _lib

    got = reported_sizes(_lib.load(), _lib)
    assert sorted(got) == sorted(RECORDED)
    for name, want in RECORDED.items():
        assert got[name] == want, (name, got[name], want)
    assert got["refused"][0] == 0 and got["refused"][1] > 60


# ---- the reach of the LSTM kernels' one-descriptor loaders (csrc/gemm_tile.h DmaDesc::PerPlane, csrc/layout.h within_dma_reach):
# a workspace or a packed blob that reaches the descriptor's range is refused ----
BUF_RANGE = 0x7FFFF000  # csrc/common.h kBufRange
B_TOP = 1 << 30         # (the layouts round B up in int arithmetic: stay clear of INT_MAX)


def _style_dims(_lib, n_mels, filters, d_enc):
    f = (C.c_int32 * _lib.STYLE_MAX_CONVS)(*filters)
    return _lib.StyleDims(n_mels=n_mels, n_convs=len(filters), filters=f, d_enc=d_enc, kind=_lib.STYLE_ENCODER, bn_eps=1e-5)


def _reach_families(_lib):
    """-> {name: (create / destroy prefix, dims, name of the workspace query, L or T)}"""
    return {"ttsdec": ("ttsdec", _lib.Dims(80, 1, 256, 512, 1024, 1024, 0.1, 0.5, 5, 512, 5, 1e-5, _lib.CELL_TACO2PROD, 0, _lib.POSTNET_TYPE_MEL),
                       "ttsdec_workspace_bytes", 37),
            "ttsenc": ("ttsenc", _lib.EncDims(148, 512, 512, 5, 1e-5), "ttsenc_workspace_bytes", 37),
            "ttsenc_style": ("ttsenc_style", _style_dims(_lib, 80, (32, 32, 64, 64, 128, 128), 128), "ttsenc_style_workspace_bytes", 37)}


def test_the_range_constant_is_the_librarys():
    import re

    src = open(os.path.join(ROOT, "torch-tts_amd", "csrc", "common.h")).read()
    assert [int(v, 16) for v in re.findall(r"constexpr unsigned kBufRange = (0x[0-9A-Fa-f]+)u;", src)] == [BUF_RANGE]


def test_workspace_queries_refuse_what_reaches_the_descriptor_range():
    from torch_tts_amd import _lib

    lib = _lib.load()
    for name, (fam, d, query, L) in _reach_families(_lib).items():
        h = C.c_void_p()
        assert getattr(lib, fam + "_create")(C.byref(d), C.byref(h)) == _lib.OK, name
        ws = lambda B: getattr(lib, query)(h, B, L)
        assert ws(1) != 0 and ws(B_TOP) == 0, name
        lo, hi, seen = 1, B_TOP, {}  # ws(lo) != 0, ws(hi) == 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            seen[mid] = ws(mid)
            lo, hi = (mid, hi) if seen[mid] else (lo, mid)
        print(name, "largest B", lo, "bytes", ws(lo), "of", BUF_RANGE)
        assert 0 < ws(lo) < BUF_RANGE and ws(lo + 1) == 0, (name, lo, ws(lo), ws(lo + 1))
        assert all((v != 0) == (B <= lo) for B, v in seen.items()), name  # (what the bisection stands on)
        # non-decreasing up to there: a geometric ladder from 1, and every B of the last stretch
        ladder = sorted({min(lo, int(1.07 ** i)) for i in range(400)} | set(range(max(1, lo - 130), lo + 1)))
        sizes = [ws(B) for B in ladder]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), name
        assert getattr(lib, fam + "_destroy")(h) == _lib.OK


def test_create_refuses_a_blob_that_reaches_the_descriptor_range():
    """Dims whose only offence is the size of the packed blob; one size below, the same dims are accepted and stay below the range."""
    from torch_tts_amd import _lib

    lib = _lib.load()
    dec = lambda H: _lib.Dims(80, 1, 256, 512, H, H, 0.1, 0.5, 0, 0, 5, 1e-5, _lib.CELL_TACO2PROD, 0, _lib.POSTNET_TYPE_MEL)
    cases = {"ttsdec": (dec(2048), dec(4096)),  # the LSTM matrices, ~13.2 H^2 elements in three forms of 4 bytes each: 2.7 GB at H = 4096
             "ttsenc": (_lib.EncDims(148, 512, 8192, 5, 1e-5), _lib.EncDims(148, 512, 16384, 5, 1e-5)),  # w_hh: 2 x 4 (d_out / 2)^2
             "ttsenc_style": (_style_dims(_lib, 128, (1024,), 1024), _style_dims(_lib, 256, (1024,), 1024))}  # w_ih: 4 d_enc x 1024 x n_mels / 2
    for fam, (fits, too_big) in cases.items():
        h = C.c_void_p()
        assert getattr(lib, fam + "_create")(C.byref(fits), C.byref(h)) == _lib.OK, fam
        assert 0 < getattr(lib, fam + "_packed_bytes")(h) < BUF_RANGE, fam
        assert getattr(lib, fam + "_destroy")(h) == _lib.OK
        h = C.c_void_p()
        assert getattr(lib, fam + "_create")(C.byref(too_big), C.byref(h)) == _lib.ERR_DIMS, fam
        assert not h.value, fam


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from torch_tts_amd import _lib

    for k, v in reported_sizes(_lib.load(), _lib).items():
        print(f'    "{k}": {v},')
