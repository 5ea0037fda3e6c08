"""Host side of tests/test_kwalk_ends_hip.py: the Postnet hidden widths of that file give K walks of 1, 2, S-2, S-1, S and S+1
tiles on the tiles csrc/decode_kernels.hip launch_gemm_cfg picks for those shapes.  The tiles are restated here and pinned to the
dispatcher's source text, so a change of tile choice fails this test instead of silently thinning the GPU test's coverage."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSTNET_HIDDEN = (8, 16, 32, 48, 64, 72, 96, 112)  # tests/test_kwalk_ends_hip.py POSTNET_HIDDEN

# arithmetic -> (the dispatcher's line for small M, bytes of a tile row per plane, element bytes, ring depth S)
# TileCfg<WM, WN, WK, S, PREC, AUXB, TM, TN, HK>: ROWB = (HK ? 64 : 128) * WK (csrc/gemm_tile.h)
TILES = {
    "f32": ("using Cfg = TileCfg<1, 1, 4, 4>;", 128 * 4, 4, 4),
    "split_f16": ("using Cfg = TileCfg<2, 2, 1, (PREC == PREC_BF16 ? 5 : 4), PREC>;", 128, 2, 4),
    "bf16": ("using Cfg = TileCfg<2, 2, 1, (PREC == PREC_BF16 ? 5 : 4), PREC>;", 128, 2, 5),
}


def _launch_gemm_cfg_source():
    src = open(os.path.join(ROOT, "torch-tts_amd", "csrc", "decode_kernels.hip")).read()
    a = src.index("static void launch_gemm_cfg(")
    return src[a : src.index("static void launch_gemm_dil(", a)]


def test_gpu_test_constants_are_the_same():
    hip = open(os.path.join(ROOT, "tests", "test_kwalk_ends_hip.py")).read()
    m = re.search(r"^POSTNET_HIDDEN = \(([^)]*)\)", hip, re.M)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == POSTNET_HIDDEN


def test_dispatcher_still_picks_the_tiles_restated_here():
    body = _launch_gemm_cfg_source()
    for mode, (line, rowb, eb, S) in TILES.items():
        assert line in body, (mode, line)
    # the small-M exact-fp32 branch is the `else` of the 64 x 64 one, and the 16-bit modes never reach it
    assert "if (PREC != PREC_F32 || (a.fixed_tile != 1 && a.M >= 64 && tiles_big >= 512)) {" in body
    # 3 utterances x 5 frames = 15 rows: below every big-tile threshold of the dispatcher
    assert "a.M >= 2048" in body and "tiles_big < 512" in body


def test_postnet_hidden_widths_cover_every_walk_length():
    """K = 5 * hidden for the hidden -> hidden convs; tiles = ceil(K / k per tile)"""
    for mode, (_, rowb, eb, S) in TILES.items():
        kt = rowb // eb
        walks = {-(-5 * h // kt) for h in POSTNET_HIDDEN}
        want = {1, 2, S - 2, S - 1, S, S + 1}
        assert want <= walks, (mode, kt, S, sorted(walks))
