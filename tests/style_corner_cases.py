"""The corners of the dims that ttsenc_style_create accepts (1 to 8 conv stages of any filter count % 4 == 0 up to 1024, any n_mels,
d_enc % 4 == 0 up to 1024, any d_emb up to 1024, d_vae up to 256, up to 64 tokens and 16 heads) that no other test runs: one table
shared by tests/golden/make_golden_style_corners.py (which runs the REFERENCE's modules on it), tests/test_style_corners_host.py
and tests/test_style_corners_hip.py, so that all three see the same cases.

Nothing here stores a weight.  A module is built in a namespace `ns` (the reference's modules.style in the golden script,
torch_tts_amd.style in the tests); its encoder is replaced by ReferenceEncoder(n_mels, d_enc, filters) and, for the GST kinds, its
stl by STL(dim_query=d_enc, ...) - the reference's GST builds both at their defaults - as test_style_host.make_module and
make_golden_style.py do, both drawn after torch.manual_seed(seed), the VAE linears drawn again behind them; then `randomize` moves
what a fresh module leaves at zero or one.  (Its
".bns." test does not match the keys of a bare ReferenceEncoder - "bns.0.weight": the encoder-only cases keep a BatchNorm gain of
one.  That is the recipe as the other style tests have always used it.)  Inputs are seeded randn, zero past each length; eps is
seeded too and handed to both sides.

No seed of the table had to be changed for the margin condition of test_style_corners_host.py (fp32 within a quarter of the bar
from fp64): it holds for every case and layout as listed."""
import torch

KINDS = ("encoder", "vae", "gst", "gstvae")

# name -> dims, layouts [(B, T, lengths or the cycle the lengths are drawn from)], seed; what each case reaches:
CASES = {
    # the smallest of everything; one stage: no implicit GEMM runs at all; F = 1; H = K = 4 in the LSTM
    "S1": dict(kind="encoder", n_mels=1, filters=[4], d_enc=4, layouts=[(3, 5, [5, 2, 1])], seed=401),
    # C0 = 12: ppb = 85, one idle thread; Ci = 12 and 20: 36- and 60-float K segments, no whole 32-k tiles; Co = 20 on the 128 x 32
    # tile and Co = 36 on the 64 x 64 tile, both ragged; d_emb % 4 != 0; d_vae = 1; H % 8 == 4
    "S2": dict(kind="vae", n_mels=20, filters=[12, 20, 36], d_enc=20, d_emb=6, d_vae=1, layouts=[(3, 37, [37, 18, 1])], seed=402),
    # TTSENC_STYLE_MAX_CONVS stages; T' = 3 with 2 / 1 / 1 steps; F reaches 1 at stage 3; dk = 2; a softmax over one token
    "S3": dict(kind="gst", n_mels=7, filters=[8] * 8, d_enc=8, d_emb=6, n_heads=3, n_tokens=1, layouts=[(3, 600, [600, 511, 1])], seed=403),
    # Ci >= 64: the split-K 32 x 32 tile with Co = 68 and 132 (ragged last column tile); every limit of the tail kernel at its maximum
    "S4": dict(kind="gstvae", n_mels=16, filters=[64, 68, 132], d_enc=36, d_emb=1024, n_heads=16, n_tokens=64, d_vae=256,
               layouts=[(3, 37, [37, 18, 1])], seed=404),
    # C0 = 1024: ppb = 1; Ci = Co = 1024 (K = 9216); H = K = 1024 in the LSTM
    "S5": dict(kind="encoder", n_mels=4, filters=[1024, 1024], d_enc=1024, layouts=[(2, 9, [9, 4])], seed=405),
    # the LSTM on the 64 x 16 tile (B = 129) and on the 64 x 8 tile (B = 97), a ragged last row block in both; Ci = 4: 12-float K
    # segments; d_enc just over the tail kernel's 256 threads
    "S6": dict(kind="vae", n_mels=8, filters=[4, 4, 8], d_enc=260, d_emb=5, d_vae=3,
               layouts=[(129, 26, "cycle"), (97, 26, "cycle")], cycle=[26, 1, 25, 13, 8, 7], seed=406),
    # the gx GEMM with 2013 rows x 1024 columns: 32 x 16 = 512 tiles, the 64 x 64 fp32 tile; 61 LSTM steps, rows stopping at
    # different ones
    "S7": dict(kind="encoder", n_mels=4, filters=[8], d_enc=256, layouts=[(33, 122, "cycle")], cycle=[122, 1, 121, 61, 2, 1], seed=407),
    # F = 1 from stage 0 on: only the centre kx tap is inside the picture; Ci = 4 to Co = 1024 (16 column tiles of the 64 x 64 tile);
    # one head over 64 tokens
    "S8": dict(kind="gst", n_mels=2, filters=[4, 1024], d_enc=12, d_emb=16, n_heads=1, n_tokens=64, layouts=[(3, 9, [9, 4, 1])], seed=408),
}
NO_LENGTHS = ("S1", "S2", "S3", "S4", "S5", "S8")  # the cases the GPU test also runs with lengths=None (every row all T' steps)


def randomize(m, seed):
    """Fresh modules have zero biases and unit BatchNorm: move them (as the fixture's generator does), so that nothing cancels."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif k.endswith("running_mean"):
                v.add_(0.1 * torch.randn(v.shape, generator=g))
            elif ".bns." in k and k.endswith(".weight"):
                v.copy_(1.5 + 0.5 * torch.rand(v.shape, generator=g))
            elif k.endswith("logvar_linear.bias"):
                v.copy_(-1.0 + 0.5 * torch.randn(v.shape, generator=g))
            elif k.endswith("mean_linear.bias"):
                v.copy_(0.7 + 0.5 * torch.randn(v.shape, generator=g))
            elif "bias" in k:
                v.add_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("convs.0.weight"):
                v.mul_(3.0)
    if hasattr(m, "invalidate"):  # (the drop-ins' packed blob; the reference's modules have none)
        m.invalidate()
    return m.eval()


def make_module(ns, name):
    """The case's module from ns.ReferenceEncoder / VAE / GST / GST_VAE / STL, filled from the case's seed, in eval mode on the CPU."""
    c = CASES[name]
    kind = c["kind"]
    # the shell first: what it draws differs between the namespaces (the reference's GST builds its STL with dim_query = 128, the
    # drop-in with dim_enc), so the seed is set behind it and every part that stays is drawn from there on, in one fixed order
    if kind == "vae":
        m = ns.VAE(num_mels=c["n_mels"], dim_emb=c["d_emb"], dim_enc=c["d_enc"], dim_vae=c["d_vae"])
    elif kind != "encoder":
        kw = dict(num_mels=c["n_mels"], dim_emb=c["d_emb"], dim_enc=c["d_enc"], num_tokens=c["n_tokens"], num_heads=c["n_heads"])
        m = ns.GST(**kw) if kind == "gst" else ns.GST_VAE(**kw, dim_vae=c["d_vae"])
    torch.manual_seed(c["seed"])
    enc = ns.ReferenceEncoder(num_mels=c["n_mels"], dim_out=c["d_enc"], ref_enc_filters=list(c["filters"]))
    if kind == "encoder":
        return randomize(enc, c["seed"])
    m.encoder = enc
    if kind in ("gst", "gstvae"):
        m.stl = ns.STL(dim_query=c["d_enc"], num_tokens=c["n_tokens"], dim_emb=c["d_emb"], num_heads=c["n_heads"])
    if kind in ("vae", "gstvae"):
        for lin in (m.mean_linear, m.logvar_linear, m.fc_out):
            lin.reset_parameters()
    return randomize(m, c["seed"])


def layouts(name):
    """[(B, T, lengths [B] as a list)] of a case."""
    c = CASES[name]
    out = []
    for B, T, lengths in c["layouts"]:
        if lengths == "cycle":
            lengths = [c["cycle"][b % len(c["cycle"])] for b in range(B)]
        assert len(lengths) == B and max(lengths) == T
        out.append((B, T, list(lengths)))
    return out


def all_layouts():
    """[(name, i)] over every layout of every case."""
    return [(n, i) for n in CASES for i in range(len(CASES[n]["layouts"]))]


def inputs(name, i=0):
    """(x [B, T, n_mels] zero past each length, lengths [B] int64, eps [B, d_vae] or None) of layout i, seeded by the case."""
    c = CASES[name]
    B, T, lengths = layouts(name)[i]
    g = torch.Generator().manual_seed(1000 * c["seed"] + i)
    x = torch.randn(B, T, c["n_mels"], generator=g)
    for b, n in enumerate(lengths):
        x[b, n:] = 0
    eps = torch.randn(B, c["d_vae"], generator=g) if "d_vae" in c else None
    return x, torch.tensor(lengths), eps


def key(name, i):
    return f"{name}/B{layouts(name)[i][0]}"


# ---------------------------------------------------------------------------------------------------------------------------
# what the library does with a case's dims, restated (tests/test_style_corners_host.py pins each rule to the source text)
# ---------------------------------------------------------------------------------------------------------------------------
def half_up(n, times=1):
    for _ in range(times):
        n = (n + 1) // 2
    return n


def conv_tile(Ci, Co):
    """style.hip launch_conv: the tile of an implicit-GEMM stage, from its channel counts alone."""
    return "32x32 split-K" if Ci >= 64 else ("128x32" if Co <= 32 else "64x64")


def conv_tiles(name):
    """[(Ci, Co, tile)] of stages 1 .. K-1."""
    f = CASES[name]["filters"]
    return [(f[i - 1], f[i], conv_tile(f[i - 1], f[i])) for i in range(1, len(f))]


def lstm_tile(B):
    """decode_kernels.hip launch_lstm, exact fp32: rows x units of the tile."""
    return "64x16" if B > 128 else ("64x8" if B >= 96 else "32x8")


def gx_gemm(name, i=0):
    """(M, N, K, tile) of the LSTM's input projection: decode_kernels.hip launch_gemm_cfg, exact fp32."""
    c = CASES[name]
    B, T, _ = layouts(name)[i]
    K = len(c["filters"])
    M, N = B * half_up(T, K), 4 * c["d_enc"]
    big = M >= 64 and ((M + 63) // 64) * ((N + 63) // 64) >= 512
    return M, N, half_up(c["n_mels"], K) * c["filters"][-1], "64x64" if big else "32x32 split-K"


def steps(name, i=0):
    """Each row's LSTM step count: clip(len >> K, 1, T')."""
    c = CASES[name]
    _, T, lengths = layouts(name)[i]
    K = len(c["filters"])
    return [min(max(n >> K, 1), half_up(T, K)) for n in lengths]
