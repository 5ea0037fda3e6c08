"""The corners of the dims that ttsvits_create (the text encoder and the coupling flow, both directions) and ttspost_create (the
posterior encoder) accept and that no other test runs: one table per family, shared by tests/golden/make_golden_vits2_dims_corners.py
(which runs the REFERENCE's modules on them), tests/test_vits2_dims_corners_host.py and tests/test_vits2_dims_corners_hip.py, so that
all three see the same cases.

Nothing here stores a weight: every module - the reference's in the golden script, the drop-in in the tests; `ns` below is whichever
namespace holds the classes - is filled by recipes.fill_by_key(module, seed, gain), weight-norm gains included.  The inputs are
seeded too; the golden file keeps them beside the reference's outputs.  The fp64 restatements the three files judge by are at the
bottom: oracle.vits2_oracle.text_encoder / flow_reverse and test_vc_host.flow_forward / posterior_encoder on a module's state dict.

One batch layout throughout, B = 3, T = 37, lengths 37 / 18 / 1: M = 111 rows, ragged 16- and 32-row tiles, an utterance of one
frame, utterances starting inside a tile.  A case with its own layout carries B, T and lengths."""
import torch

import recipes
from oracle import vits2_oracle as V
from test_vc_host import flow_dims, flow_forward, posterior_encoder

B, T, LENGTHS = 3, 37, [37, 18, 1]
WIDE = dict(B=3, T=9, lengths=[9, 4, 1])  # the 1024-channel cases: 27 rows
N_VOCAB = 11
WINDOW = 4    # attentions.Encoder's default, which models.TextEncoder does not override
STRIDE = 13   # the big cases' outputs are stored at this stride of the flattened tensor (as dims_corners.npz's feature maps)
BIG = ("E6", "F5", "Q5")

# ---------------------------------------------------------------------------------------------------------------------------
# Text encoder: TextEncoder(n_vocab, inter, hidden, filter, heads, layers, kernel, p_dropout, gin_channels=gin).  models.TextEncoder
# cannot pass cond_layer_idx (attentions.Encoder then takes 2 and asserts 2 < n_layers): `cond` is set on the built encoder, on
# both sides - its forward and the drop-in's dims read the attribute.
# ---------------------------------------------------------------------------------------------------------------------------
TE_CASES = {
    # smallest of everything; first = last layer; one tap; dk 4, scalar attention
    "E1": dict(hidden=4, filter=4, heads=1, layers=1, kernel=1, inter=4, gin=0, cond=0, gain=1.2, seed=101),
    # C % 8 != 0, F % 8 = 0: exact conv_1 writes planes for a split conv_2; Cin 20, where a k tile straddles taps
    "E2": dict(hidden=20, filter=48, heads=5, layers=2, kernel=5, inter=8, gin=0, cond=0, gain=1.2, seed=102),
    # C % 8 = 0, F % 8 != 0: split conv_1, exact conv_2 reads fp32 `f`; cond at layer 0; inter % 8 != 0 in `proj`.  (3 layers, not
    # 2: the reference's constructor asserts its default cond_layer_idx 2 < n_layers before the index can be set)
    "E3": dict(hidden=32, filter=20, heads=2, layers=3, kernel=7, inter=12, gin=4, cond=0, gain=1.2, seed=103),
    # kMaxLayers; cond at the last layer; Cin 12
    "E4": dict(hidden=12, filter=12, heads=3, layers=12, kernel=3, inter=4, gin=4, cond=11, gain=1.2, seed=104),
    # no layers: stats come from the embedding alone
    "E5": dict(hidden=16, filter=16, heads=2, layers=0, kernel=3, inter=8, gin=0, cond=0, gain=1.2, seed=105),
    # LayerNorm <16> at its edge; dk 256, the widest the scalar kernel takes; nine taps over F = 8
    "E6": dict(hidden=1024, filter=8, heads=4, layers=1, kernel=9, inter=4, gin=0, cond=0, gain=1.2, seed=106, **WIDE),
    # LayerNorm <4> (128 < C <= 256) at a width nobody ran; dk 80, scalar
    "E7": dict(hidden=160, filter=8, heads=2, layers=1, kernel=3, inter=4, gin=0, cond=0, gain=1.2, seed=107),
}

# ---------------------------------------------------------------------------------------------------------------------------
# Flow: ResidualCouplingTransformersBlock(channels, hidden, kernel, 1, wn_layers, n_flows=flows, gin_channels=gin,
# use_transformer_flows=True); every case in both directions.  (recipes.fill_by_key pins the reverse flow at gain 0.8.)
# ---------------------------------------------------------------------------------------------------------------------------
FLOW_CASES = {
    # half = 4 (stack C % 8 != 0, dk 2); one flow (no Flip in front, Flip in the copy-out only); one WN layer (first = last); one tap
    "F1": dict(channels=8, hidden=4, kernel=1, wn_layers=1, flows=1, gin=0, gain=0.8, seed=111),
    # half = 12; hidden % 8 != 0, so the gate keeps fp32 `acts` in split mode; kMaxWn; odd flow count; g
    "F2": dict(channels=24, hidden=20, kernel=7, wn_layers=8, flows=3, gin=4, gain=0.8, seed=112),
    # kMaxFlows
    "F3": dict(channels=16, hidden=8, kernel=3, wn_layers=2, flows=8, gin=0, gain=0.8, seed=113),
    # no flows: output equals input in both directions
    "F4": dict(channels=16, hidden=8, kernel=3, wn_layers=2, flows=0, gin=0, gain=0.8, seed=114),
    # half = 512: LayerNorm <16>, dk 256
    "F5": dict(channels=1024, hidden=8, kernel=3, wn_layers=1, flows=1, gin=0, gain=0.8, seed=115, **WIDE),
    # half = 20; 31 taps, wider than every utterance but the first
    "F6": dict(channels=40, hidden=36, kernel=31, wn_layers=3, flows=2, gin=8, gain=0.8, seed=116),
}

# ---------------------------------------------------------------------------------------------------------------------------
# Posterior encoder: PosteriorEncoder(spec, inter, hidden, kernel, 1, layers, gin_channels=gin); the draw eps is given
# ---------------------------------------------------------------------------------------------------------------------------
POST_CASES = {
    # smallest of everything; staged spectrogram of one channel
    "Q1": dict(spec=1, inter=4, hidden=4, kernel=1, layers=1, gin=0, gain=0.8, seed=121),
    # odd spec below one 16-byte row; widest kernel; hidden % 8 != 0
    "Q2": dict(spec=7, inter=12, hidden=20, kernel=31, layers=3, gin=4, gain=0.8, seed=122),
    # kMaxPostWn: 32 accumulations into the skip sum.  gain 0.6: at 0.8 the skip sum drives logs to 8.3 and z = eps * exp(logs) to
    # 234, so that z's bar would judge exp's conditioning (an error of logs within ITS bar is 8e-4 of z) and not the kernels; at 0.6
    # |logs| <= 3.3, as deep as the other cases'
    "Q3": dict(spec=13, inter=8, hidden=8, kernel=3, layers=32, gin=0, gain=0.6, seed=123),
    # hidden just over 256, not a multiple of 8
    "Q4": dict(spec=80, inter=4, hidden=260, kernel=3, layers=2, gin=0, gain=0.8, seed=124),
    # the model's spec and inter at a kernel and depth nobody ran
    "Q5": dict(spec=513, inter=192, hidden=64, kernel=9, layers=2, gin=256, gain=0.8, seed=125, B=2, T=19, lengths=[19, 8]),
}
FAMILIES = {"te": TE_CASES, "flow": FLOW_CASES, "post": POST_CASES}


def layout(c):
    """-> B, T, lengths of a case"""
    return c.get("B", B), c.get("T", T), list(c.get("lengths", LENGTHS))


def mask_of(c):
    b, t, lengths = layout(c)
    return V.sequence_mask(torch.tensor(lengths), t).unsqueeze(1).float()


def _g(c):
    return recipes.seeded_randn(7000 + c["seed"], layout(c)[0], c["gin"], 1) if c["gin"] else None


def make_text_encoder(ns, name):
    c = TE_CASES[name]
    te = ns.TextEncoder(N_VOCAB, c["inter"], c["hidden"], c["filter"], c["heads"], c["layers"], c["kernel"], 0.1, gin_channels=c["gin"]).eval()
    if c["gin"]:
        te.encoder.cond_layer_idx = c["cond"]
    recipes.fill_by_key(te, c["seed"], gain=c["gain"])
    return te


def make_flow(ns, name):
    c = FLOW_CASES[name]
    fl = ns.ResidualCouplingTransformersBlock(c["channels"], c["hidden"], c["kernel"], 1, c["wn_layers"], n_flows=c["flows"],
                                              gin_channels=c["gin"], use_transformer_flows=True).eval()
    recipes.fill_by_key(fl, c["seed"], gain=c["gain"])
    return fl


def make_post(ns, name):
    c = POST_CASES[name]
    pe = ns.PosteriorEncoder(c["spec"], c["inter"], c["hidden"], c["kernel"], 1, c["layers"], gin_channels=c["gin"]).eval()
    recipes.fill_by_key(pe, c["seed"], gain=c["gain"])
    return pe


def te_inputs(name):
    """-> ids [B, T] (every id of the table's range, padded frames too), lengths [B], g [B, gin, 1] or None"""
    c = TE_CASES[name]
    b, t, lengths = layout(c)
    return dict(ids=recipes.seeded_ids(c["seed"], N_VOCAB, b, t), lengths=torch.tensor(lengths), g=_g(c))


def flow_inputs(name):
    """-> z [B, channels, T] with zero padded frames (the flow passes x0 through as it comes), lengths, g"""
    c = FLOW_CASES[name]
    b, t, lengths = layout(c)
    return dict(z=recipes.seeded_randn(c["seed"], b, c["channels"], t) * mask_of(c), lengths=torch.tensor(lengths), g=_g(c))


def post_inputs(name):
    """-> y [B, spec, T] (padded frames NOT zero: the reference masks behind `pre`), lengths, g, the draw eps [B, inter, T]"""
    c = POST_CASES[name]
    b, t, lengths = layout(c)
    return dict(y=recipes.seeded_randn(c["seed"], b, c["spec"], t), lengths=torch.tensor(lengths), g=_g(c),
                eps=recipes.seeded_randn(9000 + c["seed"], b, c["inter"], t))


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 restatements, on a module's state dict (CPU tensors of any float dtype) and a case's inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _d(x):
    return None if x is None else x.double()


def te_ref64(name, sd, i):
    """-> x, m, logs [B, C, T] in fp64"""
    c = TE_CASES[name]
    d = V.Vits2Dims(n_vocab=N_VOCAB, inter_channels=c["inter"], hidden_channels=c["hidden"], filter_channels=c["filter"], n_heads=c["heads"],
                    n_layers=c["layers"], kernel_size=c["kernel"], window_size=WINDOW, gin_channels=c["gin"], cond_layer_idx=c["cond"])
    x, m, logs, _ = V.text_encoder(i["ids"], i["lengths"], {f"enc_p.{k}": v.double() for k, v in sd.items()}, d, g=_d(i["g"]))
    return x, m, logs


def flow_ref64(name, sd, i):
    """-> the reverse and the forward pass of z [B, channels, T] in fp64"""
    c = FLOW_CASES[name]
    d = flow_dims(c["channels"], c["hidden"], c["kernel"], c["wn_layers"], c["flows"], c["gin"])
    wts = {f"flow.{k}": v.double() for k, v in sd.items()}
    mask = mask_of(c).double()
    return V.flow_reverse(i["z"].double(), mask, wts, d, g=_d(i["g"])), flow_forward(i["z"].double(), mask, wts, d, g=_d(i["g"]))


def post_ref64(name, sd, i):
    """-> z, m, logs [B, inter, T] in fp64"""
    c = POST_CASES[name]
    return posterior_encoder({k: v.double() for k, v in sd.items()}, i["y"].double(), i["lengths"], _d(i["g"]), i["eps"].double(),
                             c["layers"], c["kernel"])[:3]
