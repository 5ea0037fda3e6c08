"""GPU parity of the VITS2 row GEMMs on every tile and K-walk length the dispatcher gives them (tests/vits2_tile_cases.py): every case
through torch_tts_amd.vits2.TextEncoder, ResidualCouplingTransformersBlock (reverse and forward_cl) and PosteriorEncoder at each of
its layouts, in exact fp32 and in split-fp16, against the fp64 restatements of oracle/vits2_oracle.py and tests/test_vc_host.py on
the sampled utterances under the bar tests/test_vits2_hip.py and tests/test_vc_hip.py hold these families to, rtol 1e-4 / atol 1e-5
on every element of every output, padded frames exactly zero.  tests/test_vits2_tiles_host.py shows which tile edge, walk length
and switch side each case reaches (its census), that the restatements are the reference at these dims, that their own fp32 is
within half of the bar at these shapes, and that the bar would notice a dropped K stage or column tile.

The worst fraction of the bar over a case's outputs, as measured on an MI355X (f32 / split_f16; every run prints them per output):
(the worst of a case's layouts; the sampled utterances above 5000 rows):
  W8 0.416 / 0.364 (a LayerNorm over eight values: the fp32 restatement itself is at 0.39)   W16 0.096 / 0.111   W24 0.246 / 0.232
  W40 0.240 / 0.210   W48 0.300 / 0.290   X2 0.290 / 0.412   X3 0.142 / 0.090
  RF 0.094 / 0.061
  RQ 0.048 / 0.036   N1 0.027 / 0.028   S1 0.059 / 0.031   L24 0.022 / 0.017   L40 0.022 / 0.017   L72 0.020 / 0.026   L104 0.020 / 0.018
  L136 0.017 / 0.019   L168 0.019 / 0.019
The switches, one side against the other as a fraction of twice the bar: 2047 | 2048 rows in split-fp16 0 (the same bits: the
64 x 64, lean and 128 x 128 split tiles add a row's k16 products in one order); 10 880 | 10 881 rows in exact fp32 0.027 (other
bits: the 32 x 32 tile splits K over four waves).
No tile was wrong."""
import pytest
import torch

import vits2_tile_cases as K
from hip_helpers import assert_workspace_fits
from torch_tts_amd import vits2
from torch_tts_amd.engine import Handle

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5
PRECISIONS = ["f32", "split_f16"]
RUN_IDS = [K.run_id(r) for r in K.RUNS]
OUTPUTS = K.OUTPUTS
_built = {}  # (family, case) -> the drop-in on the GPU; (family, case, layout, precision) -> its outputs on the whole batch


@pytest.fixture(scope="module", autouse=True)
def _drop_modules():
    yield
    _built.clear()


def once(key, make):
    if key not in _built:
        _built[key] = make()
    return _built[key]


def fraction(a, b, scale=1.0):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(((a - b).abs() / (scale * (ATOL + RTOL * b.abs()))).max())


def module(fam, name):
    return once((fam, name), lambda: K.make(vits2, fam, name).cuda().eval())


def _dev(t):
    return None if t is None else t.cuda()


def run(fam, name, li, precision, i=None):
    """The case's outputs ([B, C, T], on the CPU) at layout li on inputs `i` (None: the layout's own)."""
    mod = module(fam, name)
    layout = K.LAYOUTS[name][li]
    i = K.refs(fam, name, li)[0] if i is None else i
    lengths, g = i["lengths"].cuda(), _dev(i["g"])
    mod.precision = precision
    try:
        with torch.no_grad():
            if fam == "te":
                x, m, logs, _ = mod(i["ids"].cuda(), lengths, g=g)
                out = dict(x=x, m=m, logs=logs)
            elif fam == "flow":
                z = i["z"].cuda()
                rev = mod(z, K.mask_of(layout).cuda(), g=g, reverse=True)
                fwd = mod.forward_cl(z.transpose(1, 2).contiguous(), lengths, g).transpose(1, 2)
                out = dict(rev=rev, fwd=fwd)
            else:
                z, m, logs, _ = mod(i["y"].cuda(), lengths, g=g, noise=i["eps"].cuda())
                out = dict(z=z, m=m, logs=logs)
        return {k: v.contiguous().cpu() for k, v in out.items()}
    finally:
        mod.precision = "f32"


def batch(fam, name, li, precision):
    return once((fam, name, li, precision), lambda: run(fam, name, li, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("r", K.RUNS, ids=RUN_IDS)
def test_parity_with_the_fp64_restatement(r, precision):
    fam, name, li = r
    _, _, lengths = K.LAYOUTS[name][li]
    _, rows, ref = K.refs(fam, name, li)
    out = batch(fam, name, li, precision)
    worst = {k: fraction(out[k][rows], ref[k]) for k in OUTPUTS[fam]}  # every figure before the first assertion
    print(f"{K.run_id(r)} {precision}: worst |err| / (atol + rtol |ref|) over utterances {rows} = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k in OUTPUTS[fam]:
        assert bool(torch.isfinite(out[k]).all()), (name, precision, k)
        torch.testing.assert_close(out[k][rows].double(), ref[k], rtol=RTOL, atol=ATOL, msg=lambda m: f"{K.run_id(r)} {precision} {k}: {m}")
        for b, n in enumerate(lengths):  # padded frames: exactly zero, in every utterance
            assert float(out[k][b, :, n:].abs().sum()) == 0.0, (name, precision, k, b)


def _replaced(fam, name, li, which):
    """The layout's inputs with the contents of the utterances `which` replaced: same shapes, lengths and so tiles.  (ids: rolled by
    a frame; the float tensors: channels reversed and negated, which keeps z's padded frames zero.)"""
    i = dict(K.refs(fam, name, li)[0])
    for k in ("ids", "z", "y", "eps", "g"):
        if i.get(k) is not None:
            t = i[k].clone()
            for nb in which:
                t[nb] = (i[k][nb] + 1) % K.N_VOCAB if k == "ids" else -i[k][nb].flip(0)
            i[k] = t
    return i


ISOLATION = [("te", "W48", 0), ("te", "W24", 1), ("te", "X2", 0), ("te", "X2", 1), ("te", "X3", 0), ("flow", "RF", 0), ("flow", "RF", 1),
             ("post", "RQ", 0), ("post", "RQ", 1), ("post", "L168", 0), ("post", "N1", 0)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("r", ISOLATION, ids=[K.run_id(r) for r in ISOLATION])
def test_twice_and_beside_other_neighbours(r, precision):
    """Two identical calls give the same bits; with the contents of utterances b - 1 and b + 1 replaced (same shapes, so the same
    tiles), utterance b keeps its bits.  These layouts' utterances are longer than a row tile (B <= 31, so that every boundary lies
    inside a tile of every height), so none starts inside the last row tile: the last utterance holds that tile whole.  b is
    the one in front of it - its second neighbour is the ragged tile's utterance - and then the last one itself, beside a replaced
    b.  (An utterance alone need not have the bits it has in the batch: in these families the tile, and so the summation order,
    depends on M.)"""
    fam, name, li = r
    B, T, _ = K.LAYOUTS[name][li]
    out = batch(fam, name, li, precision)
    again = run(fam, name, li, precision)
    for k in OUTPUTS[fam]:
        assert torch.equal(out[k], again[k]), f"{K.run_id(r)} {precision} {k}: two identical calls differ"
    BM = max(K.TILES[t][0] for g, t, _ in K.tiles_of(fam, name, K.LAYOUTS[name][li], precision) if g[2] == B * T)
    assert (B - 1) * T < (B * T - 1) // BM * BM and B >= 4  # the last utterance starts in front of the last row tile
    own = K.refs(fam, name, li)[0]
    key = "ids" if fam == "te" else "z" if fam == "flow" else "y"
    for b, which in ((B - 2, (B - 3, B - 1)), (B - 1, (B - 2,))):
        i = _replaced(fam, name, li, which)
        assert torch.equal(i[key][b], own[key][b]) and all(not torch.equal(i[key][nb], own[key][nb]) for nb in which)
        moved = run(fam, name, li, precision, i)
        for k in OUTPUTS[fam]:
            assert torch.equal(moved[k][b], out[k][b]), f"{K.run_id(r)} {precision} {k}: utterance {b} depends on its neighbours"
            assert all(not torch.equal(moved[k][nb], out[k][nb]) for nb in which), (k, which)


@pytest.mark.parametrize("precision,lo", [("split_f16", 0), ("f32", 2)], ids=["2047|2048-split_f16", "10880|10881-f32"])
def test_both_sides_of_a_switch_agree(precision, lo):
    """The same module at M and M + 1 rows across a tile switch (the upper side's last frame is padding: both compute the same
    rows from the same frames): each side is within the bar of the fp64 restatement, and the two agree with each other over their
    common prefix within twice the bar - the bits may differ, the tiles do."""
    fam, name = "post", K.SWITCH_CASE
    a, b = batch(fam, name, lo, precision), batch(fam, name, lo + 1, precision)
    n = K.LAYOUTS[name][lo][1]
    assert K.LAYOUTS[name][lo + 1][1] == n + 1 and K.LAYOUTS[name][lo][2] == K.LAYOUTS[name][lo + 1][2] == (n,)
    ta, tb = ({t for _, t, _ in K.tiles_of(fam, name, K.LAYOUTS[name][li], precision)} for li in (lo, lo + 1))
    assert ta != tb
    worst = {k: fraction(a[k], b[k][:, :, :n], 2.0) for k in OUTPUTS[fam]}
    print(f"{name} {precision} {n} | {n + 1} rows: the two sides differ by " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of twice the bar; "
          + ", ".join(f"{k} {'same bits' if torch.equal(a[k], b[k][:, :, :n]) else 'other bits'}" for k in OUTPUTS[fam]))
    for li, out in ((lo, a), (lo + 1, b)):
        _, rows, ref = K.refs(fam, name, li)
        for k in OUTPUTS[fam]:
            torch.testing.assert_close(out[k][rows].double(), ref[k], rtol=RTOL, atol=ATOL, msg=lambda m: f"{name} {precision} layout {li} {k}: {m}")
    for k in OUTPUTS[fam]:
        torch.testing.assert_close(a[k].double(), b[k][:, :, :n].double(), rtol=2 * RTOL, atol=2 * ATOL, msg=lambda m: f"{name} {precision} {k}: {m}")
        assert float(b[k][:, :, n:].abs().sum()) == 0.0


@pytest.mark.parametrize("r", [("te", "X2", 0), ("flow", "RF", 0), ("post", "RQ", 0)], ids=["X2", "RF", "RQ"])
def test_workspace_fits_in_split_fp16(monkeypatch, r):
    """One split-fp16 large-tile case per family (planes and fp32 buffers both live; X2: exact layers between split ones): the
    reported bytes hold the call, and the result does not depend on the workspace."""
    fam, name, li = r
    want = batch(fam, name, li, "split_f16")
    got = []

    def call():
        got.append(run(fam, name, li, "split_f16"))
        return torch.cat([got[-1][k].reshape(-1) for k in OUTPUTS[fam]]).cuda()

    assert_workspace_fits(monkeypatch, Handle, "workspace", lambda eng, kind, nbytes: nbytes, call)
    for k in OUTPUTS[fam]:
        assert torch.equal(got[0][k], want[k]), f"{name} {k}: the result depends on the workspace"


@pytest.mark.parametrize("name", ["X2", "X3"])
def test_the_mixed_chain_really_runs_mixed(name):
    """Had split-fp16 fallen back as a whole, the two precisions would agree in every bit (both are within the bar:
    test_parity_with_the_fp64_restatement)."""
    for li in range(len(K.LAYOUTS[name])):
        a, b = batch("te", name, li, "split_f16"), batch("te", name, li, "f32")
        assert not torch.equal(a["x"], b["x"]) and not torch.equal(a["m"], b["m"])
