"""GPU parity at the corners of the dims that ttsenc_style_create accepts (tests/style_corner_cases.py): every case and layout
through csrc/style.hip against the module's own ``_stock_forward`` in fp64 on the CPU (tests/test_style_hip.check; the same fp32
weights and inputs in .double(); tests/test_style_corners_host.py shows that it is the reference at these dims and that the fp32
stock forward is within a quarter of the bar), under the project's bar rtol 1e-4 / atol 1e-5; the same bits through the module's
forward with exactly one engine made (no quiet fall-back); without lengths; S6's rows 0, 64 and 128 of the batch of 129 alone
(another LSTM tile, so against the oracle, not bit for bit: tests/test_style_hip.py's docstring excludes that); the same bits twice.

MEASURED on an MI355X (256 CUs), from this module's printout (profiles/style_durdisc_corners_parity.txt holds every figure, the
fp32 CPU error beside it).  Worst |err| / (atol + rtol |ref|) over enc_out, x and kl, with lengths / without:
  S1 0.003 / 0.003   S2 0.007 / 0.015   S3 0.010 / 0.005   S4 0.041 / 0.030   S5 0.011 / 0.010   S8 0.025 / 0.020
  S6 B = 129 0.011, B = 97 0.010, rows 0 / 64 / 128 alone 0.008 / 0.005 / 0.007   S7 0.009
The fp32 CPU forward lies at 0.001 - 0.028 of the bar on the same outputs."""
import copy

import pytest
import torch

import style_corner_cases as K
from test_style_corners_host import module, ref64
from test_style_hip import DEV, check, hip_outputs
from test_style_host import bar_ratio

pytestmark = pytest.mark.gpu
_built = {}  # case -> the module on the GPU, shared by the tests of this module


@pytest.fixture(scope="module", autouse=True)
def _drop_modules():
    yield
    _built.clear()


def device_module(name):
    if name not in _built:
        _built[name] = copy.deepcopy(module(name)).to(DEV)
    return _built[name]


def same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name,i", K.all_layouts())
def test_parity_forward_and_determinism(name, i):
    m, md = module(name), device_module(name)
    x, lengths, eps = K.inputs(name, i)
    B = x.shape[0]
    c = K.CASES[name]
    hip = check(K.key(name, i), m, x, lengths, eps, m_dev=md)
    assert same(hip, hip_outputs(md, x, lengths, eps)), "a second call gave other bits"
    # through the module's forward: the same bits in the reference's output shapes, on one engine
    with torch.no_grad():
        if c["kind"] == "encoder":
            assert torch.equal(md(x.to(DEV), lengths), hip["enc_out"])
        else:
            xo, extra = md(x.to(DEV), lengths, None if eps is None else eps.to(DEV))
            assert xo.shape == (B, 1, c["d_emb"]) and torch.equal(xo[:, 0], hip["x"])
            if "d_vae" in c:
                assert extra["kl"].shape == ((B, 1, c["d_vae"]) if c["kind"] == "gstvae" else (B, c["d_vae"]))
                assert torch.equal(extra["kl"].reshape(B, -1), hip["kl"])
            else:
                assert extra == {}
    assert len(md._engines.engines()) == 1  # (the HIP path ran: there is no quiet fall-back)
    if name in K.NO_LENGTHS:  # every row runs all T' steps, over the zero frames behind its end too
        free = check(K.key(name, i) + ", no lengths", m, x, None, eps, m_dev=md)
        assert same(free, hip_outputs(md, x, None, eps))


def test_rows_of_the_largest_batch_alone():
    """S6 at B = 129 runs the LSTM on the 64 x 16 tile; rows 0 (first of block 0), 64 (first of block 1) and 128 (the only row of
    the ragged block 2) alone run on the 32 x 8 tile.  Each has at least 2^3 frames, so its oracle alone is its row of the batch's
    oracle (tests/test_style_hip.py's reach argument); both HIP results are within the bar of it."""
    m, md = module("S6"), device_module("S6")
    x, lengths, eps = K.inputs("S6", 0)
    assert x.shape[0] == 129
    batch, oracle = hip_outputs(md, x, lengths, eps), ref64("S6", 0)
    for b in (0, 64, 128):
        n = int(lengths[b])
        assert n >= 8
        alone = check(f"S6 row {b} alone ({n} frames)", m, x[b:b + 1, :n], lengths[b:b + 1], eps[b:b + 1], m_dev=md)
        for out, r64 in oracle.items():
            r64 = r64.reshape(batch[out].shape)
            e_alone, e_batch = bar_ratio(alone[out], r64[b:b + 1]), bar_ratio(batch[out][b:b + 1], r64[b:b + 1])
            print(f"S6 row {b} {out}: alone {e_alone:.4f} of the bar from the batch's oracle, in the batch {e_batch:.4f}")
            assert e_alone <= 1.0 and e_batch <= 1.0, (b, out, e_alone, e_batch)
    assert len(md._engines.engines()) == 1
