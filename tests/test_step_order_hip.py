"""The launch sequence of one decode step, by name and in order, against a literal table.

csrc/api.hip composes a step's launches from four decisions (step_order: the cell, frame kernel or three launches, the overlap
level, the projection as a head role / the query as a role) and names them from one table (node_name).  bench.py keys its
per-launch byte model on these names (split at '+'), and the committed profiles carry them, so a sequence or a name that moves
must fail here.  The table below was taken from the library as it was when the sequences were fifteen literal tables, and
checked against them; between them the cases reach every one of the fifteen.

What Engine.profile_step reports beside a two-role step - each role alone, "...(alone)" - is a measurement and no part of it."""
import json
import os

import pytest
import torch

from oracle import tacotron_oracle as O

pytestmark = pytest.mark.gpu

# the names
P0, P1, F, A, Q, T_, D, J = "prenet0", "prenet1", "prenet", "lstm_att", "query", "attention", "lstm_dec", "proj"
FA, JF, JFA, TD, QTD = "prenet+lstm_att", "proj+prenet", "proj+prenet+lstm_att", "attention+lstm_dec", "query+attention+lstm_dec"

PROD = dict(d_mel=80, d_pre=128, d_ctx=64, h_att=128, h_dec=192)      # frame kernel, two-role launches, register-weight projection
PROD_THREE = dict(d_mel=24, r=2, d_pre=32, d_ctx=40, h_att=72, h_dec=88)  # the frame kernel does not cover d_mel = 24
TACO2_FRAME = dict(d_mel=80, r=1, d_pre=128, d_ctx=64, h_att=128, h_dec=128)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taco2_meta.json")) as _f:
    _g = json.load(_f)["dims"]
TACO2_GOLDEN = {k: _g[k] for k in ("d_mel", "r", "d_pre", "d_ctx", "h_att", "h_dec")}  # d_mel = 24: three launches

# options -> the sequence per (B, arithmetic), in the order (3, f32), (3, split_f16), (100, f32), (100, split_f16)
LEVEL2, LEVEL2Q, LEVEL1, LEVEL0 = (JFA, Q, TD), (JFA, QTD), (JFA, Q, T_, D), (JF, A, Q, T_, D)
PROD_TABLE = {
    "": (LEVEL2, LEVEL2, LEVEL1, LEVEL2Q),  # (exact fp32 runs level 1 from 97 to 128 utterances; the query role: split-fp16 from 64)
    "overlap=0": (LEVEL0,) * 4,
    "overlap=1": (LEVEL1,) * 4,
    "overlap=2": (LEVEL2, LEVEL2, LEVEL2, LEVEL2Q),
    "head_proj=0": ((FA, Q, TD, J), (FA, Q, TD, J), (FA, Q, T_, D, J), (FA, QTD, J)),
    "head_proj=1": (LEVEL2, LEVEL2, LEVEL1, LEVEL2Q),
    "query_role=1": (LEVEL2Q, LEVEL2Q, LEVEL1, LEVEL2Q),
    "query_role=1,overlap=2": (LEVEL2Q,) * 4,
    "head_proj=0,overlap=1": ((FA, Q, T_, D, J),) * 4,
    "head_proj=0,overlap=0": ((F, A, Q, T_, D, J),) * 4,
}
TACO2_TABLE = {  # (its attention pass follows both LSTMs: level 1 at the most, and no query role)
    "": ((JFA, D, Q, T_),) * 4,
    "overlap=0": ((JF, A, D, Q, T_),) * 4,
    "overlap=1": ((JFA, D, Q, T_),) * 4,
    "overlap=2": ((JFA, D, Q, T_),) * 4,
    "head_proj=0": ((FA, D, Q, T_, J),) * 4,
    "head_proj=1": ((JFA, D, Q, T_),) * 4,
    "head_proj=0,overlap=0": ((F, A, D, Q, T_, J),) * 4,
}
# without the frame kernel there is no two-role launch and no head role: no option moves the sequence
OPTIONS = ("", "overlap=0", "overlap=1", "overlap=2", "head_proj=0", "head_proj=1")
PROD_THREE_TABLE = {o: ((P0, P1, A, Q, T_, D, J),) * 4 for o in OPTIONS + ("query_role=1",)}
TACO2_GOLDEN_TABLE = {o: ((P0, P1, A, D, Q, T_, J),) * 4 for o in OPTIONS}

CELLS = {
    "prod": (PROD, False, PROD_TABLE),
    "prod_three_launches": (PROD_THREE, False, PROD_THREE_TABLE),
    "taco2_frame": (TACO2_FRAME, True, TACO2_TABLE),
    "taco2_golden": (TACO2_GOLDEN, True, TACO2_GOLDEN_TABLE),
}
COLUMNS = ((3, "f32"), (3, "split_f16"), (100, "f32"), (100, "split_f16"))


@pytest.mark.parametrize("cell", sorted(CELLS))
def test_launch_names_of_a_step_in_order(cell, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import hip_helpers as H
    from torch_tts_amd import _lib

    kw, taco2, table = CELLS[cell]
    dims = O.DecoderDims(**kw)
    wts = O.random_taco2_weights(dims, d_pre_hidden=128, seed=3) if taco2 else O.random_decoder_weights(dims, seed=5, nonzero_init_state=True)
    make = H.make_taco2_decoder if taco2 else H.make_decoder
    for options, want in table.items():
        monkeypatch.setenv("TTSDEC_OPTIONS", options)
        for (B, prec), names in zip(COLUMNS, want):
            dec = make(dims, wts)  # a new module = a new handle, which reads the options
            dec.precision = prec
            eng = dec.engine(torch.device("cuda:0"))
            for opt in filter(None, options.split(",")):
                k, v = opt.split("=")
                assert eng.get_option(k) == int(v), opt
            mem = O.synthetic_memory(B, 7, dims.d_ctx, seed=1).cuda()
            # (profile_step returns a dict keyed by name, in launch order: a sequence that repeated a name would show it once -
            # none of the sequences does, every name in a row of the tables is distinct)
            got = tuple(n for n in eng.profile_step(mem, 1, _lib.DROPOUT_OFF, None, 0) if not n.endswith("(alone)"))
            assert got == names, (cell, options, B, prec, got, names)
