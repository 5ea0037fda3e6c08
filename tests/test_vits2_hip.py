"""GPU parity of the VITS2 path: ttsvits_* through the drop-in modules against
(a) vectors from the reference's own blocks and (b) the CPU oracle at the ModelConfig-default sizes."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import vits2_oracle as V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-4, 1e-5


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f"{what}: max abs err {err.max().item():.3e} (ref max {b.abs().max().item():.3e}), {int(bad.sum())} elements out"


@pytest.fixture(scope="module")
def gv():
    z = np.load(os.path.join(HERE, "golden", "vits2_small.npz"))
    meta = json.load(open(os.path.join(HERE, "golden", "vits2_meta.json")))
    wts = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    cases = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("w/")}
    return {"wts": wts, "c": cases, "d": meta["dims"]}


def _text_encoder(d, wts):
    import torch_tts_amd as T

    te = T.vits2.TextEncoder(d["n_vocab"], d["inter_channels"], d["hidden_channels"], d["filter_channels"], d["n_heads"], d["n_layers"],
                             d["kernel_size"], 0.1, gin_channels=d.get("gin_channels", 0))
    sd = {k[len("enc_p."):]: v for k, v in wts.items() if k.startswith("enc_p.")}
    te.load_state_dict(sd, strict=True)
    return te.cuda().eval()


def _flow(d, wts):
    import torch_tts_amd as T

    fl = T.vits2.ResidualCouplingTransformersBlock(d["inter_channels"], d["flow_hidden"], d["flow_kernel"], 1, d["flow_wn_layers"],
                                                   n_flows=d["n_flows"], gin_channels=d.get("gin_channels", 0), use_transformer_flows=True)
    sd = {k[len("flow."):]: v for k, v in wts.items() if k.startswith("flow.")}
    missing, unexpected = fl.load_state_dict(sd, strict=False)
    assert not unexpected and all("post_transformer" in k for k in missing), (missing, unexpected)
    return fl.cuda().eval()


def test_text_encoder_golden(gv):
    c = gv["c"]
    te = _text_encoder(gv["d"], gv["wts"])
    with torch.no_grad():
        x, m, logs, mask = te(c["te/ids"].cuda(), c["te/lengths"].cuda())
    _close(x, c["te/x"], "x")
    _close(m, c["te/m"], "m")
    _close(logs, c["te/logs"], "logs")
    assert mask.shape == (3, 1, 13) and float(x[2, :, 1:].abs().max()) == 0.0


def test_flow_reverse_golden(gv):
    c = gv["c"]
    fl = _flow(gv["d"], gv["wts"])
    ymask = V.sequence_mask(c["flow/lengths"], 17).unsqueeze(1).float()
    with torch.no_grad():
        out = fl(c["flow/z"].cuda(), ymask.cuda(), reverse=True)
    _close(out, c["flow/out"], "flow out")


# (T = 300: ten key tiles and nineteen value groups, so the dk = 96 attention kernel's rings of 2 tiles / 2 groups per wave are
# refilled - at 120 tokens every wave's tiles fit the rings' first fill; T = 1000: the largest score tile that still fits LDS)
@pytest.mark.parametrize("B,T,lengths", [(4, 120, [120, 77, 31, 1]), (2, 37, None), (2, 300, [300, 161]), (1, 1000, [983])])
def test_text_encoder_default_dims_vs_oracle(B, T, lengths):
    d = V.Vits2Dims()
    wts = V.random_vits2_weights(d, seed=5)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, d.n_vocab, (B, T), generator=g)
    lens = torch.tensor(lengths if lengths else [T] * B)
    ox, om, ol, _ = V.text_encoder(ids, lens, wts, d)
    te = _text_encoder({**d.__dict__}, wts)
    with torch.no_grad():
        x, m, logs, _ = te(ids.cuda(), lens.cuda())
    _close(x, ox, "x")
    _close(m, om, "m")
    _close(logs, ol, "logs")


@pytest.mark.parametrize("B,T,lengths", [(4, 600, [600, 411, 87, 2]), (3, 50, None)])
def test_flow_reverse_default_dims_vs_oracle(B, T, lengths):
    d = V.Vits2Dims()
    wts = V.random_vits2_weights(d, seed=6)
    g = torch.Generator().manual_seed(3)
    z = torch.randn(B, d.inter_channels, T, generator=g)
    lens = torch.tensor(lengths if lengths else [T] * B)
    ymask = V.sequence_mask(lens, T).unsqueeze(1).float()
    ref = V.flow_reverse(z, ymask, wts, d)
    fl = _flow({**d.__dict__}, wts)
    with torch.no_grad():
        out = fl(z.cuda(), ymask.cuda(), reverse=True)
    # north_star's bar (1e-4 relative, 1e-5 absolute floor).  Through 4 coupling layers the fp32 ORACLE's own rounding
    # noise is 0.6 of that bar (measured against its fp64 run, tools/vits2_error_probe.py: 6.9e-6 on values near zero),
    # the HIP path's 0.3 - so the HIP path is held to the bar against the oracle evaluated in fp64, and to 2x the bar
    # against the fp32 oracle (two fp32 evaluations of the same function).
    ref64 = V.flow_reverse(z.double(), ymask.double(), {k: v.double() for k, v in wts.items()}, d).float()
    _close(out, ref64, "flow out vs fp64 oracle", rtol=1e-4, atol=1e-5)
    _close(out, ref, "flow out", rtol=2e-4, atol=2e-5)
    # padded frames are exactly zero in both (a value that cancels to 0 in one fp32 evaluation and to 1e-6 in the other is not
    # a difference: only values well away from zero are compared)
    big = ref.abs() > 1e-4
    assert torch.equal((out.cpu() != 0) & big, (ref != 0) & big)


def test_vits_modules_refuse_what_is_outside_the_path():
    import torch_tts_amd as T

    fl = T.vits2.ResidualCouplingTransformersBlock(192, 192, 5, 1, 4, use_transformer_flows=True).cuda().eval()
    x = torch.zeros(1, 192, 8, device="cuda")
    with torch.no_grad(), pytest.raises(NotImplementedError):
        fl(x, torch.ones(1, 1, 8, device="cuda"), reverse=False)
    with pytest.raises(NotImplementedError):
        T.vits2.ResidualCouplingTransformersBlock(192, 192, 5, 1, 4, use_transformer_flows=False)


def test_text_encoder_sequences_shorter_than_the_window(gv):
    c = gv["c"]
    te = _text_encoder(gv["d"], gv["wts"])
    for Ts in (1, 3):
        with torch.no_grad():
            x, _, _, _ = te(c[f"short{Ts}/ids"].cuda(), c[f"short{Ts}/lengths"].cuda())
        _close(x, c[f"short{Ts}/x"], f"x T={Ts}")


def test_flow_reverse_long_sequence_uses_the_scalar_attention_fallback():
    """T = 1300 frames does not fit the matrix-core attention's score tile in LDS: the scalar kernel runs."""
    d = V.Vits2Dims(n_flows=1)
    wts = V.random_vits2_weights(d, seed=9)
    g = torch.Generator().manual_seed(4)
    B, T = 1, 1300
    z = torch.randn(B, d.inter_channels, T, generator=g)
    lens = torch.tensor([T - 37])
    ymask = V.sequence_mask(lens, T).unsqueeze(1).float()
    ref64 = V.flow_reverse(z.double(), ymask.double(), {k: v.double() for k, v in wts.items()}, d).float()
    fl = _flow({**d.__dict__}, wts)
    with torch.no_grad():
        out = fl(z.cuda(), ymask.cuda(), reverse=True)
    _close(out, ref64, "flow out (T=1300)", rtol=1e-4, atol=1e-5)


# ---- speaker conditioning (gin_channels > 0) ----
def test_speaker_conditioning_golden(gv):
    """g [B, gin, 1] through both entry points against outputs of models.TextEncoder / ResidualCouplingTransformersBlock themselves
    (tests/golden/make_golden_vits2.py, the g/* arrays); g=None on the same conditioned modules takes the unconditioned branch."""
    z = np.load(os.path.join(HERE, "golden", "vits2_small.npz"))
    wg = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("wg/")}
    dg = json.load(open(os.path.join(HERE, "golden", "vits2_meta.json")))["dims_g"]
    c = gv["c"]
    g = c["g/spk"].cuda()
    ymask = V.sequence_mask(c["flow/lengths"], 17).unsqueeze(1).float().cuda()
    for prec in ("split_f16", "f32"):
        te, fl = _text_encoder(dg, wg), _flow(dg, wg)
        te.precision = fl.precision = prec
        with torch.no_grad():
            x, m, logs, _ = te(c["te/ids"].cuda(), c["te/lengths"].cuda(), g=g)
            x0, _, _, _ = te(c["te/ids"].cuda(), c["te/lengths"].cuda())
            out = fl(c["flow/z"].cuda(), ymask, g=g, reverse=True)
            out0 = fl(c["flow/z"].cuda(), ymask, reverse=True)
            out2 = fl(c["flow/z"].cuda(), ymask, g=g[:, :, 0], reverse=True)  # ([B, gin] is accepted as well)
        _close(x, c["g/te/x"], f"{prec} x"); _close(m, c["g/te/m"], f"{prec} m"); _close(logs, c["g/te/logs"], f"{prec} logs")
        _close(x0, c["g/te/x_no_g"], f"{prec} x without g")
        _close(out, c["g/flow/out"], f"{prec} flow out"); _close(out0, c["g/flow/out_no_g"], f"{prec} flow out without g")
        assert torch.equal(out, out2)


@pytest.mark.parametrize("B,T,lengths", [(3, 200, [200, 131, 7])])
def test_speaker_conditioning_default_dims_vs_oracle(B, T, lengths):
    """ModelConfig-default widths with the multi-speaker gin_channels = 256 (cli.py) against the oracle, fp32 and fp64."""
    d = V.Vits2Dims(gin_channels=256)
    wts = V.random_vits2_weights(d, seed=8)
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(B, d.inter_channels, T, generator=gen)
    ids = torch.randint(0, d.n_vocab, (B, T), generator=gen)
    g = torch.randn(B, d.gin_channels, 1, generator=gen)
    lens = torch.tensor(lengths)
    ymask = V.sequence_mask(lens, T).unsqueeze(1).float()
    w64 = {k: v.double() for k, v in wts.items()}
    ref = V.flow_reverse(z, ymask, wts, d, g=g)
    ref64 = V.flow_reverse(z.double(), ymask.double(), w64, d, g=g.double()).float()
    assert float((ref - V.flow_reverse(z, ymask, wts, d)).abs().max()) > 1e-2
    fl = _flow({**d.__dict__}, wts)
    te = _text_encoder({**d.__dict__}, wts)
    ox, om, ol, _ = V.text_encoder(ids, lens, wts, d, g=g)
    with torch.no_grad():
        out = fl(z.cuda(), ymask.cuda(), g=g.cuda(), reverse=True)
        x, m, logs, _ = te(ids.cuda(), lens.cuda(), g=g.cuda())
    _close(out, ref64, "flow out vs fp64 oracle", rtol=1e-4, atol=1e-5)
    _close(out, ref, "flow out", rtol=2e-4, atol=2e-5)
    _close(x, ox, "x"); _close(m, om, "m"); _close(logs, ol, "logs")


def test_speaker_conditioning_refusals():
    import torch_tts_amd as T

    fl = T.vits2.ResidualCouplingTransformersBlock(16, 24, 5, 1, 3, n_flows=2, gin_channels=8, use_transformer_flows=True).cuda().eval()
    x, mk = torch.zeros(2, 16, 9, device="cuda"), torch.ones(2, 1, 9, device="cuda")
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            fl(x, mk, g=torch.zeros(2, 8, 9, device="cuda"), reverse=True)  # time-varying g
        with pytest.raises(ValueError):
            fl(x, mk, g=torch.zeros(2, 4, 1, device="cuda"), reverse=True)  # wrong width
        plain = T.vits2.ResidualCouplingTransformersBlock(16, 24, 5, 1, 3, n_flows=2, use_transformer_flows=True).cuda().eval()
        with pytest.raises(ValueError):
            plain(x, mk, g=torch.zeros(2, 8, 1, device="cuda"), reverse=True)  # g for a module built without gin_channels
    with pytest.raises(AssertionError):
        T.vits2.TextEncoder(11, 16, 32, 48, 2, 2, 3, 0.1, gin_channels=8)  # attentions.py:50-52: cond_layer_idx 2 needs 3 layers


# ---- bench.py's VITS2 shapes (BASELINE.json configs[4]): TextEncoder [64, 120], reverse flow [64, 192, 600] ----
# At 64 x 600 = 38400 rows the flow's fp32 GEMMs take the 64x64 tile with the generic epilogue (csrc/decode_kernels.hip
# launch_gemm_cfg: ceil(M / 64) * ceil(N / 64) >= 512), split-fp16 the 128x128 and the lean short-K 64x64 tiles (M >= 2048);
# the TextEncoder's 7680 rows move its qkv / FFN / proj GEMMs to the 64x64 tile too.  None of these is reached at the sizes
# above.  Utterances never interact, so the GPU runs the whole batch and the oracle a sample of it.
_BENCH_B, _BENCH_TX, _BENCH_TY = 64, 120, 600
_BENCH_VITS2 = {}


def _bench_vits2_case(kind):
    """Weights, inputs, lengths, the sampled utterances and the oracle's outputs on them (fp32 TextEncoder, fp32 and fp64 flow);
    kind "full": every utterance full length, as bench.py runs; "ragged": lengths 1 and full among the sample, the others' last
    valid row inside a 64-row tile."""
    if kind in _BENCH_VITS2:
        return _BENCH_VITS2[kind]
    import hip_helpers as H

    d = V.Vits2Dims()
    wts = V.random_vits2_weights(d, seed=6)  # (post weights non-zero: the coupling does real work, as bench.py arranges)
    assert float(wts["flow.flows.0.post.weight"].abs().max()) > 0.0
    B, Tx, Ty = _BENCH_B, _BENCH_TX, _BENCH_TY
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, d.n_vocab, (B, Tx), generator=gen)
    z = torch.randn(B, d.inter_channels, Ty, generator=gen)
    bounds = H.last_tile_rows(B * Ty, 64, 128)
    sample = H.sample_utterances(B, Ty, bounds + [(r // Tx) * Ty for r in H.last_tile_rows(B * Tx, 64, 128)], k_random=3, seed=7)
    xl, yl = torch.full((B,), Tx), torch.full((B,), Ty)
    if kind == "ragged":
        xl = torch.randint(1, Tx + 1, (B,), generator=gen)
        yl = torch.randint(1, Ty + 1, (B,), generator=gen)
        xl[sample[0]], yl[sample[0]] = Tx, Ty
        xl[sample[-1]], yl[sample[-1]] = 1, 1
        for b in sample[1:-1]:  # the last valid row 20 rows into a 64-row tile of the [B * T] matrix
            xl[b] = next(n for n in range(Tx, 0, -1) if (b * Tx + n - 1) % 64 == 20)
            yl[b] = next(n for n in range(Ty, 0, -1) if (b * Ty + n - 1) % 64 == 20)
    ymask = V.sequence_mask(yl, Ty).unsqueeze(1).float()
    s = torch.tensor(sample)
    w64 = {k: v.double() for k, v in wts.items()}
    ox, om, ol, _ = V.text_encoder(ids[s], xl[s], wts, d)
    oz = V.flow_reverse(z[s], ymask[s], wts, d)
    oz64 = V.flow_reverse(z[s].double(), ymask[s].double(), w64, d).float()
    _BENCH_VITS2[kind] = dict(d=d, wts=wts, ids=ids, z=z, xl=xl, yl=yl, ymask=ymask, sample=sample, ox=ox, om=om, ol=ol, oz=oz, oz64=oz64)
    return _BENCH_VITS2[kind]


@pytest.mark.parametrize("kind", ["full", "ragged"])
@pytest.mark.parametrize("prec", ["f32", "split_f16"])
def test_vits2_at_the_benchmarked_batch_vs_oracle(prec, kind):
    c = _bench_vits2_case(kind)
    d, s = c["d"], torch.tensor(c["sample"])
    te, fl = _text_encoder({**d.__dict__}, c["wts"]), _flow({**d.__dict__}, c["wts"])
    te.precision = fl.precision = prec
    with torch.no_grad():
        x, m, logs, _ = te(c["ids"].cuda(), c["xl"].cuda())
        out = fl(c["z"].cuda(), c["ymask"].cuda(), reverse=True)
    assert x.shape == (_BENCH_B, d.hidden_channels, _BENCH_TX) and out.shape == (_BENCH_B, d.inter_channels, _BENCH_TY)
    x, m, logs, out = (t.cpu()[s] for t in (x, m, logs, out))
    print(f"{prec} {kind}: utterances {c['sample']}, text lengths {c['xl'][s].tolist()}, frame lengths {c['yl'][s].tolist()}")
    _close(x, c["ox"], f"{prec} x")
    _close(m, c["om"], f"{prec} m")
    _close(logs, c["ol"], f"{prec} logs")
    _close(out, c["oz64"], f"{prec} flow out vs fp64 oracle", rtol=1e-4, atol=1e-5)
    _close(out, c["oz"], f"{prec} flow out", rtol=2e-4, atol=2e-5)
    for i, b in enumerate(c["sample"]):  # padded frames are exactly zero (the oracle's are)
        nx, ny = int(c["xl"][b]), int(c["yl"][b])
        for name, t in (("x", x), ("m", m), ("logs", logs)):
            assert not bool(t[i, :, nx:].ne(0).any()), (prec, kind, b, name)
        assert not bool(out[i, :, ny:].ne(0).any()), (prec, kind, b, "flow out")
