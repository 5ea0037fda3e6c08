"""GPU parity of each VITS2 attention kernel (csrc/vits2.hip: mha_kernel, mha_mfma_kernel<DKH>, mha_flash_kernel<DK>) at its own
edges, through TextEncoder and ResidualCouplingTransformersBlock on the inputs of tests/vits2_attention_cases.py.  What those
inputs make a kernel do - which kernel runs, where the flash kernel's lazy maximum moves and rescales - is asserted on the CPU in
tests/test_vits2_attention_host.py; every test here asserts the kernel it claims to reach before it runs.

The bar for every case: the HIP output against the oracle evaluated in fp64 at rtol 1e-4 / atol 1e-5, against the fp32 oracle at
twice that; padded frames exactly zero (wherever the oracle's are: all but the channels the flow passes through); every output
finite.  Each test prints its error in units of the bar."""
import pytest
import torch

import vits2_attention_cases as A

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
_ids = A.spec_id


def _check(what, out, ref64, ref32, lengths):
    """out, ref* [B, C, T]"""
    out = out.detach().cpu()
    assert out.shape == ref64.shape, (what, out.shape, ref64.shape)
    assert bool(torch.isfinite(out).all()), f"{what}: non-finite output"
    for b, n in enumerate(lengths):  # (the flow hands its first half through as it came; everything computed is masked)
        assert torch.equal(out[b, :, n:] != 0, ref32[b, :, n:] != 0), f"{what}: utterance {b}: padded frames are not exactly zero where the oracle's are"
    u64, u32 = A.bar_units(out, ref64), A.bar_units(out, ref32)
    print(f"{what}: {u64:.3f} of the bar against the fp64 oracle, {u32 / 2:.3f} of the doubled bar against the fp32 oracle")
    assert u64 <= 1.0, f"{what}: {u64:.3f} of the bar (rtol {A.RTOL}, atol {A.ATOL}) against the fp64 oracle"
    assert u32 <= 2.0, f"{what}: {u32:.3f} of the bar against the fp32 oracle (2 allowed)"


def _run_flow(case, precision):
    import torch_tts_amd as T

    d = case.dims
    fl = T.vits2.ResidualCouplingTransformersBlock(d.inter_channels, d.flow_hidden, d.flow_kernel, 1, d.flow_wn_layers, n_flows=d.n_flows,
                                                   use_transformer_flows=True)
    sd = {k[len("flow."):]: v for k, v in case.wts.items() if k.startswith("flow.")}
    missing, unexpected = fl.load_state_dict(sd, strict=False)
    assert not unexpected and all("post_transformer" in k for k in missing), (missing, unexpected)
    fl = fl.cuda().eval()
    fl.precision = precision
    with torch.no_grad():
        out = fl(case.z.cuda(), case.ymask.cuda(), reverse=True)
    _check(f"{case.name} {precision} [{case.choice(precision)}]", out, case.reference(F64), case.reference(F32), case.lengths)


def _run_text(case, precision):
    import torch_tts_amd as T

    d = case.dims
    te = T.vits2.TextEncoder(d.n_vocab, d.inter_channels, d.hidden_channels, d.filter_channels, d.n_heads, d.n_layers, d.kernel_size, 0.1)
    if d.window_size != te.encoder.window_size:  # (before the weights are loaded and before the first forward: _dims() reads it from here)
        te.encoder = T.vits2.Encoder(d.hidden_channels, d.filter_channels, d.n_heads, d.n_layers, d.kernel_size, 0.1, window_size=d.window_size)
    te.load_state_dict({k[len("enc_p."):]: v for k, v in case.wts.items() if k.startswith("enc_p.")}, strict=True)
    te = te.cuda().eval()
    te.precision = precision
    assert te._dims()["window_size"] == d.window_size
    with torch.no_grad():
        outs = te(case.ids.cuda(), torch.tensor(case.lengths).cuda())[:3]
    for name, out, r64, r32 in zip(("x", "m", "logs"), outs, case.reference(F64), case.reference(F32)):
        _check(f"{case.name} {precision} [{case.choice(precision)}] {name}", out, r64, r32, case.lengths)


# ---- the flash kernel (split_f16, no window) ----
@pytest.mark.parametrize("spec", A.FLASH_MAIN, ids=_ids)
def test_flash_kernel_rescales_under_a_moving_maximum(spec):
    """flash<16 / 32 / 48 / 64> x {scaled: alpha in (0, 1) for some lanes at every tile after the first, the ragged one included;
    ascending: every lane at every valid tile; descending: never}.  4 (utterance, head) pairs: the plain grid order."""
    case = A.flow_case(*spec)
    assert case.choice("split_f16") == f"flash<{spec[1] // 4}>" and A.flash_grid_order(len(case.lengths), 2) == "plain"
    _run_flow(case, "split_f16")


@pytest.mark.parametrize("spec", A.FLASH_REMAP, ids=_ids)
def test_flash_kernel_under_the_xcd_remap(spec):
    """8 pairs: workgroup ids go through the XCD remap; lengths 97 and 1 leave whole workgroups with masked queries only."""
    case = A.flow_case(*spec)
    assert case.choice("split_f16") == "flash<48>" and A.flash_grid_order(len(case.lengths), 2) == "remap"
    _run_flow(case, "split_f16")


@pytest.mark.parametrize("spec", A.FLASH_SHORT, ids=_ids)
def test_flash_kernel_on_one_and_two_tiles(spec):
    """T = 1, 32: one tile; 33: a second tile of one key; 129: the second workgroup has one active wave and three that only stage.
    B = 3 (6 pairs: plain order), one utterance of length 1."""
    case = A.flow_case(*spec)
    assert case.choice("split_f16") == "flash<16>" and A.flash_grid_order(len(case.lengths), 2) == "plain" and 1 in case.lengths
    _run_flow(case, "split_f16")


# ---- the exact-fp32 kernels without a window, under the same large scores ----
_EXACT_KERNEL = {32: "mfma<4>", 64: "mfma<8>", 128: "scalar", 192: "mfma<24>", 256: "scalar", 384: "mfma<48>"}


@pytest.mark.parametrize("spec", A.EXACT_F32, ids=_ids)
def test_exact_fp32_kernels_under_large_scores(spec):
    """mfma<4>, mfma<8> (T = 300, and 600 where each wave's ring of 4 key tiles refills), scalar at dk 32 and 64, mfma<24>, mfma<48>
    without a window."""
    case = A.flow_case(*spec)
    assert case.choice("f32") == _EXACT_KERNEL[spec[1]]
    _run_flow(case, "f32")


@pytest.mark.parametrize("spec", A.EXACT_SPLIT, ids=_ids)
def test_mfma_kernels_feed_the_split_output_gemm(spec):
    """split_f16 at dk 8 and 96, which the flash kernel is not built for: mfma<4> / mfma<48> write the out_p planes conv_o reads."""
    case = A.flow_case(*spec)
    assert case.choice("split_f16") == _EXACT_KERNEL[spec[1]] and _EXACT_KERNEL[spec[1]].startswith("mfma")
    _run_flow(case, "split_f16")


# ---- the relative-position window (TextEncoder) ----
_TEXT_KERNEL = {16: "mfma<4>", 32: "mfma<8>", 64: "scalar", 96: "mfma<24>", 192: "mfma<48>"}


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("spec", A.TEXT_WIDTHS + A.TEXT_SCALED, ids=_ids)
def test_windowed_attention_at_every_head_width(spec, precision):
    """hidden 16, 32, 64, 96, 192 with 2 heads and window 4: mfma<4>, mfma<8>, scalar (dk 32, windowed, T > 16), mfma<24> with a
    window, mfma<48>; hidden 192 also with conv_q scaled.  Lengths 300, 161, 5: the shortest is inside one window."""
    case = A.text(*spec)
    assert case.choice(precision) == _TEXT_KERNEL[spec[0]] and case.dims.window_size == 4
    _run_text(case, precision)


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("spec", A.TEXT_LDS_EDGE, ids=_ids)
def test_windowed_attention_at_the_lds_boundary(spec, precision):
    """dk 96, window 4: T = 1165 is the last length whose score tile fits the mfma kernel's LDS, 1166 the first the scalar one takes."""
    case = A.text(*spec)
    assert case.choice(precision) == {1165: "mfma<48>", 1166: "scalar"}[case.T]
    _run_text(case, precision)


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("spec", A.TEXT_WINDOWS, ids=_ids)
def test_windowed_attention_at_other_window_widths(spec, precision):
    """window 0 (one relative row), 15 (nrel = 31 of the 32 R columns: the mfma kernel's finish<31>), 16 (the scalar kernel)."""
    case = A.text(*spec)
    assert case.choice(precision) == {0: "mfma<8>", 15: "mfma<8>", 16: "scalar"}[case.dims.window_size]
    _run_text(case, precision)
