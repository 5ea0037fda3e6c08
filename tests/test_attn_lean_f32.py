"""The exact-fp32 attention pass beside the decoder LSTM (fused_kernels.hip attn_lstm_kernel, 64 x 16 LSTM tile, B > 96).

The shipped form (step_bodies.h ATTN_LEAN) does the base pass's arithmetic in the base pass's order on fewer vector-ALU
instructions, so it must match the base form (option attn_form = 1) bit for bit; and the schedule bench.py's
headline runs must match the oracle over a full 600-frame Philox decode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
BASE_FORM = 1  # attn_form: the attention pass in its base form


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import hip_helpers

    return hip_helpers


def _decode(eng, mem, NF, opts):
    from torch_tts_amd import _lib

    for k, v in opts.items():
        eng.set_option(k, v)
    B, L = mem.shape[0], mem.shape[1]
    dev = mem.device
    y = torch.empty(B, NF, 80, device=dev)
    s = torch.empty(B, NF, device=dev)
    w = torch.empty(B, NF, L, device=dev)
    t_out = torch.zeros(2, dtype=torch.int32, device=dev)
    eng.decode(mem, t_begin=0, n_steps=NF, stop_threshold=-2.0, check_stop=True, dropout_mode=_lib.DROPOUT_PHILOX, masks=None, seed=123,
               teacher=None, teacher_flags=None, y=y, s=s, w=w, t_out=t_out)
    torch.cuda.synchronize()
    assert t_out.tolist() == [NF, 0]
    return y.cpu(), s.cpu(), w.cpu()


@pytest.mark.parametrize("B, L", [(256, 120), (200, 77)])
def test_lean_attention_pass_is_bit_identical_to_the_base_pass(H, B, L):
    """600 frames, exact fp32; B = 200 leaves a ragged last LSTM row block, L = 77 ragged wave ranges and a short last group."""
    import torch_tts_amd as T

    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    cell = T.Taco2ProdDecoderCell(512, 80, 1, [1024, 1024], dim_pre=256, dim_att=1024)
    dec = T.Decoder(cell, 1, 80)
    for m in dec.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.xavier_normal_(m.weight, gain=1.5)
    dec = dec.to(dev).eval()
    dec.precision = "f32"
    eng = dec.engine(dev)
    g = torch.Generator().manual_seed(1234)
    mem = torch.tanh(torch.randn(B, L, 512, generator=g) * 0.5).to(dev)
    NF = 600
    shipped = _decode(eng, mem, NF, {"attn_form": -1})
    base = _decode(eng, mem, NF, {"attn_form": BASE_FORM})
    assert eng.precision() == "f32"
    for name, a, b in zip("ysw", shipped, base):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: max |diff| {float((a - b).abs().max()):.3e}"


def test_shipped_f32_b256_schedule_vs_oracle_600_frames_philox(H):
    """bench.py's headline leg (B = 256, L = 120, exact fp32, on-device Philox dropout) on the schedule the library ships, against
    the oracle at the parity tests' tolerances, with the attention argmax exact on every step."""
    import test_hip_parity as P

    model, mem, masks, oy, os_, ow, _ = P._headline_case(256, "philox")
    dec = model.decoder
    dec.precision, dec.dropout_source, dec.dropout_seed = "f32", "philox", 123
    eng = dec.engine(torch.device("cuda:0"))
    eng.set_option("attn_form", -1)
    eng.set_option("query_role", -1)
    with torch.no_grad():
        y, s, w = dec(mem, None, None, 599)
    assert eng.precision() == "f32"
    y, s, w = y.cpu(), s.cpu(), w.cpu()
    for n, a, b in (("y", y, oy), ("s", s, os_), ("w", w, ow)):
        H.assert_close(a, b, RTOL, ATOL, n)
    assert torch.equal(w.argmax(-1), ow.argmax(-1))
