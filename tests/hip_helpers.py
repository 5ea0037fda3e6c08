"""Shared helpers for the GPU parity tests: build the product modules (the drop-in
mirrors of the reference's classes) from an oracle-style weight dict; pick the utterances a CPU oracle checks at bench-sized
shapes; restate conv256's launch schedule; emulate the bf16 Postnet's arithmetic on the CPU."""
import torch

import torch_tts_amd as T
from oracle import tacotron_oracle as O


def make_decoder(dims: O.DecoderDims, wts, device="cuda:0", stop_threshold=-2.0):
    cell = T.Taco2ProdDecoderCell(dims.d_ctx, dims.d_mel, dims.r, [dims.h_att, dims.h_dec], dim_pre=dims.d_pre, dim_att=dims.h_att,
                                  p_zoneout=dims.p_zoneout)
    dec = T.Decoder(cell, dims.r, dims.d_mel, stop_threshold=stop_threshold)
    missing, unexpected = dec.load_state_dict(wts, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("attention_module.bias") for k in missing), missing
    return dec.to(device).eval()


def make_taco2_decoder(dims: O.DecoderDims, wts, device="cuda:0", stop_threshold=-2.0):
    cell = T.Taco2DecoderCell(dims.d_ctx, dims.d_mel, dims.r, [dims.h_att, dims.h_dec], dim_pre=dims.d_pre, p_zoneout=dims.p_zoneout)
    dec = T.Decoder(cell, dims.r, dims.d_mel, stop_threshold=stop_threshold)
    missing, unexpected = dec.load_state_dict(wts, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("attention_module.bias") for k in missing), missing
    return dec.to(device).eval()


def flat_masks(m0, m1):
    """Per step: layer-0 mask [B, 128] then layer-1 mask [B, d_pre], flattened (include/ttsdec.h)."""
    T_ = m0.shape[0]
    return torch.cat([m0.reshape(T_, -1), m1.reshape(T_, -1)], dim=1).contiguous()


def make_postnet(d_mel, hidden, layers, wts, device="cuda:0", k=5):
    pn = T.MelPostnet(d_mel, dim_hidden=hidden, kernel_size=k, num_layers=layers)
    missing, unexpected = pn.load_state_dict(wts, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing), missing
    return pn.to(device).eval()


def run_decoder_with_masks(dec, memory, masks, *, max_steps=0, x=None, flags=None, device="cuda:0"):
    """Drives ttsdec_decode directly with injected masks (and teacher flags), the way
    Decoder.forward does for one bounded call."""
    from torch_tts_amd import _lib

    memory = memory.to(device)
    B, L, _ = memory.shape
    r, dm = dec.r, dec.dim_mel
    eng = dec.engine(memory.device)
    if x is not None:
        n = x.shape[1] // r
        teacher = x[:, : n * r].to(device).contiguous()
        fl = torch.ones(n, dtype=torch.uint8) if flags is None else torch.cat([torch.as_tensor(flags, dtype=torch.uint8), torch.ones(1, dtype=torch.uint8)])
        fl = fl.to(device)
        check = False
    else:
        n = max_steps + 1
        teacher, fl, check = None, None, True
    y = torch.empty(B, n * r, dm, device=device)
    s = torch.empty(B, n * r, device=device)
    w = torch.empty(B, n, L, device=device)
    t_out = torch.zeros(2, dtype=torch.int32, device=device)
    mode = _lib.DROPOUT_MASKS if masks is not None else _lib.DROPOUT_OFF
    eng.decode(memory, t_begin=0, n_steps=n, stop_threshold=float(dec.stop_threshold), check_stop=check, dropout_mode=mode,
               masks=None if masks is None else masks[:n].to(device).contiguous(), seed=0, teacher=teacher, teacher_flags=fl,
               y=y, s=s, w=w, t_out=t_out)
    done, fired = t_out.tolist()
    return y[:, : done * r].cpu(), s[:, : done * r].unsqueeze(2).cpu(), w[:, :done].cpu(), bool(fired)


def make_postnet2(d_mel, hidden, layers, wts, device="cuda:0"):
    pn = T.MelPostnet2(d_mel, dim_hidden=hidden, num_layers=layers)
    missing, unexpected = pn.load_state_dict(wts, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith("num_batches_tracked") for k in missing), missing
    return pn.to(device).eval()


def assert_close(a, b, rtol=1e-4, atol=1e-5, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: max abs err {float(err.max()):.3e}, {int(bad.sum())} of {bad.numel()} outside rtol={rtol} atol={atol}"


def assert_argmax(w, ow, what="attention argmax", tie=2e-6):
    """argmax(w) must equal argmax(ow) bit for bit - except on rows where the reference's own two largest weights
    differ by less than `tie` (absolute; the weights of a row sum to 1): there any fp32 evaluation order decides the
    index, the reference's included.  Prints what it tolerated."""
    a, b = w.argmax(-1), ow.argmax(-1)
    bad = a != b
    if not bool(bad.any()):
        return
    top2 = ow[bad].topk(2, dim=-1).values
    gap = (top2[:, 0] - top2[:, 1]).abs()
    err = (w[bad] - ow[bad]).abs().max(dim=-1).values
    print(f"{what}: {int(bad.sum())} of {bad.numel()} rows differ; reference top-2 gaps {gap.tolist()[:8]}, max |w - ow| there {err.tolist()[:8]}")
    assert bool((gap < tie).all()), f"{what}: argmax differs on a row whose top-2 gap is {float(gap.max()):.3e}"


# --------------------------------------------------------------------------
# bench-shape parity on a sample: utterances never interact (the decode step is row-wise; Encoder2, the Postnet convs and
# the VITS2 convs, attention and LayerNorm are per utterance), so the GPU runs the whole batch and the oracle a few rows of it
# --------------------------------------------------------------------------
def sample_utterances(B, T, boundaries=(), k_random=2, seed=0):
    """Sorted, deduplicated utterance indices of a [B, T]-row batch: the first, the last, the one holding each row index in
    `boundaries` (rows of the flattened [B * T] matrix where a kernel changes tile or launch) and `k_random` seeded others."""
    assert B >= 1 and T >= 1
    picked = {0, B - 1}
    for r in boundaries:
        assert 0 <= r < B * T, (r, B, T)
        picked.add(int(r) // T)
    rest = [b for b in torch.randperm(B, generator=torch.Generator().manual_seed(seed)).tolist() if b not in picked]
    picked.update(rest[:k_random])
    return sorted(picked)


def last_tile_rows(M, *tiles):
    """The first row of the last tile of each height in `tiles` over M rows (where a ragged last tile's row mask starts)."""
    return [((M - 1) // t) * t for t in tiles]


def conv256_schedule(M, cus, *, Cin=512, N=512, taps=5, elem_bytes=2, force=False):
    """The row schedule launch_conv256_abl (torch-tts_amd/csrc/conv256.hip) gives a [M, Cin] -> [M, N] layer on a device of
    `cus` CUs: None where the library keeps the shared GEMM tile, else {"full", "h", "nmt", "n_short"}: `full` whole 256-row
    tiles (conv256_kernel<., ., 4>), then `n_short` short tiles of `h` rows from row full * 256 (conv256_kernel<., ., nmt>).
    A restatement - the source it mirrors:

        if (M <= 0 || T <= 0 || ((Cin * EB) % kRowB) || (N % kT256) || !(taps & 1) || taps > 15) return false;
        if ((size_t)M * Cin * EB >= kOob || (size_t)N * taps * Cin * EB >= kOob) return false;  // 32-bit buffer offsets
        ...
        if (cus <= 0) return false;
        const int n_rt = (M + kT256 - 1) / kT256, slots = cus / g.n_col_tiles > 0 ? cus / g.n_col_tiles : 1;
        const int full = (n_rt / slots) * slots;        // row tiles of the whole rounds
        const int rem = M - full * kT256;               // rows left for the last round (<= 0: none)
        int h = 0, nmt = 0, n_short = 0;
        if (rem > 0) {
          h = (rem + slots - 1) / slots;
          h = (h + 7) & ~7;                             // (whole 8-row DMA groups)
          nmt = (h + 63) >> 6;
          n_short = (rem + h - 1) / h;
        }
        {
          const double ideal = (double)M / kT256 / slots, cost = (double)(full / slots) + (rem > 0 ? nmt / 4.0 : 0.0);
          const char* force = getenv("TTSDEC_CONV256_FORCE");
          if (ABL == 0 && !(force && force[0] == '1') && ideal < 0.86 * cost) return false;
        }
        if (full > 0) launch_conv256_tiles<ABL, kF32, 4>(g, 0, kT256, full, st);
        if (rem > 0) { ... nmt >= 4 ? 4 : nmt ... }
    """
    kT256, kRowB, kOob = 256, 128, 0x7FFFF000
    if M <= 0 or (Cin * elem_bytes) % kRowB or N % kT256 or not taps & 1 or taps > 15:
        return None
    if M * Cin * elem_bytes >= kOob or N * taps * Cin * elem_bytes >= kOob or cus <= 0:
        return None
    n_col = N // kT256
    n_rt = (M + kT256 - 1) // kT256
    slots = cus // n_col if cus // n_col > 0 else 1
    full = (n_rt // slots) * slots
    rem = M - full * kT256
    h = nmt = n_short = 0
    if rem > 0:
        h = (rem + slots - 1) // slots
        h = (h + 7) & ~7
        nmt = (h + 63) >> 6
        n_short = (rem + h - 1) // h
    ideal, cost = M / kT256 / slots, (full // slots) + (nmt / 4.0 if rem > 0 else 0.0)
    if not force and ideal < 0.86 * cost:
        return None
    return {"full": full, "h": h, "nmt": min(nmt, 4), "n_short": n_short}


def device_cus(device=0):
    return torch.cuda.get_device_properties(device).multi_processor_count


def postnet_bf16_emulation(y, pw, num_layers=3, acc=torch.float32, leak=False):
    """The bf16 Postnet's own arithmetic on the CPU: operands rounded to bf16 between the layers, fp32 accumulation, fp32 BN +
    isru, the residual in fp32.  y [B, T, d_mel] fp32; pw: oracle-style MelPostnet weights; the padding is the weight's
    (taps - 1) / 2, as in O.mel_postnet.
    acc=torch.float64: the same roundings with the sums (and BN + isru) in fp64 - a yardstick for how far summation order alone moves
    the result.  leak=True (taps > 1): a deliberately WRONG emulation, in which the last frame of every utterance also receives the
    first tap past its window (taps / 2 + 1) applied to frame 0 of the next utterance - the row that follows it in the flattened
    [B * T, C] activation, i.e. what a conv whose window is not clipped at an utterance's edge would compute.  The tests show that
    the bf16 bar tells it from the right one."""
    from oracle import tacotron_oracle as O

    def rb(x):
        return x.to(torch.bfloat16).to(torch.float32)

    xc = rb(y).transpose(1, 2).to(acc)
    for i in range(num_layers):
        w = rb(pw[f"conv.{i}.0.weight"]).to(acc)
        src = xc
        xc = torch.nn.functional.conv1d(src, w, None, padding=(w.shape[2] - 1) // 2)
        if leak:
            xc[:, :, -1] += torch.roll(src[:, :, 0], -1, 0) @ w[:, :, w.shape[2] // 2 + 1].T
        inv = 1.0 / torch.sqrt(pw[f"conv.{i}.1.running_var"].to(acc) + 1e-5)
        alpha = pw[f"conv.{i}.1.weight"].to(acc) * inv
        beta = pw[f"conv.{i}.1.bias"].to(acc) - pw[f"conv.{i}.1.running_mean"].to(acc) * alpha
        xc = rb(O.isru(xc * alpha[None, :, None] + beta[None, :, None])).to(acc)
    return (y.to(acc) + torch.nn.functional.linear(xc.transpose(1, 2), rb(pw["fc_out.weight"]).to(acc))).to(torch.float32)


WS_GUARD = 4096  # bytes on each side of a guarded workspace


def assert_workspace_fits(monkeypatch, cls, method, nbytes_of, run):
    """run() (-> a tensor) twice with `cls.method`, the engine's workspace getter, replaced: once on exactly the reported bytes -
    nbytes_of(engine, *the getter's arguments) - cut from the middle of a tensor whose WS_GUARD bytes on either side hold a fixed
    pattern, once on a generously oversized one.  The guards must come back untouched (an overrun is a changed byte of the test's
    own memory, not a fault) and the two results must be bit-equal."""
    bufs = []

    def guarded(self, *a):
        n = int(nbytes_of(self, *a))
        buf = torch.full((2 * WS_GUARD + n,), 0xA5, dtype=torch.uint8, device=self.device)
        assert n > 0 and buf.data_ptr() % 256 == 0
        bufs.append(buf)
        return buf[WS_GUARD:WS_GUARD + n]

    def roomy(self, *a):
        return torch.empty(4 * int(nbytes_of(self, *a)) + (1 << 20), dtype=torch.uint8, device=self.device)

    with monkeypatch.context() as mp:
        mp.setattr(cls, method, guarded)
        got = run()
        mp.setattr(cls, method, roomy)
        want = run()
    torch.cuda.synchronize()
    assert bufs, "the call took no workspace"
    for buf in bufs:
        assert bool((buf[:WS_GUARD] == 0xA5).all()) and bool((buf[-WS_GUARD:] == 0xA5).all()), "a guard of the workspace was written"
    assert torch.equal(got, want)
