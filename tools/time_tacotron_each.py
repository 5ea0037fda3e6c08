#!/usr/bin/env python3
"""Times batched synthesis (per-utterance stop rule, Postnet with lengths) on the LJSpeech model, random init:

  rule     per-step time of ttsdec_decode_each against ttsdec_decode, never firing, B x 600 steps, both arithmetic modes
  postnet  ttsdec_postnet_ragged with lengths uniform in [300, 600] against ttsdec_postnet at 256 x 600, three precisions
  synth    64 utterances whose rows stop between steps 300 and 600: encoder + forward_each + Postnet with lengths against the
           same batch run to max_steps = 1000 (the only way the batch-global rule gets every utterance whole)

Usage: python tools/time_tacotron_each.py [--step rule|postnet|synth] [--iters 5] [--limit 240]
Without --step every step runs in a child process of its own under a time limit of --limit seconds; the first that fails or
runs out of time ends the run.

How `synth` places the stop steps: two channels of the memory are cut out of the model (the weights that read them in the
attention query, both LSTMs and fc_mel are zeroed), so they reach only fc_stop.  One carries the position index l - the context's
value there is the attention's mean position, which only moves forward; the other a per-utterance constant o_b.  fc_stop reads
o_b - position, the threshold is 0: utterance b stops when its attention passes o_b.  A first pass without the rule records each
utterance's mean position per step; o_b is put between its values at steps t_b - 1 and t_b, t_b spread over [300, 600)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LJSPEECH = {
    "text": {"alphabet": "x" * 39},
    "audio": {"num_mels": 80},
    "model": {
        "encoder": {"type": "tacotron2", "dim_emb": 512, "dim_out": 512},
        "decoder": {"type": "tacotron2prod", "r": 1, "dim_pre": 256, "dim_att": 1024, "dim_rnn": [1024, 1024]},
        "postnet": {"type": "tacotron2", "dim_hidden": 512, "num_layers": 3},
    },
}
STEPS = ("rule", "postnet", "synth")


def timed(fn, iters):
    """Median wall time (ms) of fn() over `iters` runs, each fenced by a device synchronisation; one warm-up run."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def model_and_memory(B, L, seed=42):
    import torch

    import torch_tts_amd as T

    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    model = T.build_tacotron(LJSPEECH).eval().to(dev)
    model.decoder.dropout_source, model.decoder.dropout_seed = "philox", 123
    ids = torch.randint(1, 40, (B, L), generator=torch.Generator().manual_seed(1234)).to(dev)
    lens = torch.full((B,), L, dtype=torch.long, device=dev)
    return model, ids, lens, dev


def step_rule(args):
    import torch

    from torch_tts_amd import _lib

    NS = 600
    for B in (256, 64):
        model, ids, lens, dev = model_and_memory(B, 120)
        dec = model.decoder
        with torch.no_grad():
            mem = torch.cat([model.encoder(ids[i : i + 64], lens[i : i + 64]) for i in range(0, B, 64)]).contiguous()
        y, s, w = torch.empty(B, NS, 80, device=dev), torch.empty(B, NS, device=dev), torch.empty(B, NS, 120, device=dev)
        t_out = torch.zeros(2, dtype=torch.int32, device=dev)
        stop_steps = torch.empty(B, dtype=torch.int32, device=dev)
        for prec in ("f32", "split_f16"):
            dec.precision = prec
            eng = dec.engine(dev)
            common = dict(t_begin=0, n_steps=NS, stop_threshold=-1e30, dropout_mode=_lib.DROPOUT_PHILOX, masks=None, seed=123, y=y, s=s, w=w,
                          t_out=t_out)
            any_ = lambda: eng.decode(mem, check_stop=True, teacher=None, teacher_flags=None, **common)
            each = lambda: eng.decode_each(mem, stop_steps=stop_steps, **common)
            # interleaved, so that a drift of the device's clocks lands on both
            ta, te = [], []
            for _ in range(3):
                ta.append(timed(any_, args.iters)[0])
                te.append(timed(each, args.iters)[0])
            assert t_out.tolist() == [NS, 0] and int(stop_steps.min()) == 0x7FFFFFFF
            a, e = statistics.median(ta), statistics.median(te)
            print(f"rule     B={B:3d} {prec:9s} decode {a / NS * 1e3:7.2f} us/step  decode_each {e / NS * 1e3:7.2f} us/step  ratio {e / a:.4f}  "
                  f"(medians of 3 x {args.iters}; decode per round {[round(v / NS * 1e3, 2) for v in ta]}, each {[round(v / NS * 1e3, 2) for v in te]})",
                  flush=True)


def step_postnet(args):
    import torch

    import torch_tts_amd as T

    dev = torch.device("cuda:0")
    B, NF = 256, 600
    torch.manual_seed(0)
    pn = T.MelPostnet(80, 512, 5, 3).to(dev).eval()
    y = torch.randn(B, NF, 80, device=dev)
    lengths = torch.randint(300, NF + 1, (B,), generator=torch.Generator().manual_seed(5)).to(dev)
    real = int(lengths.sum()) / (B * NF)
    for mode in ("f32", "split_f16", "bf16"):
        pn.precision = mode
        with torch.no_grad():
            tp, tr = [], []
            for _ in range(3):
                tp.append(timed(lambda: pn(y), args.iters)[0])
                tr.append(timed(lambda: pn(y, lengths=lengths), args.iters)[0])
        p, r = statistics.median(tp), statistics.median(tr)
        print(f"postnet  {B} x {NF} {mode:9s} plain {p:7.3f} ms  ragged {r:7.3f} ms  ratio {r / p:.4f}  ({real:.3f} of the frames are real; "
              f"plain per round {[round(v, 3) for v in tp]}, ragged {[round(v, 3) for v in tr]})", flush=True)


def step_synth(args):
    import torch

    B, L, LO, HI, CAP = 64, 600, 300, 600, 1000
    model, ids, lens, dev = model_and_memory(B, L)
    dec, cell = model.decoder, model.decoder.decoder_cell
    D, Ha, Hd, P = cell.dim_ctx, cell.attention_rnn.hidden_size, cell.decoder_rnn.hidden_size, cell.dim_pre
    c_off, c_pos = D - 2, D - 1
    with torch.no_grad():  # the two channels reach nothing but fc_stop
        for c in (c_off, c_pos):
            cell.attention_module.query_layer.weight[c, :] = 0
            cell.attention_rnn.weight_ih[:, P + c] = 0
            cell.decoder_rnn.weight_ih[:, Ha + c] = 0
            dec.fc_mel.weight[:, Hd + c] = 0
        dec.fc_stop.weight.zero_()
        dec.fc_stop.bias.zero_()
        dec.fc_stop.weight[0, Hd + c_off] = 1.0
        dec.fc_stop.weight[0, Hd + c_pos] = -1.0
    dec.invalidate()
    pos = torch.arange(L, dtype=torch.float32, device=dev)

    def memory(offsets):
        with torch.no_grad():
            mem = model.encoder(ids, lens).clone()
        mem[:, :, c_pos] = pos[None, :]
        mem[:, :, c_off] = offsets[:, None]
        return mem

    for prec in ("f32", "split_f16"):
        dec.precision = prec
        if model.postnet is not None:
            model.postnet.precision = prec
        # pass 1: no rule, s[b, t] = -(mean attention position of b at step t)
        dec.stop_threshold = -1e30
        with torch.no_grad():
            s = dec(memory(torch.zeros(B, device=dev)), None, None, HI - 1)[1][:, :, 0]
        p = -s  # [B, HI]
        want = torch.linspace(LO, HI - 1, B).round().long().to(dev)
        rows = torch.arange(B, device=dev)
        off = (p[rows, want - 1] + p[rows, want]) / 2
        t_b = (p > off[:, None]).int().argmax(dim=1)  # the first step past the offset
        moved = float((p[:, -1] - p[:, 0]).mean())
        print(f"synth    {prec}: attention moved {moved:.1f} positions in {HI} steps; stop steps placed at {int(t_b.min())} .. {int(t_b.max())}, "
              f"mean {float(t_b.float().mean()):.0f}", flush=True)
        if int(t_b.min()) < LO // 2:
            print("synth    the attention of this model does not move enough to place the stop steps; nothing timed", flush=True)
            return
        dec.stop_threshold = 0.0
        dec.max_decoder_steps = CAP  # (an unbounded decode that missed a stop would never end)
        out = {}

        def each():
            with torch.no_grad():
                y, s_, w, lengths, stopped = dec.forward_each(memory(off), None)
                out["v"] = (model.postnet(y, lengths=lengths), lengths, stopped)

        def capped():
            dec.stop_threshold = -1e30  # (the batch-global rule would cut every utterance at the first one's end)
            with torch.no_grad():
                y, s_, w = dec(memory(off), None, None, CAP - 1)
                out["c"] = model.postnet(y)
            dec.stop_threshold = 0.0

        te, tc = [], []
        for _ in range(2):
            te.append(timed(each, args.iters)[0])
            tc.append(timed(capped, args.iters)[0])
        _, lengths, stopped = out["v"]
        assert bool(stopped.all()), "an utterance missed its stop"
        off_by = int((lengths != t_b + 1).sum())
        if off_by:  # (an offset closer to a position than the projection's rounding: the timing stands, the placement is approximate)
            print(f"synth    {prec}: {off_by} utterances stopped a step away from where pass 1 placed them", flush=True)
        e, c = statistics.median(te), statistics.median(tc)
        real = int(lengths.sum())
        print(f"synth    {prec}: B={B}, lengths {int(lengths.min())} .. {int(lengths.max())} (sum {real}): each + ragged Postnet {e:8.2f} ms = "
              f"{real / e * 1e3:9.0f} real frames/s;  run to {CAP} steps {c:8.2f} ms = {real / c * 1e3:9.0f} real frames/s;  ratio {c / e:.3f}  "
              f"(per round: each {[round(v, 2) for v in te]}, capped {[round(v, 2) for v in tc]})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each step's process may take")
    args = ap.parse_args()
    if args.step:
        {"rule": step_rule, "postnet": step_postnet, "synth": step_synth}[args.step](args)
        return 0
    for step in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(args.iters)], timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {args.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{step}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
