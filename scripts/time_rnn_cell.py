"""Fused train step (DeepSpeechTrainer.step) of the GRU model at c3's shape against the same model with the Elman (tanh) cell, nn.RNN.

    python scripts/time_rnn_cell.py [--rounds 3] [--steps 10] [--warmup 3] [--dtype bf16|f32] [--hidden 1024 --layers 5 --batch 64 --tin 1001]

One process, both models resident; the rounds alternate GRU / tanh so that clocks and the other tenants of the device affect both alike.
Every step is timed with a HIP event pair on the compute stream after warm-up; the recurrence calls inside the timed steps (ops.rnn_fwd,
ops.rnn_bwd, ops.rnn_bwd_bn) carry event pairs too, so the per-time-step cost of the forward and backward recurrences is printed beside the
step time.  Prints one line per round and cell, then the medians and spreads (max - min of the round medians) and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tin", type=int, default=1001)
    args = ap.parse_args()
    assert args.rounds >= 1 and args.steps >= 1

    import bench
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW, ops
    from asr_amd.trainers import DeepSpeechTrainer

    dev = torch.device("cuda:0")
    C = 29
    x, targets, pct, tsz = bench.synthetic_batch(args.batch, args.tin, C, 1)
    x = x.to(dev)
    cells = {}
    for cell in ("gru", "rnn"):
        torch.manual_seed(0)
        with tempfile.TemporaryDirectory() as tmp:
            model = DeepSpeech(audio_conf=bench.audio_conf(), decoder=None, label_path=bench.label_file(tmp, C), rnn_type=cell,
                               rnn_hidden_size=args.hidden, rnn_hidden_layers=args.layers, bidirectional=True)
        model.to(dev).train()
        model.precision = "bf16" if args.dtype == "bf16" else "fp32"
        opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
        cells[cell] = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)

    calls = []                                          # (kind, T, start event, end event, last_path) of every recurrence call
    orig = (ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn)

    def timed(fn, kind, t_arg):
        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            calls.append((kind, int(a[t_arg]), e0, e1, ops.rnn_last_path()))
            return r
        return wrapped

    results = {c: {"step_ms": [], "fwd_us_per_t": [], "bwd_us_per_t": [], "last_path": set(), "loss": None} for c in cells}
    for rnd in range(args.rounds):
        for cell, tr in cells.items():
            for _ in range(args.warmup):
                tr.step((x, targets, pct.clone(), tsz))
            tr.synchronize()
            ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn = timed(orig[0], "fwd", 5), timed(orig[1], "bwd", 7), timed(orig[2], "bwd", 12)
            del calls[:]
            ev = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                valid, lv = tr.step((x, targets, pct.clone(), tsz))
                e1.record()
                ev.append((e0, e1))
            ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn = orig
            torch.cuda.synchronize()
            tr.synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            per_t = {k: [a.elapsed_time(b) * 1e3 / t for kind, t, a, b, _ in calls if kind == k] for k in ("fwd", "bwd")}
            r = results[cell]
            r["step_ms"].append(statistics.median(ms))
            r["fwd_us_per_t"].append(statistics.median(per_t["fwd"]))
            r["bwd_us_per_t"].append(statistics.median(per_t["bwd"]))
            r["last_path"] |= {p for *_, p in calls}
            r["loss"] = float(lv)
            print(f"round {rnd} {cell:3s}: step median {r['step_ms'][-1]:.2f} ms (min {min(ms):.2f} max {max(ms):.2f}); recurrence per time step "
                  f"fwd {r['fwd_us_per_t'][-1]:.2f} us, bwd {r['bwd_us_per_t'][-1]:.2f} us; last_path bits {sorted(r['last_path'])}", flush=True)
    out = {"shape": dict(hidden=args.hidden, layers=args.layers, batch=args.batch, tin=args.tin, dtype=args.dtype), "rounds": args.rounds,
           "steps": args.steps}
    for cell, r in results.items():
        med = statistics.median(r["step_ms"])
        spread = max(r["step_ms"]) - min(r["step_ms"])
        print(f"{cell:3s}: step {med:.2f} ms (spread {spread:.2f} over {args.rounds} rounds); recurrence per time step fwd "
              f"{statistics.median(r['fwd_us_per_t']):.2f} us, bwd {statistics.median(r['bwd_us_per_t']):.2f} us")
        out[cell] = {"step_ms_median": round(med, 3), "step_ms_spread": round(spread, 3), "step_ms_rounds": [round(v, 3) for v in r["step_ms"]],
                     "fwd_us_per_t": round(statistics.median(r["fwd_us_per_t"]), 3), "bwd_us_per_t": round(statistics.median(r["bwd_us_per_t"]), 3),
                     "last_path_bits": sorted(r["last_path"]), "last_loss": r["loss"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
