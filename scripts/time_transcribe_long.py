"""Time the long-form transcription of posteriors you already have (decoders.transcribe_posteriors, the device half of
DeepSpeech.transcribe_long), split into its three parts, next to the same decoder on probs[None] as ONE utterance.

Synthetic posteriors, C = 29: planted text with pauses (phrases of 8 .. 200 characters, a few of 400 that exceed max_len; every character
2 .. 5 frames at 0.6 and one soft-blank frame; pauses of 25 .. 120 silent frames), T = 30 000 (ten minutes at 20 ms per frame) and
T = 180 000 (an hour).  Options: the defaults (threshold 0.9, min_gap 25, pad 5, max_len 1000, decode_batch 64).
  segment  ops.ctc_segment, two launches                                   device events around back-to-back calls
  gather   ops.ctc_segment_gather for every batch of the plan              device events
  decode   decoder.decode for every gathered batch (with its device-to-host copy and the strings)   wall clock, synchronised
  e2e      transcribe_posteriors                                            wall clock
  whole    decoder.decode(probs[None])                                      wall clock
for GreedyDecoder and BeamCTCDecoder(beam_width=16) without a language model.  The one-utterance beam decode runs only up to
--whole-beam-max-t frames (default 30 000: at T = 180 000 it did not finish within seven minutes; its tie rule walks prefix chains that
grow with the recording, csrc/ctc_beam.h).  Prints a table and one JSON line, and writes both to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABELS = "_'abcdefghijklmnopqrstuvwxyz "


def posteriors(T, C, seed):
    """(T, C) float32 probabilities on the host: -1 = silent frame (blank 0.9 .. 0.995), 0 = soft blank (0.5), c = class c at 0.6"""
    rng = np.random.default_rng(seed)
    kinds = [np.full(40, -1)]
    n = 40
    while n < T:
        chars = int(rng.choice([8, 20, 50, 100, 200, 400], p=[0.2, 0.25, 0.25, 0.15, 0.1, 0.05]))
        lab = rng.integers(2, C - 1, chars)
        lab[rng.random(chars) < 0.18] = C - 1                                              # spaces
        dur = rng.integers(2, 6, chars)
        ph = np.concatenate([np.r_[np.full(d, c), 0] for c, d in zip(lab, dur)])
        pause = np.full(int(rng.integers(25, 121)), -1)
        kinds += [ph, pause]
        n += len(ph) + len(pause)
    kinds = np.concatenate(kinds)[:T]
    u = rng.random(T)
    pb = np.where(kinds < 0, 0.9 + 0.095 * u, np.where(kinds == 0, 0.5, 0.05 + 0.25 * u))
    pl = np.where(kinds > 0, 0.6, 0.0)
    x = np.repeat(((1.0 - pb - pl) / (C - 1 - (kinds > 0)))[:, None], C, 1)
    x[:, 0] = pb
    x[kinds > 0, kinds[kinds > 0]] = 0.6
    return x.astype(np.float32)


def wall(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--whole-beam-max-t", type=int, default=30000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[30000, 180000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transcribe_long_timing.txt"))
    args = ap.parse_args()
    from asr_amd import _lib, ops
    from asr_amd.decoders import BeamCTCDecoder, GreedyDecoder, plan_segment_batches, transcribe_posteriors
    assert torch.cuda.is_available(), "time_transcribe_long.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    lines, res = [], dict(rounds=args.rounds, iters=args.iters)

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Long-form transcription of posteriors (scripts/time_transcribe_long.py; {torch.cuda.get_device_name(0)}, one process; library {_lib.version()})")
    say("C = 29, planted text with pauses; threshold 0.9, min_gap 25, pad 5, max_len 1000, decode_batch 64; ms, mean over the rounds [each round]")
    for T in args.sizes:
        probs = torch.from_numpy(posteriors(T, 29, T)).to(dev)
        start, end, flags, n_segs = ops.ctc_segment(probs[None])
        n = int(n_segs[0])
        start_h, end_h = start[0, :n].cpu().numpy(), end[0, :n].cpu().numpy()
        lens = end_h - start_h
        batches = plan_segment_batches(lens, 64)
        padded = sum(int(lens[b[0]]) * len(b) for b in batches)
        forced = int((flags[0, :n] != 0).sum())
        say()
        say(f"T = {T}: {n} segments ({forced} at a forced cut), {int(lens.min())} .. {int(lens.max())} frames, {int(lens.sum())} of {T} frames kept; "
            f"{len(batches)} batches, {padded} padded frames: padding share {1 - lens.sum() / padded:.3f}")
        res[f"T{T}_segments"], res[f"T{T}_batches"], res[f"T{T}_padding_share"] = n, len(batches), round(float(1 - lens.sum() / padded), 4)
        idx = [torch.tensor(np.stack((np.zeros(len(b), np.int32), start_h[b], lens[b])), dtype=torch.int32, device=dev) for b in batches]
        t_max = [int(lens[b[0]]) for b in batches]
        gather = lambda: [ops.ctc_segment_gather(probs[None], d[0], d[1], d[2], tm) for d, tm in zip(idx, t_max)]
        packed = gather()
        rows = {}
        for name, dec in (("greedy", GreedyDecoder(LABELS)), ("beam16", BeamCTCDecoder(LABELS, beam_width=16))):
            run_whole = name != "beam16" or T <= args.whole_beam_max_t
            if not run_whole:
                say(f"{name}: the one-utterance decode at T = {T} is not timed (--whole-beam-max-t {args.whole_beam_max_t})")
            legs = {"segment": lambda: events(lambda: ops.ctc_segment(probs[None]), args.iters),
                    "gather": lambda: events(gather, args.iters),
                    "decode": lambda dec=dec: wall(lambda: [dec.decode(p, s) for p, s in packed], 1)[0],
                    "e2e": lambda dec=dec: wall(lambda: transcribe_posteriors(probs, dec), 1)[0]}
            if run_whole:
                legs["whole"] = lambda dec=dec: wall(lambda: dec.decode(probs[None]), 1)[0]
            for k, fn in legs.items():                                                     # warm up every leg once
                print(f"  warm-up {name} {k}: {fn():.3f} ms", flush=True)
            times = {k: [] for k in legs}
            for r in range(args.rounds):
                for k, fn in legs.items():                                                 # the legs alternate within a round
                    times[k].append(fn())
                print(f"  round {r} of {name} done", flush=True)
            for k, v in times.items():
                rows[f"{name}_{k}"] = v
                res[f"T{T}_{name}_{k}_ms"], res[f"T{T}_{name}_{k}_ms_rounds"] = round(float(np.mean(v)), 3), [round(a, 3) for a in v]
        say(f"{'leg':<18}{'ms':>12}   rounds")
        for k, v in rows.items():
            say(f"{k:<18}{np.mean(v):>12.3f}   {[round(a, 3) for a in v]}  spread {max(v) - min(v):.3f}")
        for name in ("greedy", "beam16"):
            if f"{name}_whole" in rows:
                r = np.mean(rows[f"{name}_e2e"]) / np.mean(rows[f"{name}_whole"])
                res[f"T{T}_{name}_e2e_over_whole"] = round(float(r), 4)
                say(f"{name}: segmented end to end / one utterance = {r:.4f}")
            share = (np.mean(rows[f"{name}_segment"]) + np.mean(rows[f"{name}_gather"])) / np.mean(rows[f"{name}_e2e"])
            res[f"T{T}_{name}_segment_gather_share"] = round(float(share), 4)
            say(f"{name}: segment + gather = {share:.4f} of the end-to-end time")
    say()
    say("raw result line:")
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
