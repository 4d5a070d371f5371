"""Time the keyword search (ops.ctc_keyword_search: the best-class row, the free-start lattice, the pick) next to its yardstick, the
one-wavefront aligner (ops.ctc_forced_align, variant 1) on as many lattices of the same T and U: the same cell, with back-pointer
stores, a backtrace and token spans where the search stores one score and one start per frame and picks.

(a) B = 64, T = 501, C = 29, probabilities in (T,B,C) storage (a softmax of random logits, not a model's output), K = 1, 16, 128
    keywords of 8 labels.   (b) B = 1, T = 180000 (an hour of audio at 20 ms per frame), K = 16.
The aligner has no notion of shared keywords: its B * K utterances are B * K copies of the posteriors (K rows per utterance), so it
reads K times the bytes the search reads; at these sizes both are bound by the per-frame dependent chain, not by bytes.
Thresholds are U * log(0.5), the KeywordSpotter default.  Device events around `iters` back-to-back calls, the legs alternated within
every round.  Prints a table (us per call, ns per lattice and frame) and one JSON line, and writes both to --out."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(dev, B, T, C, K, U, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = (torch.randn((T, B, C), generator=g) * 2.0).to(dev)
    x = torch.softmax(z, -1).transpose(0, 1)                                               # (B,T,C) view of (T,B,C) storage
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, C, (K, U)).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = B * K
    return dict(x=x, U=U, K=K, labels=t(lab.reshape(-1)), off=t(np.arange(K, dtype=np.int32) * U), lens=t(np.full(K, U, np.int32)),
                thr=t(np.full(K, U * math.log(0.5), np.float32)), in_lens=t(np.full(B, T, np.int32)),
                # the aligner's batch: utterance b * K + k is utterance b against keyword k
                ax=x.repeat_interleave(K, dim=0).contiguous(), atargets=t(np.tile(lab.reshape(-1), B)), aoff=t(np.arange(n, dtype=np.int32) * U),
                alens=t(np.full(n, U, np.int32)), ain_lens=t(np.full(n, T, np.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--long-iters", type=int, default=5)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kws_timing.txt"))
    args = ap.parse_args()
    from asr_amd import _lib, ops
    assert torch.cuda.is_available(), "time_kws.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    shapes = [("a", 64, 501, K) for K in (1, 16, 128)] + ([] if args.skip_long else [("b", 1, 180000, 16)])
    calls, iters, lattices = {}, {}, {}
    for tag, B, T, K in shapes:
        p = problem(dev, B, T, 29, K, 8, K)
        name = f"{tag}_B{B}_T{T}_K{K}"
        calls[name + "_kws"] = lambda p=p: ops.ctc_keyword_search(p["x"], p["labels"], p["off"], p["lens"], p["U"], p["thr"], p["in_lens"], False, 32)
        calls[name + "_align"] = lambda p=p: ops.ctc_forced_align(p["ax"], p["atargets"], p["aoff"], p["ain_lens"], p["alens"], p["U"], False, 1)
        for leg in ("_kws", "_align"):
            lattices[name + leg] = (B * K, T)
            if tag == "b":
                iters[name + leg] = args.long_iters
    lines = []

    def say(s=""):
        print(s)
        lines.append(s)

    say(f"Keyword search against the one-wavefront aligner (scripts/time_kws.py; {torch.cuda.get_device_name(0)}, one process; library {_lib.version()})")
    say("C = 29, probabilities, keywords of 8 labels, thresholds 8 log 0.5, max_hits 32; kws = ops.ctc_keyword_search (three launches: best-class row,")
    say("lattice, pick); align = ops.ctc_forced_align variant 1 on B * K utterances (copies of the posteriors), one launch")
    for k, fn in calls.items():                                                            # warm up every shape of the timed window
        for _ in range(3):
            out = fn()
        torch.cuda.synchronize()
        if k.endswith("_kws"):
            nh = out[5]
            say(f"{k}: {int((nh > 0).sum())} of {nh.numel()} (utterance, keyword) pairs have a hit, {int(nh.clamp(max=32).sum())} hits, "
                f"{int(torch.isfinite(out[0]).sum())} of {out[0].numel()} frame scores finite")
        else:
            assert bool(torch.isfinite(out[0]).all()), f"{k}: an utterance of the timing batch is infeasible"
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                        # the legs alternate within a round
            n = iters.get(k, args.iters)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / n)                                 # us per call
    res = dict(rounds=args.rounds, iters=args.iters, long_iters=args.long_iters)
    say(f"us per call (device events, {args.iters} calls back to back; the b legs {args.long_iters}), mean over {args.rounds} rounds, spread = max - min")
    say(f"{'leg':<26}{'us/call':>12}{'us/lattice':>12}{'ns/(lattice frame)':>20}   rounds")
    for k, v in times.items():
        m, (n_lat, T) = float(np.mean(v)), lattices[k]
        res[k + "_us"], res[k + "_us_rounds"], res[k + "_spread_us"] = round(m, 2), [round(a, 2) for a in v], round(max(v) - min(v), 2)
        res[k + "_us_per_lattice"] = round(m / n_lat, 4)
        say(f"{k:<26}{m:>12.2f}{m / n_lat:>12.4f}{m * 1e3 / n_lat / T:>20.3f}   {[round(a, 2) for a in v]}  spread {max(v) - min(v):.2f}")
    for tag, B, T, K in shapes:
        name = f"{tag}_B{B}_T{T}_K{K}"
        r = res[name + "_kws_us"] / res[name + "_align_us"]
        res[name + "_kws_over_align"] = round(r, 3)
        say(f"{name}: search / aligner = {r:.3f} per lattice (spreads {res[name + '_kws_spread_us']:.2f} and {res[name + '_align_spread_us']:.2f} us per call)")
    say()
    say("raw result line:")
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
