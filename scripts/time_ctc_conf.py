"""Time the word / character confidences (ops.ctc_confidence) next to the two lattices they stand on.

T = 501, B = 64, C = 29 logits, every frame valid, one hypothesis of --labels labels per utterance.  The logits are peaked on the
hypothesis (every label holds half of its T // labels frames, then blanks: the layout of scripts/time_ctc_mwer.py), and a unit's
window is the frames its labels own.  Legs:
  lattices       ops.ctc_mwer at K = 1 without gradient: the lse row, alpha and beta, a weights launch          (the yardstick)
  conf_words     ops.ctc_confidence with word units of --word labels each (the last one shorter)
  conf_chars     ops.ctc_confidence with one unit per label
Device events around `iters` back-to-back calls, the legs alternated within every round.  Prints a table with every leg's spread over
the rounds and its difference to the lattices leg (what the unit kernel adds), and one JSON line; --out also writes both to a file.
No threshold is set here."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=501)
    ap.add_argument("--classes", type=int, default=29)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--word", type=int, default=6)
    ap.add_argument("--peak", type=float, default=8.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import ops
    assert torch.cuda.is_available(), "time_ctc_conf.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    B, T, C, U = args.batch, args.frames, args.classes, args.labels
    rng = np.random.default_rng(0)
    hyps = rng.integers(1, C, (B, U)).astype(np.int32)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    span = T // U                                                                      # every label holds span // 2 frames, then blanks
    for b in range(B):
        path = np.zeros(T, np.int64)
        for u in range(U):
            path[u * span:u * span + max(span // 2, 1)] = hyps[b, u]
        x[np.arange(T), b, path] += args.peak
    logits = torch.from_numpy(x).to(dev)
    t = lambda a, dt=torch.int32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)     # noqa: E731
    in_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    lab, off, lens = t(hyps.reshape(-1)), t(np.arange(B, dtype=np.int64) * U, torch.int64), t(np.full(B, U, np.int32))
    risk = torch.zeros((B, 1), dtype=torch.float32, device=dev)

    def units(n):                                                                      # units of n labels: label u owns [u span, (u + 1) span)
        lo = np.arange(0, U, n)
        hi = np.minimum(lo + n, U)
        ts, te = lo * span, hi * span
        te[-1] = T
        rep = lambda a: t(np.tile(a, (B, 1)))                                          # noqa: E731
        return t(np.full(B, len(lo), np.int32)), rep(lo), rep(hi), rep(ts), rep(te)

    calls = {"lattices": lambda: ops.ctc_mwer(logits, lab, off.view(B, 1), lens.view(B, 1), None, in_lens, U, risk, want_grad=False)[1]}
    info = {}
    for name, n in (("conf_words", args.word), ("conf_chars", 1)):
        nu, lo, hi, ts, te = units(n)
        info[name] = dict(units=int(lo.shape[1]), labels_per_unit=n, frames_per_unit=n * span)
        calls[name] = lambda nu=nu, lo=lo, hi=hi, ts=ts, te=te: ops.ctc_confidence(logits, lab, off, lens, in_lens, U, nu, lo, hi, ts, te)[1]
    for k, fn in calls.items():                                                        # warm up every shape of the timed window
        for _ in range(2):
            out = fn()
        assert bool(torch.isfinite(out).all()), f"{k}: a value of the timing batch is not finite"
        if k != "lattices":
            info[k]["mean_confidence"] = round(float(out.exp().mean()), 4)
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                    # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)                    # us per call
    res = dict(B=B, T=T, C=C, labels=U, peak=args.peak, rounds=args.rounds, iters=args.iters, legs=info)
    lines = [f"B = {B}, T = {T}, C = {C}, hypotheses of {U} labels; us per call (device events, {args.iters} calls back to back), median over "
             f"{args.rounds} rounds with their spread; added = over the lattices leg of the same run",
             f"{'leg':<14}{'us/call':>10}{'min':>9}{'max':>9}{'added':>9}   rounds"]
    base = float(np.median(times["lattices"]))
    for k, v in times.items():
        m = float(np.median(v))
        res[k + "_us"], res[k + "_min_us"], res[k + "_max_us"], res[k + "_added_us"] = round(m, 1), round(min(v), 1), round(max(v), 1), round(m - base, 1)
        lines.append(f"{k:<14}{m:>10.1f}{min(v):>9.1f}{max(v):>9.1f}{m - base:>9.1f}   {[round(a, 1) for a in v]}")
    for k, d in info.items():
        lines.append(f"{k}: {d}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
