"""Time the wildcard CTC loss (ops.ctc_star_loss) next to the plain loss (ops.ctc_loss) of the same run.

T = 501, B = 64, C = 29 logits (unit variance x 2, every frame valid); targets of 60 labels (the one-wavefront lattice) and of 150 labels
(the one-workgroup lattice).  Legs, each with the gradient pass and without it (lattice only):
  plain       ops.ctc_loss
  star_same   ops.ctc_star_loss on the same targets, no flags        (the STAR instances doing the plain loss's work)
  star_wild   ops.ctc_star_loss with a wildcard in every eighth position and both end flags set
Device events around `iters` back-to-back calls, the legs alternated within every round.  Prints a table with the ratio of every leg to
the plain leg of the same shape, and one JSON line; --out also writes the table to a file.  No threshold is set here: the ratios are
the result."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import ops
    assert torch.cuda.is_available(), "time_ctc_star.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    B, T, C = args.batch, args.frames, args.classes
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.standard_normal((T, B, C)) * 2.0).astype(np.float32)).to(dev)
    in_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    pen = float(np.log(0.5))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                  # noqa: E731
    calls = {}
    for U in (60, 150):
        lab = rng.integers(1, C, (B, U)).astype(np.int32)
        wild = lab.copy()
        wild[:, 3::8] = C
        off, lens = t(np.arange(B, dtype=np.int32) * U), t(np.full(B, U, np.int32))
        flags = t(np.full(B, 3, np.int32))
        tp, tw = t(lab.reshape(-1)), t(wild.reshape(-1))
        for g in (True, False):
            sfx = f"U{U}" + ("" if g else "_nograd")
            calls[f"plain_{sfx}"] = lambda tp=tp, off=off, lens=lens, U=U, g=g: ops.ctc_loss(logits, tp, off, in_lens, lens, U, 1.0, want_grad=g)
            calls[f"star_same_{sfx}"] = lambda tp=tp, off=off, lens=lens, U=U, g=g: ops.ctc_star_loss(logits, tp, off, in_lens, lens, U, 1.0,
                                                                                                 star_penalty=pen, want_grad=g)
            calls[f"star_wild_{sfx}"] = lambda tw=tw, off=off, lens=lens, U=U, g=g: ops.ctc_star_loss(logits, tw, off, in_lens, lens, U, 1.0,
                                                                                                 star_penalty=pen, flags=flags, want_grad=g)
    for k, fn in calls.items():                                                      # warm up every shape of the timed window
        for _ in range(5):
            out = fn()
        assert bool(torch.isfinite(out[0]).all()), f"{k}: an utterance of the timing batch is infeasible"
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                  # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)                  # us per call
    res = dict(B=B, T=T, C=C, rounds=args.rounds, iters=args.iters)
    lines = [f"B = {B}, T = {T}, C = {C}; us per call (device events, {args.iters} calls back to back), mean over {args.rounds} rounds; "
             "ratio = to the plain leg of the same shape in the same run",
             f"{'leg':<26}{'us/call':>10}{'us/frame':>10}{'ratio':>8}   rounds"]
    for k, v in times.items():
        m = float(np.mean(v))
        base = float(np.mean(times["plain_" + k.split("_U", 1)[1].join(["U", ""])]))
        res[k + "_us"], res[k + "_us_rounds"], res[k + "_ratio"] = round(m, 2), [round(a, 2) for a in v], round(m / base, 4)
        lines.append(f"{k:<26}{m:>10.2f}{m / T:>10.4f}{m / base:>8.3f}   {[round(a, 2) for a in v]}  spread {max(v) - min(v):.2f}")
    for U in (60, 150):                                                              # what the gradient pass alone costs
        for leg in ("plain", "star_same", "star_wild"):
            res[f"{leg}_U{U}_grad_pass_us"] = round(res[f"{leg}_U{U}_us"] - res[f"{leg}_U{U}_nograd_us"], 2)
        lines.append(f"gradient pass alone, U = {U} (with - without): plain {res[f'plain_U{U}_grad_pass_us']} us, star_same "
                     f"{res[f'star_same_U{U}_grad_pass_us']} us, star_wild {res[f'star_wild_U{U}_grad_pass_us']} us")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
