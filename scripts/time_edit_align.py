"""Time the edit alignment (ops.edit_align) next to the distance kernel it extends (ops.edit_distance), on the same packed problems.

--batch (64) pairs of about --words (30) words of one to nine letters, about 150 characters: pack_scoring's 2 x batch problems, half
over words and half over characters, as Decoder.score_batch / align_batch send them.  The hypothesis is the reference with --wer of its
words replaced, dropped or doubled, so the alignments have all four kinds of step.  Legs:
  distance   ops.edit_distance: the forward pass alone                                                        (the yardstick)
  align      ops.edit_align: the same forward pass with every column kept, the traceback, the two maps
Device events around `iters` back-to-back calls, the legs alternated within every round; the inputs are on the device, so a call is
its launch.  Prints a table with every leg's spread over the rounds and the ratio align / distance, and one JSON line; --out also
writes both to a file.  No threshold is set here."""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pairs(batch, words, wer, seed=0):
    rng = random.Random(seed)
    vocab = ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(1, 10))) for _ in range(500)]
    hyps, refs = [], []
    for _ in range(batch):
        ref = [rng.choice(vocab) for _ in range(max(words + rng.randrange(-5, 6), 1))]
        hyp = []
        for w in ref:
            u = rng.random()
            if u < wer / 3:
                continue
            hyp.append(rng.choice(vocab) if u < 2 * wer / 3 else w)
            if u > 1 - wer / 3:
                hyp.append(rng.choice(vocab))
        hyps.append(" ".join(hyp))
        refs.append(" ".join(ref))
    return hyps, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--words", type=int, default=30)
    ap.add_argument("--wer", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import _lib, ops
    from asr_amd.decoders import pack_scoring
    assert torch.cuda.is_available(), "time_edit_align.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    hyps, refs = make_pairs(args.batch, args.words, args.wer)
    seq, a_off, a_len, b_off, b_len, ref_w, ref_c = pack_scoring(hyps, refs)
    P, max_len = len(a_len), int(max(a_len.max(), b_len.max()))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    d = (t(seq), t(a_off), t(a_len), t(b_off), t(b_len))
    calls = {"distance": lambda: ops.edit_distance(*d, max_len=max_len), "align": lambda: ops.edit_align(*d, max_len=max_len)[0]}
    for fn in calls.values():                                            # warm up both kernels
        for _ in range(3):
            fn()
    dist, counts = calls["distance"]().cpu(), calls["align"]().cpu()
    assert int(counts.min()) >= 0 and torch.equal(counts[:, 1:].sum(1).int(), dist), "the two kernels disagree on the timing batch"
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                      # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)      # us per call
    tot = counts.sum(0).tolist()
    res = dict(pairs=args.batch, problems=P, max_len=max_len, mean_words=round(float(ref_w.mean()), 1), mean_chars=round(float(ref_c.mean()), 1),
               hits=tot[0], substitutions=tot[1], deletions=tot[2], insertions=tot[3], rounds=args.rounds, iters=args.iters,
               workspace_bytes=int(_lib.load().ds2_edit_align_workspace_bytes(P, max_len)))
    lines = [f"{args.batch} pairs of {res['mean_words']} words / {res['mean_chars']} characters on average = {P} problems, longest side {max_len}; "
             f"us per call (device events, {args.iters} calls back to back), median over {args.rounds} rounds with their spread",
             f"{'leg':<10}{'us/call':>10}{'min':>9}{'max':>9}   rounds"]
    for k, v in times.items():
        m = float(np.median(v))
        res[k + "_us"], res[k + "_min_us"], res[k + "_max_us"] = round(m, 1), round(min(v), 1), round(max(v), 1)
        lines.append(f"{k:<10}{m:>10.1f}{min(v):>9.1f}{max(v):>9.1f}   {[round(a, 1) for a in v]}")
    res["ratio"] = round(res["align_us"] / res["distance_us"], 2)
    lines.append(f"ratio align / distance: {res['ratio']}   (steps over all problems: {tot[0]} hits, {tot[1]} substitutions, {tot[2]} deletions, "
                 f"{tot[3]} insertions; workspace {res['workspace_bytes']} bytes)")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
