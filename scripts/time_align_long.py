"""Time the tiled CTC forced alignment (ops.ctc_forced_align_tiled) on long recordings.

(a) B = 1, T = 20 000, U = 3 000: the largest shape that the one-workgroup kernel (ops.ctc_forced_align, variant 2) also runs; the two
    are timed on the same input, the legs alternated within every round, and their outputs are compared bit for bit first.
(b) the same problem over a grid of tile shapes (tile_frames x tile_pairs), to choose the library's defaults.
(c) B = 1, T = 180 000, U = 50 000: an hour of speech, tiled only (default tiles, and any shapes given with --hour-tiles).
Input: log-softmax of seeded normal logits, C = 29, random labels; every problem is checked to be feasible.  Device events around
`iters` back-to-back calls (each call is the fill launch, one launch per anti-diagonal of tiles and the backtrace launch; the
workspace allocation comes from the caching allocator after the warm-up).  Prints a table, writes it to --out with one JSON line.
(Kernel-only times: run this under `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(dev, T, U, C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.log_softmax(torch.randn((1, T, C), generator=g) * 2.0, dim=-1).to(dev)
    lab = torch.randint(1, C, (U,), generator=g, dtype=torch.int32).to(dev)
    z = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    return dict(x=x, targets=lab, off=z(0), in_lens=z(T), lens=z(U), U=U, T=T)


def timed(calls, rounds, iters):
    """us per call of every leg: device events around `iters` back-to-back calls, the legs alternated within every round."""
    for fn in calls.values():                                                        # warm up every shape of the timed window
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--labels", type=int, default=3000)
    ap.add_argument("--grid-frames", default="64,256,1024")
    ap.add_argument("--grid-pairs", default="64,256,1024")
    ap.add_argument("--hour-frames", type=int, default=180000)
    ap.add_argument("--hour-labels", type=int, default=50000)
    ap.add_argument("--hour-tiles", default="", help="further tile shapes for (c), e.g. 256x64,1024x1024")
    ap.add_argument("--no-hour", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_long_timing.txt"))
    args = ap.parse_args()
    from asr_amd import _lib, ops
    assert torch.cuda.is_available(), "time_align_long.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    C = 29
    lines, res = [], dict(C=C, rounds=args.rounds, iters=args.iters)

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def tiled(g, tf=0, tp=0):
        return ops.ctc_forced_align_tiled(g["x"], g["targets"], g["off"], g["in_lens"], g["lens"], g["U"], True, tf, tp)

    def report(times, T):
        say(f"{'leg':<26}{'us/call':>12}{'us/frame':>10}   rounds")
        for k, v in times.items():
            m = float(np.mean(v))
            res[k + "_us"], res[k + "_us_rounds"], res[k + "_spread_us"] = round(m, 1), [round(a, 1) for a in v], round(max(v) - min(v), 1)
            say(f"{k:<26}{m:>12.1f}{m / T:>10.4f}   {[round(a, 1) for a in v]}  spread {max(v) - min(v):.1f}")

    say(f"Tiled CTC forced alignment (scripts/time_align_long.py; MI355X, one process; library {_lib.version()})")
    say(f"us per call, device events around {args.iters} calls back to back, mean over {args.rounds} rounds [rounds] spread = max - min; "
        "log-probability input, C = 29, B = 1")
    # (a) against the one-workgroup kernel
    g = problem(dev, args.frames, args.labels, C, 1)
    plain = lambda: ops.ctc_forced_align(g["x"], g["targets"], g["off"], g["in_lens"], g["lens"], g["U"], True, 2)
    ref, got = plain(), tiled(g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref[0]).all()), "the timing problem is infeasible"
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ref, got))
    assert same, "the tiled lattice and variant 2 disagree"
    say()
    say(f"(a) T = {g['T']}, U = {g['U']}: default tiles against ops.ctc_forced_align(variant=2) (one workgroup); outputs equal bit for bit: {same}")
    report(timed({"a_variant2_one_workgroup": plain, "a_tiled_default": lambda: tiled(g)}, args.rounds, args.iters), g["T"])
    res["a_tiled_over_variant2"] = round(res["a_tiled_default_us"] / res["a_variant2_one_workgroup_us"], 3)
    say(f"tiled / one workgroup = {res['a_tiled_over_variant2']}")
    # (b) the tile shapes
    shapes = [(tf, tp) for tf in map(int, args.grid_frames.split(",")) for tp in map(int, args.grid_pairs.split(","))]
    for tf, tp in shapes:
        out = tiled(g, tf, tp)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ref, out)), (tf, tp)
    say()
    say(f"(b) the same problem by tile shape (tile_frames x tile_pairs; 64 pairs = one wavefront per tile, DPP instead of the LDS row); "
        "every shape's outputs equal variant 2's bit for bit")
    report(timed({f"b_tiled_{tf}x{tp}": (lambda tf=tf, tp=tp: tiled(g, tf, tp)) for tf, tp in shapes}, args.rounds, args.iters), g["T"])
    best = min(shapes, key=lambda s: res[f"b_tiled_{s[0]}x{s[1]}_us"])
    res["b_fastest"] = f"{best[0]}x{best[1]}"
    say(f"fastest: {best[0]} frames x {best[1]} pairs")
    # (c) an hour
    if not args.no_hour:
        h = problem(dev, args.hour_frames, args.hour_labels, C, 2)
        hour = [(0, 0)] + [tuple(int(v) for v in s.split("x")) for s in args.hour_tiles.split(",") if s]
        outs = [tiled(h, tf, tp) for tf, tp in hour]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(outs[0][0]).all()), "the hour problem is infeasible"
        for o in outs[1:]:
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0], o))
        del outs
        wsb = _lib.load().ds2_ctc_align_tiled_workspace_bytes(1, h["T"], h["U"], 0, 0)
        say()
        say(f"(c) T = {h['T']}, U = {h['U']} (an hour of speech), tiled only; workspace {wsb / 1e9:.2f} GB; "
            f"score {float(tiled(h)[0][0]):.1f}; the shapes' outputs equal one another bit for bit")
        names = {f"c_hour_tiled_{'default' if (tf, tp) == (0, 0) else f'{tf}x{tp}'}": (lambda tf=tf, tp=tp: tiled(h, tf, tp)) for tf, tp in hour}
        report(timed(names, max(2, args.rounds - 1), max(2, args.iters // 2)), h["T"])
    else:
        say()
        say("(c) an hour of speech: not measured in this run (--no-hour)")
    say()
    say("Not pinned: parity with any external aligner, and what a window edge of DeepSpeech.posteriors_long costs in accuracy (unmeasured).")
    say()
    say("raw result line:")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
