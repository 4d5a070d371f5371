"""Time the wildcard / free-ends alignment entries (ops.ctc_forced_align_star, ops.ctc_forced_align_star_tiled) next to the plain ones
and their pre-pass (the wildcard row, ds2_ctc_align_star_row_f32) alone.

(a) the shape of scripts/time_align.py: B = 64, T = 501, C = 29, probabilities in (T,B,C) storage, U = 60 (one wavefront per utterance)
    and U = 150 (one workgroup); here the probabilities are a softmax of random logits, not a model's output.
(b) the shape (a) of scripts/time_align_long.py: B = 1, T = 20000, U = 3000, log-probabilities, default tiles.
Legs per shape: plain = the entry without wildcards; star_noop = the wildcard entry on the same input (no wildcard label, NULL flags: the
pre-pass and the STAR instantiation of the lattice are what is added); star = every tenth label and both ends made wildcards, both flags
set; row = the pre-pass alone.  (c) the pre-pass alone on a wide label set, B = 8, T = 501, C = 3000.
Device events around `iters` back-to-back calls, the legs alternated within every round.  Prints a table and one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(dev, B, T, C, U, is_log, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = (torch.randn((T, B, C), generator=g) * 2.0).to(dev)
    x = (torch.log_softmax(z, -1) if is_log else torch.softmax(z, -1)).transpose(0, 1)       # (B,T,C) view of (T,B,C) storage
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, C, (B, U)).astype(np.int32)
    star = lab.copy()
    star[:, ::10] = C
    star[:, -1] = C
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(x=x, U=U, is_log=is_log, targets=t(lab.reshape(-1)), star_targets=t(star.reshape(-1)), off=t(np.arange(B, dtype=np.int32) * U),
                lens=t(np.full(B, U, np.int32)), in_lens=t(np.full(B, T, np.int32)), flags=t(np.full(B, 3, np.int32)),
                g=torch.empty((B, T), dtype=torch.float32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--long-iters", type=int, default=5)
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    from asr_amd import _lib, ops
    assert torch.cuda.is_available(), "time_align_star.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    pen = math.log(0.5)

    def row(p):
        x = p["x"]
        _lib.check(lib.ds2_ctc_align_star_row_f32(x.data_ptr(), x.stride(0), x.stride(1), x.shape[0], x.shape[1], x.shape[2],
                                                  1 if p["is_log"] else 0, p["in_lens"].data_ptr(), pen, p["g"].data_ptr(), None),
                   "ds2_ctc_align_star_row_f32")

    calls, iters = {}, {}
    for U in (60, 150):
        p = problem(dev, 64, 501, 29, U, False, U)
        a = lambda p=p, tg="targets": (p["x"], p[tg], p["off"], p["in_lens"], p["lens"], p["U"], p["is_log"])
        calls[f"a_plain_U{U}"] = lambda a=a: ops.ctc_forced_align(*a(), 0)
        calls[f"a_star_noop_U{U}"] = lambda a=a: ops.ctc_forced_align_star(*a(), 0, star_penalty=pen, flags=None)
        calls[f"a_star_U{U}"] = lambda a=a, p=p: ops.ctc_forced_align_star(*a(tg="star_targets"), 0, star_penalty=pen, flags=p["flags"])
    calls["a_row_alone"] = lambda p=p: row(p)
    if not args.skip_long:
        q = problem(dev, 1, 20000, 29, 3000, True, 7)
        b = lambda tg="targets": (q["x"], q[tg], q["off"], q["in_lens"], q["lens"], q["U"], True)
        calls["b_tiled_plain"] = lambda: ops.ctc_forced_align_tiled(*b())
        calls["b_tiled_star_noop"] = lambda: ops.ctc_forced_align_star_tiled(*b(), star_penalty=pen, flags=None)
        calls["b_tiled_star"] = lambda: ops.ctc_forced_align_star_tiled(*b("star_targets"), star_penalty=pen, flags=q["flags"])
        calls["b_row_alone"] = lambda: row(q)
        iters.update({k: args.long_iters for k in calls if k.startswith("b_tiled")})
    w = problem(dev, 8, 501, 3000, 4, True, 9)
    calls["c_row_alone_C3000"] = lambda: row(w)
    for k, fn in calls.items():                                                      # warm up every shape of the timed window
        for _ in range(3):
            out = fn()
        if out is not None:
            assert bool(torch.isfinite(out[0]).all()), f"{k}: an utterance of the timing batch is infeasible"
    torch.cuda.synchronize()
    for U in (60, 150):                                                              # the no-op legs write the plain entry's bits
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                   for x, y in zip(calls[f"a_plain_U{U}"](), calls[f"a_star_noop_U{U}"]()))
        print(f"U = {U}: star entry without wildcards equals the plain entry bit for bit: {same}")
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                  # the legs alternate within a round
            n = iters.get(k, args.iters)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / n)                           # us per call
    res = dict(rounds=args.rounds, iters=args.iters, long_iters=args.long_iters)
    print(f"us per call (device events, {args.iters} calls back to back; b_tiled legs {args.long_iters}), mean over {args.rounds} rounds [rounds] spread = max - min")
    print(f"{'leg':<22}{'us/call':>10}   rounds")
    for k, v in times.items():
        m = float(np.mean(v))
        res[k + "_us"], res[k + "_us_rounds"], res[k + "_spread_us"] = round(m, 2), [round(a, 2) for a in v], round(max(v) - min(v), 2)
        print(f"{k:<22}{m:>10.2f}   {[round(a, 2) for a in v]}  spread {max(v) - min(v):.2f}")
    for k, p in (("a_row_alone", p), ("c_row_alone_C3000", w)) + ((("b_row_alone", q),) if not args.skip_long else ()):
        nbytes = p["x"].numel() * 4 + p["g"].numel() * 4
        res[k + "_GBps"] = round(nbytes / (res[k + "_us"] * 1e-6) / 1e9, 1)
        print(f"{k}: {nbytes / 1e6:.2f} MB read and written, {res[k + '_GBps']} GB/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
