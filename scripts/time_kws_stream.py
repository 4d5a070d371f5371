"""Time the streaming keyword search (ops.ctc_kws_stream_feed) next to the one-call search (ops.ctc_keyword_search) on the same frames.

(1) the one-call ENTRY, ds2_ctc_kws_f32 with preallocated outputs and workspace, on this library and, with --parent-lib, on a library
    built from the parent commit, both loaded into this process, writing the same buffers, and run as this, parent, parent, this within
    every round, after one untimed visit (the first leg after another shape's legs is slower, whichever library it calls): the one-call kernel instances are the same code in both, so a difference beyond the spread of repeated runs would
    be a defect.
(2) a whole stream over the same frames in chunks of 250 / 50 / 10 frames (a fresh state, every chunk one feed, the last with finish),
    as a multiple of one ops.ctc_keyword_search call.  Both sides go through their ops wrapper, which allocates the outputs of
    every call; a feed is three launches like the one call.
(3) an hour (B = 1, T = 180000, K = 16) in 1000-frame chunks against the one call.
(4) the state bytes per (utterance, keyword).
(a) B = 64, T = 501, C = 29, probabilities in (T,B,C) storage (a softmax of random logits, not a model's output), K = 1, 16, 128 keywords
of 8 labels, thresholds U * log(0.5), max_hits 32, pending 1024.  Device events around `iters` back-to-back repetitions, the legs
alternated within every round.  Prints a table and one JSON line, and writes both to --out."""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PENDING, MAX_HITS = 1024, 32


def problem(dev, B, T, C, K, U, seed):
    """the batches of scripts/time_kws.py (the same seeds), without the aligner's copies"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = (torch.randn((T, B, C), generator=g) * 2.0).to(dev)
    x = torch.softmax(z, -1).transpose(0, 1)                                               # (B,T,C) view of (T,B,C) storage
    lab = np.random.default_rng(seed).integers(1, C, (K, U)).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(x=x, U=U, K=K, labels=t(lab.reshape(-1)), off=t(np.arange(K, dtype=np.int32) * U), lens=t(np.full(K, U, np.int32)),
                thr=t(np.full(K, U * math.log(0.5), np.float32)), in_lens=t(np.full(B, T, np.int32)))


def entry_buffers(lib, p, dev):
    """the outputs and the workspace of ds2_ctc_kws_f32 on problem p, allocated once and shared by the two libraries' legs"""
    B, T, _ = p["x"].shape
    K = p["K"]
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    return (f32(B, K, T), i32(B, K, T), i32(B, K, MAX_HITS), i32(B, K, MAX_HITS), f32(B, K, MAX_HITS), i32(B, K),
            torch.empty(lib.ds2_ctc_kws_workspace_bytes(B, T, K, MAX_HITS), dtype=torch.uint8, device=dev))


def entry_call(lib, p, bufs):
    """ds2_ctc_kws_f32 of `lib` on problem p into bufs -> a function of no arguments"""
    B, T, C = p["x"].shape
    K = p["K"]
    keep = fs, fst, hs, he, hv, nh = bufs[:6]
    ws = bufs[6]
    wsb = ws.numel()
    assert wsb == lib.ds2_ctc_kws_workspace_bytes(B, T, K, MAX_HITS)
    args = (p["x"].data_ptr(), p["x"].stride(0), p["x"].stride(1), B, T, C, 0, p["in_lens"].data_ptr(), p["labels"].data_ptr(), p["off"].data_ptr(),
            p["lens"].data_ptr(), K, p["U"], p["thr"].data_ptr(), MAX_HITS, fs.data_ptr(), fst.data_ptr(), hs.data_ptr(), he.data_ptr(),
            hv.data_ptr(), nh.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)

    def call(keep=keep, ws=ws):
        assert lib.ds2_ctc_kws_f32(*args) == 0
        return keep
    return call


def stream_call(ops, p, chunk, dev):
    """a whole stream over p's frames in feeds of `chunk` frames, from a zeroed state to the finish -> a function of no arguments"""
    B, T, _ = p["x"].shape
    state = ops.ctc_kws_stream_state(B, p["K"], PENDING, dev)
    cuts = list(range(0, T, chunk))

    def call(count=False):
        """count: -> (final hits over all feeds, candidates dropped), device scalars, for the check against the one call"""
        state.zero_()
        finals = 0
        for t0 in cuts:
            out = ops.ctc_kws_stream_feed(p["x"][:, t0:t0 + chunk], None, state, p["labels"], p["off"], p["lens"], p["U"], p["thr"], PENDING, t0,
                                          False, MAX_HITS, None, t0 + chunk >= T)
            if count:
                finals = finals + out[3].sum()
        return (finals, out[8].sum()) if count else out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--long-iters", type=int, default=3)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libds2hip.so built from the parent commit, for leg (1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kws_stream_timing.txt"))
    args = ap.parse_args()
    from asr_amd import _lib, ops
    assert torch.cuda.is_available(), "time_kws_stream.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("ds2_ctc_kws_workspace_bytes", "ds2_ctc_kws_f32"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    calls, iters, base = {}, {}, {}
    shapes = [("a", 64, 501, K, (250, 50, 10)) for K in (1, 16, 128)] + ([] if args.skip_long else [("b", 1, 180000, 16, (1000,))])
    for tag, B, T, K, chunks in shapes:
        p = problem(dev, B, T, 29, K, 8, K)
        name = f"{tag}_B{B}_T{T}_K{K}"
        bufs = entry_buffers(lib, p, dev)
        legs = {"_entry_this": entry_call(lib, p, bufs)}
        if parent is not None:
            legs["_entry_parent"] = entry_call(parent, p, bufs)
        legs["_onecall"] = lambda p=p: ops.ctc_keyword_search(p["x"], p["labels"], p["off"], p["lens"], p["U"], p["thr"], p["in_lens"], False, MAX_HITS)
        for c in chunks:
            legs[f"_stream{c}"] = stream_call(ops, p, c, dev)
        for leg, fn in legs.items():
            calls[name + leg], base[name + leg] = fn, name
            if tag == "b":
                iters[name + leg] = args.long_iters
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Streaming keyword search against the one-call search (scripts/time_kws_stream.py; {torch.cuda.get_device_name(0)}, one process; "
        f"library {_lib.version()})")
    say(f"C = 29, probabilities, keywords of 8 labels, thresholds 8 log 0.5, max_hits {MAX_HITS}, pending {PENDING}; entry = ds2_ctc_kws_f32 with "
        "preallocated buffers")
    say("(this library / the parent commit's); onecall = ops.ctc_keyword_search; streamN = a zeroed state, then ops.ctc_kws_stream_feed per N frames")
    say(f"state: {lib.ds2_ctc_kws_stream_state_bytes(1, 1, PENDING)} bytes per (utterance, keyword) at pending {PENDING} "
        f"(4 * (264 + 3 * pending); {lib.ds2_ctc_kws_stream_state_bytes(1, 1, 64)} at pending 64)")
    for k, fn in calls.items():                                                            # warm up every shape of the timed window
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        if k.endswith("_onecall"):
            want = out
        elif "_stream" in k:                                                               # (the tests compare the hits themselves)
            finals, dropped = fn(count=True)
            say(f"{k}: {int(finals)} final hits over the stream, the one call has {int(want[5].clamp(max=MAX_HITS).sum())}; {int(dropped)} candidates dropped")
            assert int(finals) == int(want[5].clamp(max=MAX_HITS).sum()) and int(dropped) == 0
    times, visits = {k: [] for k in calls}, {}
    # The legs alternate within a round.  The first visits after the host-bound stream legs of the previous shape run slower than later
    # ones, whichever library they call (while this script was written: by up to 7 % at K = 128, fading over some 20 ms), so the two
    # entry legs of a shape run as this (four untimed visits), this, parent, parent, this.
    order = []
    for k in calls:
        order += [(k, False)] * 4 + [(k, True)] if k.endswith("_entry_this") else [(k, True)]
        if k.endswith("_entry_parent"):
            order += [(k, True), (k[:-len("parent")] + "this", True)]
    for _ in range(args.rounds):
        visit = {k: [] for k in calls}
        for k, timed in order:
            fn, n = calls[k], iters.get(k, args.iters)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            if timed:
                visit[k].append(e0.elapsed_time(e1) * 1e3 / n)                             # us per repetition
        for k, v in visit.items():
            times[k].append(float(np.mean(v)))
            if len(v) > 1:
                visits.setdefault(k, []).append([round(a, 2) for a in v])
    res = dict(rounds=args.rounds, iters=args.iters, long_iters=args.long_iters, pending=PENDING,
               state_bytes_per_pair=lib.ds2_ctc_kws_stream_state_bytes(1, 1, PENDING))
    say(f"us per repetition (device events, {args.iters} back to back; the b legs {args.long_iters}), mean over {args.rounds} rounds, spread = max - min")
    say(f"{'leg':<34}{'us':>12}{'x onecall':>11}   rounds")
    for k, v in times.items():
        m = float(np.mean(v))
        res[k + "_us"], res[k + "_us_rounds"], res[k + "_spread_us"] = round(m, 2), [round(a, 2) for a in v], round(max(v) - min(v), 2)
    for k, v in times.items():
        r = res[k + "_us"] / res[base[k] + "_onecall_us"]
        if "_stream" in k:
            res[k + "_over_onecall"] = round(r, 3)
        say(f"{k:<34}{res[k + '_us']:>12.2f}{r:>11.3f}   {res[k + '_us_rounds']}  spread {res[k + '_spread_us']:.2f}")
    if parent is not None:
        for tag, B, T, K, _ in shapes:
            name = f"{tag}_B{B}_T{T}_K{K}"
            d = res[name + "_entry_this_us"] - res[name + "_entry_parent_us"]
            res[name + "_entry_this_minus_parent_us"] = round(d, 2)
            say(f"{name}: one-call entry, this - parent = {d:+.2f} us (spreads {res[name + '_entry_this_spread_us']:.2f} and "
                f"{res[name + '_entry_parent_spread_us']:.2f} us); the two visits of every round: this {visits[name + '_entry_this']}, "
                f"parent {visits[name + '_entry_parent']}")
    say()
    say("raw result line:")
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
