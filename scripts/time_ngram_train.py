"""Time the n-gram estimation (asr_amd/decoders/lm_train.py, ops.ngram_*, csrc/ngram_train.h) leg by leg on Zipf corpora.

Corpora: tokens drawn with weights 1 / (i + 1); "char": 26 letters (n_vocab = 29 with <unk>, <s>, </s>), order 5, sentences of 1..80
characters; "word": 50 000 words, order 3, sentences of 1..24 words.  Sizes: --sizes tokens (default 1e6 and 1e7).
Legs, wall clock with a device synchronisation on either side, the median of --reps runs (--host-reps for the legs that run on the
host) and spread = max - min:
  tokenise   lm_train.tokenize on the sentence strings (Python)
  count      ops.ngram_count: the tables' allocation and clearing, and the counting launch
  solve      ops.ngram_solve: the adjusted-count launches, the count-of-counts download, the probability launches
  collect    ops.ngram_collect: the sort of the distinct entries by key on the device and their download
  write      NgramEstimate(...).write_arpa to a temporary file (Python)
  host twin  ops.ngram_estimate_host on the same ids (std::unordered_map, one thread)
There is no parent or reference path to compare with: the kernel legs stand against the host twin only.  NOT measured here: merging the
duplicates of a wave before the atomic, sizes beyond --sizes, more than one GPU.  Prints a table and one JSON line per corpus."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CONFIGS = {"char": dict(n_tokens_vocab=26, order=5, max_len=80, mode="char"), "word": dict(n_tokens_vocab=50000, order=3, max_len=24, mode="word")}


def corpus(kind, n_tokens, seed=0):
    """sentence strings of a Zipf corpus with n_tokens tokens in all"""
    cfg = CONFIGS[kind]
    rng = np.random.default_rng(seed)
    V = cfg["n_tokens_vocab"]
    w = 1.0 / (np.arange(V) + 1.0)
    ids = rng.choice(V, size=n_tokens, p=w / w.sum())
    lens = rng.integers(1, cfg["max_len"] + 1, size=3 * n_tokens // cfg["max_len"] + 2)
    cuts = np.minimum(np.concatenate(([0], np.cumsum(lens))), n_tokens)
    cuts = cuts[:int(np.searchsorted(cuts, n_tokens)) + 1]
    if kind == "char":
        text = (ids + 97).astype(np.uint8).tobytes().decode("ascii")
        return [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    words = np.array([f"w{i}" for i in range(V)], dtype=object)[ids]
    return [" ".join(words[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def timed(fn, reps, sync):
    out, ts = None, []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    ts.sort()
    return out, {"s": round(ts[len(ts) // 2], 4), "spread": round(ts[-1] - ts[0], 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=float, nargs="+", default=[1e6, 1e7])
    ap.add_argument("--kinds", nargs="+", default=list(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import ops
    from asr_amd.decoders import lm_train
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"n-gram estimation, {torch.cuda.get_device_name(0)}; seconds, median of reps, spread = max - min")
    for kind in args.kinds:
        cfg = CONFIGS[kind]
        for size in args.sizes:
            n = int(size)
            sentences = corpus(kind, n)
            legs = {}
            (vocab, flat, offsets, n_empty), legs["tokenise"] = timed(lambda: lm_train.tokenize(sentences, cfg["mode"]), args.host_reps, False)
            d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
            ops.ngram_solve(ops.ngram_count(d_flat[:1000], torch.tensor([0, 1000], device=dev), len(vocab), cfg["order"]))   # warm-up
            st, legs["count"] = timed(lambda: ops.ngram_count(d_flat, d_off, len(vocab), cfg["order"]), args.reps, True)
            # solve is timed on a fresh count each time (it adds into the tables)
            ts = []
            for _ in range(args.reps):
                st = ops.ngram_count(d_flat, d_off, len(vocab), cfg["order"])
                _, one = timed(lambda: ops.ngram_solve(st), 1, True)
                ts.append(one["s"])
            ts.sort()
            legs["solve"] = {"s": ts[len(ts) // 2], "spread": round(ts[-1] - ts[0], 4), "reps": args.reps}
            raw, legs["collect"] = timed(lambda: ops.ngram_collect(st), args.reps, True)
            est = lm_train.NgramEstimate(raw, cfg["mode"], vocab, int(flat.size), len(offsets) - 1, n_empty)
            with tempfile.TemporaryDirectory() as d:
                _, legs["write"] = timed(lambda: est.write_arpa(os.path.join(d, "m.arpa")), args.host_reps, False)
                file_mb = os.path.getsize(os.path.join(d, "m.arpa")) / 1e6
            host, legs["host twin"] = timed(lambda: ops.ngram_estimate_host(flat, offsets, len(vocab), cfg["order"]), args.host_reps, False)
            agree = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                        for a, b in zip(raw["orders"], host["orders"]))
            distinct = [len(sec[0]) for sec in raw["orders"]]
            say(f"{kind} order {cfg['order']}, {n} tokens, {len(offsets) - 1} sentences, n_vocab {len(vocab)}: distinct {distinct}, "
                f"slots {st['slots']}, file {file_mb:.1f} MB, fallback orders {raw['fallback_orders']}, integers equal the host twin's: {agree}")
            for name, r in legs.items():
                say(f"  {name:10s} {r['s']:10.4f} s   spread {r['spread']:8.4f}   ({r['reps']} reps)")
            kernels, end_to_end = legs["count"]["s"] + legs["solve"]["s"], sum(r["s"] for k, r in legs.items() if k != "host twin")
            say(f"  count + solve {kernels:.4f} s against the host twin's {legs['host twin']['s']:.4f} s; end to end {end_to_end:.2f} s, "
                f"of which tokenise + write {legs['tokenise']['s'] + legs['write']['s']:.2f} s")
            say(json.dumps({"kind": kind, "tokens": n, "order": cfg["order"], "distinct": distinct, "legs": legs, "agree": agree}))


if __name__ == "__main__":
    main()
