"""Time the streaming beam search (ops.ctc_beam_stream_feed, csrc/ctc_beam_stream.h) next to the one-call decode of the same frames.

Planted posteriors, C = 29: words of a synthetic vocabulary (scripts/make_synthetic_arpa.py, 2000 words, 20 000 n-grams, order 3)
separated by spaces, every character 2 .. 4 frames at 0.6 with the rest spread over the other classes, one soft-blank frame after it.
  batch  B = 64, T = 501, K = 100, plain (cutoff_top_n 40) and word LM (cutoff_top_n 38, alpha 0.8, beta 1.0):
           one-call   ops.ctc_beam_decode
           stream     the same frames in chunks of 50 and of 250 frames, without read-outs and with one read-out (n_out = 1) per chunk,
                      the final read-out (n_out = K) included in both
  long   B = 1, T = 30 000, K = 16, plain, the planted recording of scripts/time_transcribe_long.py: one-call against 1000-frame chunks
         (nodes allocated for the whole recording; BeamStream's doubling adds its copies, timed separately as `grow`)
Device events around each leg, the median of --reps calls after one warm-up, spread = max - min.  --one-call times the one-call legs
alone: run it from a checkout of another commit (--root) in the same session to compare two builds of the same kernel instances.
Each leg is one process-local measurement; nothing here times the hour-long one-utterance decode (it did not finish within seven minutes,
for a reason nobody has established).  Prints a table and one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = "_'abcdefghijklmnopqrstuvwxyz "


def planted(B, T, words, seed):
    """(B, T, 29) float32 probabilities on the host spelling dictionary words"""
    rng = np.random.default_rng(seed)
    C = len(LABELS)
    x = np.empty((B, T, C), dtype=np.float32)
    for b in range(B):
        kinds = []
        while len(kinds) < T:
            w = words[int(rng.integers(0, len(words)))] + " "
            for ch in w:
                kinds += [LABELS.index(ch)] * int(rng.integers(2, 5)) + [0]
        kinds = np.array(kinds[:T])
        u = rng.random(T)
        pb = np.where(kinds == 0, 0.5, 0.05 + 0.25 * u)
        pl = np.where(kinds > 0, 0.6, 0.0)
        x[b] = np.repeat(((1.0 - pb - pl) / (C - 1 - (kinds > 0)))[:, None], C, 1)
        x[b, :, 0] = pb
        x[b, kinds > 0, kinds[kinds > 0]] = 0.6
    return x


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 3), "spread": round(ms[-1] - ms[0], 3)}


def stream_fn(ops, x, K, chunk, partial, search, grow=False):
    """one whole stream over x (B, T, C) on the device: fresh state, feeds of `chunk` frames, the final read-out"""
    B, T, C = x.shape
    dev = x.device

    def run():
        state = ops.ctc_beam_stream_state(B, K, search.get("lm"), search.get("hotwords"), dev)
        cap = 256 if grow else T
        nodes = ops.ctc_beam_stream_nodes(B, cap, K, dev)
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            if t0 + n > cap:
                new = cap
                while new < t0 + n:
                    new *= 2
                nodes, cap = ops.ctc_beam_stream_nodes(B, new, K, dev, nodes, cap), new
            ops.ctc_beam_stream_feed(x[:, t0:t0 + n], None, state, nodes, cap, t0, 1 if partial else 0, beam_width=K, **search)
        return ops.ctc_beam_stream_feed(None, None, state, nodes, cap, T, K, beam_width=K, classes=C, **search)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-call", action="store_true", help="the one-call legs of the batch shape alone")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose asr_amd is timed")
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    sys.path.insert(0, HERE)
    from asr_amd import ops
    from asr_amd.decoders import BeamCTCDecoder
    from make_synthetic_arpa import make
    dev = torch.device("cuda", 0)
    B, T, K = 64, 501, 100
    with tempfile.TemporaryDirectory() as tmp:
        arpa = os.path.join(tmp, "word3.arpa")
        make(arpa, "word", 3, 20000, 2000, 0)
        lm = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, lm_path=arpa).lm
        with open(arpa) as f:
            text = f.read()
    unigrams = text[text.index("\\1-grams:"):text.index("\\2-grams:")].splitlines()[1:]
    words = [ln.split("\t")[1] for ln in unigrams if "\t" in ln and not ln.split("\t")[1].startswith("<")]
    x = torch.from_numpy(planted(B, T, words, 1)).to(dev)
    arms = {"plain": dict(cutoff_top_n=40), "word_lm": dict(cutoff_top_n=38, lm=lm, alpha=0.8, beta=1.0)}
    res = {"root": os.path.relpath(args.root), "batch": {"B": B, "T": T, "K": K}, "reps": args.reps, "legs": {}}
    lines = [f"# python scripts/time_beam_stream.py {' '.join(sys.argv[1:])}",
             "# ms: median of %d calls after a warm-up (spread = max - min); ratio = leg / one-call of the same run" % args.reps,
             f"{'leg':34s} {'ms':>10s} {'spread':>8s} {'ratio':>6s}"]

    def leg(name, fn, base=None, reps=args.reps):
        r = timed(fn, reps)
        if base is not None:
            r["ratio"] = round(r["ms"] / base["ms"], 3)
        res["legs"][name] = r
        lines.append(f"{name:34s} {r['ms']:10.3f} {r['spread']:8.3f} {r.get('ratio', 1.0):6.3f}")
        print(lines[-1], flush=True)
        return r

    for arm, search in arms.items():
        one = leg(f"B64 {arm} one-call", lambda: ops.ctc_beam_decode(x, None, 0, K, **search))
        if args.one_call:
            continue
        # the stream must give the one-call decode's bits before its time means anything
        want, got = ops.ctc_beam_decode(x, None, 0, K, **search), stream_fn(ops, x, K, 50, True, search)()
        assert torch.equal(got[2], want[2]) and torch.equal(got[3].view(torch.int32), want[3].view(torch.int32))
        assert torch.equal(got[0][:, :, :T], want[0]) and torch.equal(got[1][:, :, :T], want[1])
        for chunk in (50, 250):
            for partial in (False, True):
                leg(f"B64 {arm} stream {chunk}{' +partial' if partial else ''}", stream_fn(ops, x, K, chunk, partial, search), one)
    if not args.one_call and not args.skip_long:
        from time_transcribe_long import posteriors
        y = torch.from_numpy(posteriors(30000, len(LABELS), 30000)).to(dev)[None]
        plain = dict(cutoff_top_n=40)
        one = leg("B1 T30000 K16 one-call", lambda: ops.ctc_beam_decode(y, None, 0, 16, **plain), reps=3)
        leg("B1 T30000 K16 stream 1000", stream_fn(ops, y, 16, 1000, False, plain), one, reps=3)
        leg("B1 T30000 K16 stream 1000 +partial", stream_fn(ops, y, 16, 1000, True, plain), one, reps=3)
        leg("B1 T30000 K16 stream 1000 grow", stream_fn(ops, y, 16, 1000, False, plain, grow=True), one, reps=3)
    lines.append(json.dumps(res))
    print(lines[-1])
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
