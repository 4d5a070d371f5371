"""Time the word-LM beam search against the SIZE of its language model: one width-100 decode of B = 64 utterances of T = 501 frames
(cutoff_top_n 38, alpha 0.8, beta 1.0, as scripts/time_beam_stream.py) with the full model of a Zipf word corpus (scripts/
time_ngram_train.py, --tokens words, order 3) and with the same model pruned at --thetas, all estimated in this process.

The posteriors spell held-out sentences of the corpus (the last 10 %): every character for one frame, a blank frame after it, the
label's logit raised by --peak over unit-variance noise, so that the beams carry real words of the vocabulary and their neighbours and
the search probes the hashed table (csrc/ctc_lm.h) at every word end.  The 13 labels are "_w0123456789 ".
The decoders are alternated over --rounds rounds, one decode each per round and each round starting with another model, timed by
device events after one warm-up decode each; the median and spread = max - min per model are reported, with the n-grams, the bytes of
the packed tables, and how many of the 64 best transcripts differ from the full model's.  Prints a table and one JSON line."""
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
sys.path.insert(0, HERE)
from time_ngram_train import corpus   # noqa: E402

LABELS = "_w0123456789 "


def posteriors(sentences, B, T, peak, seed=0):
    """(B, T, C) probabilities that spell consecutive sentences: a character frame, then a blank frame; lengths all T"""
    rng = np.random.default_rng(seed)
    index = {c: i for i, c in enumerate(LABELS)}
    z = rng.standard_normal((B, T, len(LABELS))).astype(np.float32)
    at = 0
    for b in range(B):
        text = ""
        while len(text) < T // 2 and at < len(sentences):
            text += (" " if text else "") + sentences[at]
            at += 1
        text = text[:T // 2]
        text = text[:text.rfind(" ")] if " " in text else text           # end on a whole word
        path = np.zeros(T, np.int64)
        path[0:2 * len(text):2] = [index[c] for c in text]
        z[b, np.arange(T), path] += peak
    return torch.softmax(torch.from_numpy(z), -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=float, default=1e7)
    ap.add_argument("--thetas", type=float, nargs="+", default=[1e-7, 1e-6])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--peak", type=float, default=6.0)
    ap.add_argument("--width", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import ops
    from asr_amd.decoders import lm_train
    from asr_amd.decoders.lm import NgramLM
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    B, T = 64, 501
    sentences = corpus("word", int(args.tokens))
    cut = len(sentences) - len(sentences) // 10
    probs = posteriors(sentences[cut:], B, T, args.peak).to(dev)
    t0 = time.perf_counter()
    full = lm_train.estimate_ngram(sentences[:cut], order=3, mode="word", device=dev)
    say(f"word-LM decode against the model's size, {torch.cuda.get_device_name(0)}: B {B}, T {T}, width {args.width}, cutoff_top_n 38, alpha 0.8, "
        f"beta 1.0; {int(args.tokens)} words, order 3, estimated in {time.perf_counter() - t0:.1f} s; mean max probability "
        f"{float(probs.max(-1).values.mean()):.3f}; milliseconds by device events, median of {args.rounds} alternated rounds")
    space = LABELS.index(" ")
    models = []
    with tempfile.TemporaryDirectory() as d:
        for theta in [None] + list(args.thetas):
            t0 = time.perf_counter()
            est = full if theta is None else full.prune(theta, device=dev)
            lm = NgramLM(est.write_arpa(os.path.join(d, "m.arpa")), dict(enumerate(LABELS)), 0, space)
            lm.device_tables(dev)
            models.append(("full" if theta is None else f"{theta:g}", est, lm))
            say(f"  model {models[-1][0]:6s} {lm.n_ngrams:9d} n-grams, packed {lm.packed.nbytes / 1e6:8.1f} MB, written and loaded in "
                f"{time.perf_counter() - t0:.1f} s")
    decode = lambda lm: ops.ctc_beam_decode(probs, None, 0, args.width, 38, 1.0, lm, 0.8, 1.0)   # noqa: E731
    outs = {}
    for name, _, lm in models:                                           # warm-up, and the transcripts
        outs[name] = decode(lm)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in models}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.rounds):
        for name, _, lm in models[r % len(models):] + models[:r % len(models)]:   # each round starts with another model
            a.record()
            decode(lm)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    best = lambda o: [tuple(int(x) for x in row) for row in _best_labels(o)]   # noqa: E731
    ref = best(outs["full"])
    rows = []
    for name, est, lm in models:
        t = sorted(ms[name])
        differ = sum(1 for x, y in zip(best(outs[name]), ref) if x != y)
        rows.append({"model": name, "ngrams": lm.n_ngrams, "packed_bytes": int(lm.packed.nbytes), "ms": round(t[len(t) // 2], 2),
                     "spread": round(t[-1] - t[0], 2), "differ": differ})
        say(f"  decode {name:6s} {rows[-1]['ms']:9.2f} ms   spread {rows[-1]['spread']:7.2f}   best transcripts that differ from the full model's: "
            f"{differ} of {B}")
    say(json.dumps({"tokens": int(args.tokens), "width": args.width, "rounds": args.rounds, "rows": rows}))


def _best_labels(out):
    """the best hypothesis' labels per utterance from ops.ctc_beam_decode's (labels (B, K, T), offsets, lengths (B, K), scores)"""
    labels, lengths = out[0].cpu(), out[2].cpu()
    return [labels[i, 0, :int(lengths[i, 0])].tolist() for i in range(labels.shape[0])]


if __name__ == "__main__":
    main()
