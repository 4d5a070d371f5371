"""Write a seeded synthetic ARPA n-gram model for timing BeamCTCDecoder's language-model arm (no toolkit needed).
Word mode: a vocabulary of random lowercase words (letters and the apostrophe of the 29-class labels); character mode: the single
characters themselves.  Every 1-gram, then random n-grams of every higher order (some starting with <s>) up to --ngrams in all,
log10 probs in [-4, -0.1] and backoffs on every order below the top.
Usage: python scripts/make_synthetic_arpa.py OUT.arpa[.gz] [--mode word|char] [--order 3] [--ngrams 200000] [--vocab 20000] [--seed 0]"""
import argparse
import gzip
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LETTERS = "abcdefghijklmnopqrstuvwxyz'"


def make(out, mode="word", order=3, ngrams=200000, vocab=20000, seed=0):
    rng = np.random.default_rng(seed)
    if mode == "word":
        words = set()
        while len(words) < vocab:
            n = int(rng.integers(1, 9))
            words.add("".join(LETTERS[i] for i in rng.integers(0, 26, size=n)))
        words = sorted(words)
    else:
        words = list(LETTERS)
    V = len(words)
    sections = [[("<s>", -99.0), ("</s>", float(rng.uniform(-2, -1)))] + [(w, float(rng.uniform(-4, -1))) for w in words]]
    left = max(0, ngrams - len(sections[0]))
    for k in range(2, order + 1):
        want = left // (order - k + 1)
        seen = set()
        tries = 0
        while len(seen) < want and tries < 50:
            idx = rng.integers(0, V, size=(want - len(seen), k))
            bos = rng.random(len(idx)) < 0.1
            for row, b in zip(idx.tolist(), bos.tolist()):
                g = ("<s>",) + tuple(words[i] for i in row[1:]) if b else tuple(words[i] for i in row)
                seen.add(" ".join(g))
            tries += 1
        left -= len(seen)
        sections.append([(g, float(p)) for g, p in zip(sorted(seen), rng.uniform(-3, -0.1, size=len(seen)))])
    op = gzip.open if out.endswith(".gz") else open
    with op(out, "wt", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, sec in enumerate(sections):
            f.write(f"ngram {k + 1}={len(sec)}\n")
        for k, sec in enumerate(sections):
            f.write(f"\n\\{k + 1}-grams:\n")
            bows = rng.uniform(-1, 0, size=len(sec)) if k + 1 < order else None
            for j, (g, p) in enumerate(sec):
                f.write(f"{p:.5f}\t{g}" + (f"\t{bows[j]:.5f}" if bows is not None else "") + "\n")
        f.write("\n\\end\\\n")
    return out, sum(len(s) for s in sections)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--mode", choices=("word", "char"), default="word")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--ngrams", type=int, default=200000)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    out, n = make(a.out, a.mode, a.order, a.ngrams, a.vocab, a.seed)
    print(f"wrote {out}: {a.mode} {a.order}-gram, {n} n-grams")


if __name__ == "__main__":
    main()
