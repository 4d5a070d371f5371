"""fp64 restatement of the language-model arm of the CTC prefix beam search, `ds2_ctc_beam_decode_lm_f32` (include/ds2hip.h), written
from the contract: a naive dict-based ARPA reader, the backoff score, the word-mode dictionary rules and the fused search.  Like
tests/ctc_beam_oracle.py it reports decision margins (`frame_margins`, `final_gaps`, `cutoff_margin`), so `decisive` and
`decisive_ranks` from there apply to its results."""
from __future__ import annotations

import gzip
import math

import numpy as np

from ctc_beam_oracle import brute_force_label_logprobs, decisive, decisive_ranks, prune   # noqa: F401

NEG = -math.inf
OOV = -1000.0
SPECIAL = ("<s>", "</s>", "<unk>")


class NaiveLM:
    """ARPA file -> {tokens tuple: (log10 prob, log10 backoff)}; vocabulary = the 1-grams"""

    def __init__(self, path):
        op = gzip.open if str(path).endswith(".gz") else open
        with op(path, "rt", encoding="utf-8") as f:
            lines = [ln.strip() for ln in f]
        self.table, self.order, n = {}, 0, 0
        for ln in lines:
            if ln.startswith("ngram ") and "=" in ln:
                self.order = max(self.order, int(ln[6:].split("=")[0]))
            elif ln.startswith("\\") and ln.endswith("-grams:"):
                n = int(ln[1:-7])
            elif ln and n and not ln.startswith("\\"):
                p = ln.split()
                self.table[tuple(p[1:n + 1])] = (float(p[0]), float(p[n + 1]) if len(p) > n + 1 else 0.0)
        self.vocab = {k[0] for k in self.table if len(k) == 1}
        self.char_mode = all(len(w) == 1 for w in self.vocab if w not in SPECIAL)

    def cond(self, h, w):
        """lm(w | h) for the context h (a tuple), by the recursive backoff rule"""
        if (*h, w) in self.table:
            return self.table[(*h, w)][0]
        return self.table.get(h, (0.0, 0.0))[1] + self.cond(h[1:], w)

    def score(self, history, w):
        """lm(w | last order-1 tokens of history, <s>-padded); OOV when a token is outside the vocabulary"""
        m = self.order - 1
        h = tuple((["<s>"] * m + list(history))[len(history):]) if m else ()
        if w not in self.vocab or any(t not in self.vocab for t in h):
            return OOV
        return self.cond(h, w)


class Fusion:
    """the LM terms of a decoder's labels: chars[i] is label i's character, `space` the space label (word mode)"""

    def __init__(self, lm, chars, blank, space, alpha, beta):
        self.lm, self.chars, self.blank, self.space, self.alpha, self.beta = lm, chars, blank, space, alpha, beta
        if not lm.char_mode:
            assert space is not None
            ok = {c for i, c in enumerate(chars) if i not in (blank, space)}
            self.dictionary = {w for w in lm.vocab if w not in SPECIAL and all(ch in ok for ch in w)}
            self.prefixes = {w[:k] for w in self.dictionary for k in range(len(w) + 1)}

    def _split(self, prefix):
        words, cur = [], ""
        for x in prefix:
            if x == self.space:
                words.append(cur)
                cur = ""
            else:
                cur += self.chars[x]
        return words, cur

    def bonus(self, prefix, c):
        """the term of the extension prefix -> prefix + (c,) (-inf when the dictionary rules it out)"""
        if self.lm.char_mode:
            return self.alpha * self.lm.score([self.chars[x] for x in prefix], self.chars[c]) + self.beta
        words, cur = self._split(prefix)
        if c == self.space:
            if cur not in self.dictionary:
                return NEG
            return self.alpha * self.lm.score(words, cur) + self.beta
        return 0.0 if cur + self.chars[c] in self.prefixes else NEG

    def end(self, prefix):
        """the end-of-utterance term"""
        if self.lm.char_mode or not prefix or prefix[-1] == self.space:
            return 0.0
        words, cur = self._split(prefix)
        return self.alpha * (self.lm.score(words, cur) if cur in self.dictionary else OOV) + self.beta

    def labeling(self, lab):
        """sum of every term the search adds for a complete labeling, or -inf when the labeling is not admissible"""
        tot = 0.0
        for k in range(len(lab)):
            tot += self.bonus(lab[:k], lab[k])
        return tot + self.end(tuple(lab))


def _order_key(prefix, total):
    return (-total, len(prefix), prefix)


def beam_search(probs, fusion, size=None, blank=0, beam_width=100, cutoff_top_n=40, cutoff_prob=1.0):
    """probs (T, C) probabilities of one utterance -> dict(beams=[(labels, offsets, total)], frame_margins, final_gaps, cutoff_margin);
    `beams` holds the survivors only"""
    probs = np.asarray(probs, dtype=np.float64)
    T, C = probs.shape
    n = T if size is None else max(0, min(int(size), T))
    K = int(beam_width)
    beams = {(): (0.0, NEG, ())}   # prefix -> (pb, pnb, offsets)
    frame_margins, cut_margin = [], math.inf
    with np.errstate(divide="ignore"):
        for t in range(n):
            kept, m = prune(probs[t], cutoff_top_n, cutoff_prob)
            cut_margin = min(cut_margin, m)
            lp = np.log(probs[t])
            acc = {}   # prefix -> [pb, pnb, offsets]

            def add(pr, pb, pnb, off):
                a = acc.setdefault(pr, [NEG, NEG, off])
                a[0], a[1] = np.logaddexp(a[0], pb), np.logaddexp(a[1], pnb)

            for pr, (pb, pnb, off) in beams.items():
                tot = np.logaddexp(pb, pnb)
                for c in kept.tolist():
                    if c == blank:
                        add(pr, tot + lp[c], NEG, off)
                    elif pr and c == pr[-1]:
                        add(pr, NEG, pnb + lp[c], off)
                        add(pr + (c,), NEG, pb + lp[c] + fusion.bonus(pr, c), off + (t,))
                    else:
                        add(pr + (c,), NEG, tot + lp[c] + fusion.bonus(pr, c), off + (t,))
            # a prefix that was a beam keeps its offsets
            cands = [(pr, a[0], a[1], float(np.logaddexp(a[0], a[1])), beams[pr][2] if pr in beams else a[2]) for pr, a in acc.items()]
            cands = [x for x in cands if x[3] > NEG]
            cands.sort(key=lambda x: _order_key(x[0], x[3]))
            frame_margins.append(cands[K - 1][3] - cands[K][3] if len(cands) > K else math.inf)
            beams = {x[0]: (x[1], x[2], x[4]) for x in cands[:K]}
            if not beams:
                break
    out = [(pr, off, float(np.logaddexp(pb, pnb)) + fusion.end(pr)) for pr, (pb, pnb, off) in beams.items()]
    out.sort(key=lambda x: _order_key(x[0], x[2]))
    gaps = [out[k][2] - out[k + 1][2] for k in range(len(out) - 1)]
    return dict(beams=out, frame_margins=frame_margins, final_gaps=gaps, cutoff_margin=cut_margin)


def brute_force_best(probs, fusion, blank=0):
    """argmax over every admissible labeling of log P(labeling) + its LM terms, ties by the contract's order -> (labels, total)"""
    best = None
    for lab, lp in brute_force_label_logprobs(probs, blank).items():
        s = lp + fusion.labeling(lab)
        if s > NEG and (best is None or _order_key(lab, s) < _order_key(*best)):
            best = (lab, s)
    return best
