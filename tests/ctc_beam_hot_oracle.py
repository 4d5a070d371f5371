"""fp64 restatement of the hotword arm of the CTC prefix beam search, `ds2_ctc_beam_decode_hot_f32` (include/ds2hip.h), written from
the contract: phrases as label-id tuples, the trie as the set of their prefixes, the longest-suffix step found by trying every suffix,
potentials rounded once to fp32, the end-of-utterance term, and `credit`, the naive scan the invariant speaks of, which knows nothing
of nodes or potentials.  `HotFusion` is a `fusion` object for `ctc_beam_lm_oracle.beam_search` (imported, unmodified); with `inner`
(a `ctc_beam_lm_oracle.Fusion`) the language-model terms are added."""
from __future__ import annotations

import math

import numpy as np

from ctc_beam_lm_oracle import NEG, beam_search, brute_force_best, decisive, decisive_ranks   # noqa: F401


class HotFusion:
    def __init__(self, phrases, weights, inner=None):
        self.phrases = [tuple(int(c) for c in p) for p in phrases]
        self.weights = [float(w) for w in weights]
        assert len(self.phrases) == len(self.weights) >= 1
        for p, w in zip(self.phrases, self.weights):
            assert len(p) >= 1 and math.isfinite(w) and w >= 0.0
        for i, p in enumerate(self.phrases):
            for j, q in enumerate(self.phrases):
                assert i == j or q[:len(p)] != p, "equal phrases, or one a prefix of another"
        self.inner = inner
        self.ends = dict(zip(self.phrases, self.weights))
        # node = a prefix of a phrase (the root is ()); phi = depth * max weight of the phrases through it, fp64, rounded once to fp32
        self.phi = {}
        for p, w in zip(self.phrases, self.weights):
            for k in range(len(p) + 1):
                self.phi[p[:k]] = max(self.phi.get(p[:k], 0.0), w)
        self.phi = {n: float(np.float32(len(n) * w)) for n, w in self.phi.items()}

    def longest(self, seq):
        """the longest suffix of seq that is a trie node"""
        for k in range(len(seq) + 1):
            if seq[k:] in self.phi:
                return seq[k:]

    def step(self, state, c):
        """-> (new state, n', term): n' the node reached, term = phi(n') - phi(state)"""
        n2 = self.longest(state + (c,))
        return (() if n2 in self.ends else n2), n2, self.phi[n2] - self.phi[state]

    def state(self, prefix):
        st = ()
        for c in prefix:
            st = self.step(st, c)[0]
        return st

    def bonus(self, prefix, c):
        t = self.step(self.state(tuple(prefix)), c)[2]
        return t + (self.inner.bonus(prefix, c) if self.inner is not None else 0.0)

    def end(self, prefix):
        return -self.phi[self.state(tuple(prefix))] + (self.inner.end(prefix) if self.inner is not None else 0.0)

    def labeling(self, lab):
        """sum of every term the search adds for a complete labeling (-inf when the inner fusion rules it out)"""
        lab = tuple(lab)
        return sum(self.bonus(lab[:k], lab[k]) for k in range(len(lab))) + self.end(lab)

    def credit(self, lab):
        """the naive scan: keep the longest suffix of the labels since the last credit that is a prefix of a phrase; when it is a
        whole phrase, credit len * w and restart.  Hotword terms only (no inner fusion)."""
        total, since = 0.0, []
        for c in lab:
            since.append(int(c))
            best = ()
            for k in range(len(since), 0, -1):   # suffix lengths, longest first
                s = tuple(since[len(since) - k:])
                if any(p[:k] == s for p in self.phrases):
                    best = s
                    break
            if best in self.ends:
                total += len(best) * self.ends[best]
                since = []
        return total
