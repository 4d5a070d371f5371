"""The pruning and evaluation contract (include/ds2hip.h, ds2_ngram_eval / ds2_ngram_prune_*) restated in plain fp64 Python over tuples
of token strings: the listed model, its lookup with ARPA backoff, the entropy values of Stolcke 1998, the count cut, the closure and the
renormalisation.  Sums are math.fsum.  It builds on ngram_train_oracle (estimate, and the same corpora); nothing is shared with asr_amd."""
from __future__ import annotations

import math
from collections import defaultdict

import ngram_train_oracle as O
from ngram_train_oracle import BOS, EOS, UNK


class Listed:
    """A model as a file lists it.  N; p[n]: {n-gram: p}; bow[n]: {n-gram: backoff} where one is listed; vocab in file order."""


def from_estimate(m):
    """the model that ngram_train_oracle.listing(m) writes, with the probabilities before they are rounded to logarithms"""
    L = Listed()
    L.N, L.vocab = m.N, list(m.vocab)
    L.p, L.bow = [None] + [dict() for _ in range(m.N)], [None] + [dict() for _ in range(m.N)]
    L.p[1][(UNK,)] = m.unk_p
    for n in range(1, m.N + 1):
        for g in m.c[n]:
            L.p[n][g] = 1e-99 if g == (BOS,) else m.p[n][g]
            if n < m.N and g[-1] != EOS and m.S[n + 1].get(g, 0) > 0:
                L.bow[n][g] = m.gamma[n + 1][g] if m.gamma[n + 1][g] > 0 else 1e-99
    return L


def prob(L, h, w):
    """(p_M(w | h), the order of the n-gram that was listed); (None, 0) when w is not even a 1-gram"""
    h = tuple(h)
    h = h[len(h) - (L.N - 1):] if len(h) > L.N - 1 else h
    scale = 1.0
    while True:
        g = h + (w,)
        if g in L.p[len(g)]:
            return scale * L.p[len(g)][g], len(g)
        if not h:
            return None, 0
        scale *= L.bow[len(h)].get(h, 1.0)
        h = h[1:]


def children(L):
    """{context: [its listed children]} over the n-grams of order >= 2"""
    ext = defaultdict(list)
    for n in range(2, L.N + 1):
        for g in L.p[n]:
            ext[g[:-1]].append(g)
    return ext


def history(L, h):
    """P(h) = prod_i p_M(h_i | h_1 .. h_{i-1}); a leading <s> is scored as p_M(</s>)"""
    out = 1.0
    for i, w in enumerate(h):
        out *= prob(L, h[:i], EOS if (i == 0 and w == BOS) else w)[0]
    return out


def values(L):
    """{n-gram of order >= 2: exp(dH) - 1 of removing it alone}, and {context: (num, den)}"""
    val, nd = {}, {}
    for h, kids in children(L).items():
        ps = [L.p[len(g)][g] for g in kids]
        qs = [prob(L, h[1:], g[-1])[0] for g in kids]
        num, den = 1.0 - math.fsum(ps), 1.0 - math.fsum(qs)
        nd[h] = (num, den)
        alpha, Ph = L.bow[len(h)].get(h, 1.0), history(L, h)
        for g, p, q in zip(kids, ps, qs):
            la = math.log((num + p) / (den + q))
            dH = -Ph * (p * (math.log(q) + la - math.log(p)) + num * (la - math.log(alpha)))
            val[g] = math.expm1(dH)
    return val, nd


def cut(L, marked):
    """closure and renormalisation for a set of marked n-grams -> the new Listed model (or L itself when nothing leaves), which also has
    nd[context] = (num', den') of every recomputed backoff"""
    marked = set(marked)
    assert all(len(g) >= 2 for g in marked)
    for n in range(L.N - 1, 1, -1):                                   # a marked n-gram that is the context of a kept (n+1)-gram is kept
        marked -= {g[:-1] for g in L.p[n + 1] if g not in marked}
    if not marked:
        return L
    M = Listed()
    M.vocab = L.vocab
    kept = [None] + [{g: p for g, p in L.p[n].items() if g not in marked} for n in range(1, L.N + 1)]
    M.N = max(n for n in range(1, L.N + 1) if kept[n])
    M.p, M.bow, M.nd = kept[:M.N + 1], [None] + [dict() for _ in range(M.N)], {}
    ext = children(M)
    for n in range(1, M.N):                                            # bottom up: den' reads the model already finished below
        for h in M.p[n]:
            kids = ext.get(h)
            if not kids:
                continue
            num = 1.0 - math.fsum(M.p[n + 1][g] for g in kids)
            den = 1.0 - math.fsum(prob(M, h[1:], g[-1])[0] for g in kids)
            M.nd[h] = (num, den)
            M.bow[n][h] = num / den if num / den > 0 else 1e-99
    return M


def prune(L, threshold=None, min_count=None, counts=None):
    """the two modes in the contract's order -> the new model; counts[n]: {n-gram: raw count} (ngram_train_oracle's m.c)"""
    if min_count is not None:
        L = cut(L, {g for n in range(2, L.N + 1) for g in L.p[n] if counts[n][g] < min_count[n - 1]})
    if threshold is not None:
        val, _ = values(L)
        L = cut(L, {g for g, v in val.items() if v < threshold})
    return L


def distribution_sum(L, h):
    """sum over the vocabulary (without <s>) of p(w | h), every word looked up on its own"""
    return math.fsum(prob(L, h, w)[0] for w in L.vocab if w != BOS)


def score(L, sentences):
    """the scored positions of sentences (token lists; empty ones included): [(p or None, order)] in sentence order, </s> included; a
    token outside the vocabulary is <unk>"""
    known, out = set(L.vocab), []
    for s in sentences:
        f = [BOS] + [w if (w in known and w not in (BOS, EOS)) else UNK for w in s] + [EOS]
        out += [prob(L, f[max(0, i - (L.N - 1)):i], f[i]) for i in range(1, len(f))]
    return out


__all__ = ["O", "Listed", "from_estimate", "prob", "values", "cut", "prune", "distribution_sum", "score", "history", "children"]
