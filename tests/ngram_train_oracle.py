"""The n-gram estimator's contract (include/ds2hip.h, ds2_ngram_*) restated in plain fp64 Python over tuples of token strings:
interpolated modified Kneser-Ney, the listing of an ARPA file, and the lookup with ARPA backoff semantics that reads it back.
Nothing here is shared with asr_amd; the corpora the CPU and GPU tests use are made here too."""
from __future__ import annotations

import math
from collections import Counter, defaultdict

import numpy as np

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
FALLBACK = (0.5, 1.0, 1.5)


class Model:
    pass


def frame(sentences):
    """token lists -> framed token tuples, empty sentences dropped"""
    return [(BOS,) + tuple(s) + (EOS,) for s in sentences if len(s)]


def raw_counts(framed, N):
    c = [Counter() for _ in range(N + 1)]
    for f in framed:
        for n in range(1, N + 1):
            for i in range(len(f) - n + 1):
                c[n][f[i:i + n]] += 1
    return c


def estimate(sentences, N, fallback=FALLBACK):
    """sentences: lists of token strings.  -> Model with, per order n (index n, 0 unused): c, a (dicts over n-gram tuples), t (t_1..t_4),
    D (D_0..D_3), p (dict), and gamma[n] (dict over contexts of n - 1 tokens); vocab in file order, unk_p, fallback_orders."""
    m = Model()
    m.N = N
    framed = frame(sentences)
    m.n_empty = sum(1 for s in sentences if not len(s))
    m.c = raw_counts(framed, N)
    tokens = sorted({w for s in sentences for w in s})
    m.vocab = [UNK, BOS, EOS] + tokens
    pos = {w: i for i, w in enumerate(m.vocab)}
    m.sort_key = lambda g: tuple(pos[w] for w in g)
    # adjusted counts
    m.a = [None] * (N + 1)
    for n in range(1, N + 1):
        if n == N:
            a = dict(m.c[n])
        else:
            left = defaultdict(set)
            for g in m.c[n + 1]:
                left[g[1:]].add(g[0])
            a = {g: (m.c[n][g] if (n >= 2 and g[0] == BOS) else len(left[g])) for g in m.c[n]}
        if n == 1:
            a[(BOS,)] = 0
        m.a[n] = a
    # discounts
    m.t, m.D, m.fallback_orders = [None] * (N + 1), [None] * (N + 1), []
    for n in range(1, N + 1):
        t = [sum(1 for v in m.a[n].values() if v == k) for k in range(1, 5)]
        ok = all(x > 0 for x in t)
        D = [0.0, 0.0, 0.0, 0.0]
        if ok:
            Y = t[0] / (t[0] + 2.0 * t[1])
            for k in (1, 2, 3):
                D[k] = k - (k + 1) * Y * t[k] / t[k - 1]
                ok = ok and 0.0 <= D[k] <= k
        if not ok:
            D = [0.0] + [float(x) for x in fallback]
            m.fallback_orders.append(n)
        m.t[n], m.D[n] = t, D
    # context statistics and gamma
    m.S, m.gamma = [None] * (N + 1), [None] * (N + 1)
    for n in range(1, N + 1):
        S, Nk = defaultdict(int), defaultdict(lambda: [0, 0, 0, 0])
        for g, a in m.a[n].items():
            S[g[:-1]] += a
            if a > 0:
                Nk[g[:-1]][min(a, 3)] += 1
        D = m.D[n]
        m.S[n] = dict(S)
        m.gamma[n] = {h: ((D[1] * Nk[h][1] + D[2] * Nk[h][2]) + D[3] * Nk[h][3]) / S[h] for h in S if S[h] > 0}
    # probabilities
    m.V = len(tokens) + 2
    m.unk_p = m.gamma[1][()] / m.V
    m.p = [None] * (N + 1)
    for n in range(1, N + 1):
        D, p = m.D[n], {}
        for g, a in m.a[n].items():
            h = g[:-1]
            lower = m.p[n - 1][g[1:]] if n >= 2 else None
            head = (a - D[min(a, 3)]) / m.S[n][h]
            p[g] = head + (m.gamma[n][h] / m.V if n == 1 else m.gamma[n][h] * lower)
        m.p[n] = p
    return m


def log10_or_99(x):
    return math.log10(x) if x > 0 else -99.0


def listing(m):
    """the file: per order (index n - 1) a list of (tokens tuple, log10 p, log10 backoff or None) in file order; <unk> first"""
    out = []
    for n in range(1, m.N + 1):
        sec = []
        for g in sorted(m.c[n], key=m.sort_key):
            lp = -99.0 if g == (BOS,) else log10_or_99(m.p[n][g])
            bow = None
            if n < m.N and g[-1] != EOS and m.S[n + 1].get(g, 0) > 0:
                bow = log10_or_99(m.gamma[n + 1][g])
            sec.append((g, lp, bow))
        if n == 1:
            sec.insert(0, ((UNK,), log10_or_99(m.unk_p), None))
        out.append(sec)
    return out


def arpa_prob(m, h, w):
    """p(w | h) as a reader of the file computes it: the listed n-gram, else backoff(h) * p(w | h[1:]); a word outside V is <unk>"""
    h = tuple(h)[-(m.N - 1):] if m.N > 1 else ()
    while True:
        g = h + (w,)
        n = len(g)
        if g in m.p[n] and g != (BOS,):
            return m.p[n][g]
        if n == 1:
            return m.unk_p
        listed = h in m.c[n - 1] and h[-1] != EOS and m.S[n].get(h, 0) > 0
        rest = arpa_prob(m, h[1:], w)
        return (m.gamma[n][h] if listed else 1.0) * rest


def contexts(m):
    """every context whose distribution must sum to 1: the empty one, and every counted n-gram (n < N) not ending in </s>"""
    out = [()]
    for n in range(1, m.N):
        out += [g for g in m.c[n] if g[-1] != EOS]
    return out


def distribution_sum(m, h):
    """sum over V of p(w | h), every word looked up on its own"""
    return math.fsum(arpa_prob(m, h, w) for w in m.vocab if w != BOS)


def distribution_sums(m):
    """the same sum for EVERY context in time linear in the model: the words listed after h contribute their own p, every other word
    backoff(h) * p(w | h[1:]), and those add up to backoff(h) * (sum(h[1:]) - the listed words' p(w | h[1:])), all of which are listed
    one order down because a counted h w has a counted h[1:] w.  -> {context: sum}"""
    ext = defaultdict(list)
    for n in range(1, m.N + 1):
        for g in m.c[n]:
            if g != (BOS,):
                ext[g[:-1]].append(g)
    total = {(): math.fsum([m.p[1][g] for g in ext[()]] + [m.unk_p])}
    for h in sorted(contexts(m)[1:], key=len):
        n = len(h) + 1
        own = math.fsum(m.p[n][g] for g in ext[h])
        below = math.fsum(m.p[n - 1][g[1:]] for g in ext[h])
        total[h] = own + m.gamma[n][h] * (total[h[1:]] - below)
    return total


# ---- corpora ---------------------------------------------------------------------------------------------------------

def zipf_corpus(seed, n_words=2000, n_sent=3000, max_len=12):
    """the word corpus: n_words words with weights 1 / (i + 1), n_sent sentences of 0..max_len tokens"""
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(n_words) + 1.0)
    w /= w.sum()
    lens = rng.integers(0, max_len + 1, size=n_sent)
    ids = rng.choice(n_words, size=int(lens.sum()), p=w)
    out, at = [], 0
    for L in lens:
        out.append([f"w{int(i)}" for i in ids[at:at + L]])
        at += L
    return out


def char_corpus(seed, n_sent=400, max_len=40):
    """the character corpus: 26 letters, Zipf-weighted, sentences of 0..max_len characters"""
    rng = np.random.default_rng(seed)
    alphabet = [chr(ord("a") + i) for i in range(26)]
    w = 1.0 / (np.arange(len(alphabet)) + 1.0)
    w /= w.sum()
    lens = rng.integers(0, max_len + 1, size=n_sent)
    ids = rng.choice(len(alphabet), size=int(lens.sum()), p=w)
    out, at = [], 0
    for L in lens:
        out.append([alphabet[int(i)] for i in ids[at:at + L]])
        at += L
    return out


TINY = [s.split() for s in ("a b c", "a b", "b c a", "c", "a a b", "b")]   # 3 words, 6 sentences


def to_ids(sentences):
    """token lists -> (vocab in file order, flat int32 ids, int64 offsets): ids are positions in the vocabulary, tokens from 3 up"""
    tokens = sorted({w for s in sentences for w in s})
    vocab = [UNK, BOS, EOS] + tokens
    pos = {w: i for i, w in enumerate(vocab)}
    flat = np.array([pos[w] for s in sentences for w in s], dtype=np.int32)
    off = np.zeros(len(sentences) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in sentences])
    return vocab, flat, off
