"""NumPy restatement of the wildcard / free-ends contract of `ds2_ctc_align_star_f32` (include/ds2hip.h), written from that text — TEST
code, not shipped.  The label value C is the wildcard: an ordinary odd state that emits g[t] = max_c e[t][c] + star_penalty (the max
first, then ONE add in `dtype`).  flags bit 0: the path may also start in state 2 or 3; bit 1: it may also end in state S-3 or S-4.
`align(e, target, C, star_penalty, flags, dtype)` is the recurrence (float32: the bit-exact twin of the kernels), `brute_force`
enumerates every alignment of a tiny problem under the global tie rule, `check_path` is the validity check of a state sequence."""
from __future__ import annotations

import itertools

import numpy as np

import ctc_align_oracle as A

FREE_START, FREE_END = 1, 2


def star_row(e, star_penalty, dtype=np.float32):
    """g (T): the largest emission of every frame over all classes, blank included, plus the penalty (an fp32 argument)."""
    e = np.asarray(e).astype(dtype)
    with np.errstate(invalid="ignore"):
        return (e.max(axis=1).astype(dtype) + dtype(np.float32(star_penalty))).astype(dtype)


def extend(e, star_penalty, dtype=np.float32):
    """(T, C) emissions -> (T, C + 1): column C is the wildcard's emission, so that the label value C indexes it."""
    e = np.asarray(e).astype(dtype)
    return np.concatenate((e, star_row(e, star_penalty, dtype)[:, None]), axis=1)


def start_states(S, flags):
    return list(range(min(S, 4 if flags & FREE_START else 2)))


def end_states(S, flags):
    return [s for s in range(S - 1, S - (5 if flags & FREE_END else 3), -1) if s >= 0]


def align(e, target, C=None, star_penalty=0.0, flags=0, dtype=np.float32):
    """e (T_b, C) log-probabilities, target a sequence of U labels in [1, C] (C the wildcard).  Returns the dict of
    ctc_align_oracle.align; a token that no frame takes has tok_start = tok_end = -1 and tok_logp = 0."""
    e = np.asarray(e).astype(dtype)
    target = [int(c) for c in target]
    T = e.shape[0]
    C = e.shape[1] if C is None else int(C)
    assert e.shape[1] == C
    U = len(target)
    S = 2 * U + 1
    if T <= 0:
        out = A.infeasible(T, U)
        if U == 0:
            out.update(score=dtype(0), feasible=True)
        return out
    if any(c < 1 or c > C for c in target):
        return A.infeasible(T, U)
    ee = extend(e, star_penalty, dtype)
    NEG = dtype(-np.inf)
    cls = np.array([A.state_class(s, target) for s in range(S)])
    skip = np.array([A.skip_allowed(s, target) for s in range(S)])
    v = np.full(S, NEG, dtype)
    for s in start_states(S, flags):
        v[s] = ee[0, cls[s]]
    bp = np.zeros((T, S), np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a1 = np.concatenate(([NEG], v[:-1])).astype(dtype)
            a2 = np.where(skip, np.concatenate(([NEG, NEG], v[:-2]))[:S], NEG).astype(dtype)
            m, move = v.copy(), np.zeros(S, np.int8)
            step = a1 > m                       # strictly greater: a tie keeps the smaller move
            m, move = np.where(step, a1, m), np.where(step, 1, move)
            sk = a2 > m
            m, move = np.where(sk, a2, m), np.where(sk, 2, move)
            v = (m.astype(dtype) + ee[t, cls]).astype(dtype)
            bp[t] = move
    ends = end_states(S, flags)                 # descending: a tie goes to the larger state
    end = ends[0]
    for s in ends[1:]:
        if v[s] > v[end]:
            end = s
    score = v[end]
    if score == NEG:
        return A.infeasible(T, U)
    states = np.empty(T, np.int32)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    out = spans(ee, states, target, dtype)
    out.update(score=score, states=states, feasible=True)
    return out


def spans(ee, states, target, dtype=np.float32):
    """Token spans of a valid state sequence over the EXTENDED emissions and the per-token sums in ascending t; a skipped token gets
    (-1, -1) and 0."""
    ee = np.asarray(ee).astype(dtype)
    U = len(target)
    ts, te, lp = np.full(U, -1, np.int32), np.full(U, -1, np.int32), np.zeros(U, dtype)
    for u in range(U):
        idx = np.nonzero(np.asarray(states) == 2 * u + 1)[0]
        if len(idx) == 0:
            continue
        ts[u], te[u] = idx[0], idx[-1] + 1
        acc = ee[idx[0], int(target[u])]
        for t in idx[1:]:
            acc = dtype(acc + ee[t, int(target[u])])
        lp[u] = acc
    return dict(tok_start=ts, tok_end=te, tok_logp=lp)


def check_path(states, target, flags=0):
    """A legal alignment: starts in an allowed start state, ends in an allowed end state, moves by 0, 1 or 2 (2 only into an odd state
    whose label value differs from the one before it)."""
    states = [int(s) for s in states]
    S = 2 * len(target) + 1
    if not states or states[0] not in start_states(S, flags) or states[-1] not in end_states(S, flags):
        return False
    for p, s in zip(states, states[1:]):
        d = s - p
        if d not in (0, 1, 2) or s >= S or (d == 2 and not A.skip_allowed(s, target)):
            return False
    return True


def brute_force(ee, target, flags=0, dtype=np.float64):
    """Every legal state sequence of a tiny problem over the EXTENDED emissions (extend()); the best score and, among the sequences
    reaching it, the one that is lexicographically greatest read from the last frame backwards.  (score, states) or (-inf, None)."""
    ee = np.asarray(ee).astype(dtype)
    T = ee.shape[0]
    S = 2 * len(target) + 1
    best, best_path = -np.inf, None
    for path in itertools.product(range(S), repeat=T):
        if not check_path(path, target, flags):
            continue
        sc = A.path_score(ee, path, target, dtype)
        if sc == -np.inf:
            continue
        if sc > best or (sc == best and path[::-1] > best_path[::-1]):
            best, best_path = sc, path
    return best, (None if best_path is None else np.array(best_path, np.int32))


def align_batch(x, targets, tgt_off, in_lens, tgt_lens, star_penalty=0.0, flags=None, dtype=np.float32):
    """The batched call's outputs from (B,T,C) log-probabilities: score (B), states (B,T), tok_start / tok_end / tok_logp (flat)."""
    x = np.asarray(x)
    B, T, C = x.shape
    n = int(np.sum(tgt_lens))
    score, states = np.empty(B, dtype), np.full((B, T), -1, np.int32)
    ts, te, lp = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -np.inf, dtype)
    for b in range(B):
        Tb = T if in_lens is None else min(int(in_lens[b]), T)
        o, U = int(tgt_off[b]), int(tgt_lens[b])
        r = align(x[b, :max(Tb, 0)], targets[o:o + U], C, star_penalty, 0 if flags is None else int(flags[b]), dtype)
        score[b] = r["score"]
        states[b, :max(Tb, 0)] = r["states"]
        ts[o:o + U], te[o:o + U], lp[o:o + U] = r["tok_start"], r["tok_end"], r["tok_logp"]
    return dict(score=score, states=states, tok_start=ts, tok_end=te, tok_logp=lp)
