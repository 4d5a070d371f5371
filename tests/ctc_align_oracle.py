"""NumPy restatement of the CTC forced-alignment contract of `ds2_ctc_align_f32` (include/ds2hip.h), written from that text — TEST
code, not shipped.  `align(e, target, dtype)` is the recurrence: with dtype=float32 it is the bit-exact twin of the kernel (a max of
fp32 values and one fp32 add per cell), with float64 it scores paths exactly.  `brute_force` enumerates every alignment of a tiny
problem and applies the global tie rule; `check_path` is the validity check of a state sequence."""
from __future__ import annotations

import itertools

import numpy as np


def state_class(s, target):
    return int(target[s >> 1]) if s & 1 else 0


def skip_allowed(s, target):
    return bool(s & 1) and s >= 3 and int(target[s >> 1]) != int(target[(s >> 1) - 1])


def infeasible(T, U):
    return dict(score=-np.inf, states=np.full(max(T, 0), -1, np.int32), tok_start=np.full(U, -1, np.int32),
                tok_end=np.full(U, -1, np.int32), tok_logp=np.full(U, -np.inf, np.float32), feasible=False)


def align(e, target, dtype=np.float32):
    """e (T_b, C) log-probabilities (any float dtype, cast to `dtype`), target a sequence of U labels.  Returns a dict: score (a `dtype`
    scalar), states (T_b) int32, tok_start / tok_end (U) int32, tok_logp (U) `dtype`, feasible."""
    e = np.asarray(e).astype(dtype)
    target = [int(c) for c in target]
    T, C = e.shape
    U = len(target)
    S = 2 * U + 1
    if T <= 0:
        out = infeasible(T, U)
        if U == 0:
            out.update(score=dtype(0), feasible=True)
        return out
    if any(c < 1 or c >= C for c in target):
        return infeasible(T, U)
    NEG = dtype(-np.inf)
    cls = np.array([state_class(s, target) for s in range(S)])
    skip = np.array([skip_allowed(s, target) for s in range(S)])
    v = np.full(S, NEG, dtype)
    v[0] = e[0, 0]
    if S > 1:
        v[1] = e[0, cls[1]]
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
            v = (m.astype(dtype) + e[t, cls]).astype(dtype)
            bp[t] = move
    end = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        end = S - 2
    score = v[end]
    if score == NEG:
        return infeasible(T, U)
    states = np.empty(T, np.int32)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    out = spans(e, states, target, dtype)
    out.update(score=score, states=states, feasible=True)
    return out


def spans(e, states, target, dtype=np.float32):
    """Token spans of a valid state sequence and the per-token emission sums in ascending t (the first emission, then one add each)."""
    e = np.asarray(e).astype(dtype)
    U = len(target)
    ts, te, lp = np.full(U, -1, np.int32), np.full(U, -1, np.int32), np.zeros(U, dtype)
    for u in range(U):
        idx = np.nonzero(np.asarray(states) == 2 * u + 1)[0]
        ts[u], te[u] = idx[0], idx[-1] + 1
        acc = e[idx[0], int(target[u])]
        for t in idx[1:]:
            acc = dtype(acc + e[t, int(target[u])])
        lp[u] = acc
    return dict(tok_start=ts, tok_end=te, tok_logp=lp)


def path_score(e, states, target, dtype=np.float64):
    """The value of a state sequence, summed in ascending t in `dtype`."""
    e = np.asarray(e).astype(dtype)
    acc = e[0, state_class(int(states[0]), target)]
    for t in range(1, len(states)):
        acc = dtype(acc + e[t, state_class(int(states[t]), target)])
    return acc


def check_path(states, target):
    """A legal alignment: starts in {0, 1}, ends in {S-2, S-1}, moves by 0, 1, or 2 (2 only into an odd state whose label differs from
    the label before it)."""
    states = [int(s) for s in states]
    S = 2 * len(target) + 1
    if not states or states[0] not in (0, 1) or states[0] >= S or states[-1] not in (S - 1, S - 2) or states[-1] < 0:
        return False
    for p, s in zip(states, states[1:]):
        d = s - p
        if d not in (0, 1, 2) or s >= S or (d == 2 and not skip_allowed(s, target)):
            return False
    return True


def brute_force(e, target, dtype=np.float64):
    """Every legal state sequence of a tiny problem; the best score and, among the sequences reaching it, the one that is
    lexicographically greatest read from the last frame backwards.  Returns (score, states) or (-inf, None)."""
    e = np.asarray(e).astype(dtype)
    T = e.shape[0]
    S = 2 * len(target) + 1
    best, best_path = -np.inf, None
    for path in itertools.product(range(S), repeat=T):
        if not check_path(path, target):
            continue
        sc = path_score(e, path, target, dtype)
        if sc == -np.inf:
            continue
        if sc > best or (sc == best and path[::-1] > best_path[::-1]):
            best, best_path = sc, path
    return best, (None if best_path is None else np.array(best_path, np.int32))


def align_batch(x, targets, tgt_off, in_lens, tgt_lens, dtype=np.float32):
    """The batched call's outputs from (B,T,C) log-probabilities: score (B), states (B,T), tok_start / tok_end / tok_logp (flat)."""
    x = np.asarray(x)
    B, T, _ = x.shape
    n = int(np.sum(tgt_lens))
    score, states = np.empty(B, dtype), np.full((B, T), -1, np.int32)
    ts, te, lp = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -np.inf, dtype)
    for b in range(B):
        Tb = T if in_lens is None else min(int(in_lens[b]), T)
        o, U = int(tgt_off[b]), int(tgt_lens[b])
        r = align(x[b, :max(Tb, 0)], targets[o:o + U], dtype)
        score[b] = r["score"]
        states[b, :max(Tb, 0)] = r["states"]
        ts[o:o + U], te[o:o + U], lp[o:o + U] = r["tok_start"], r["tok_end"], r["tok_logp"]
    return dict(score=score, states=states, tok_start=ts, tok_end=te, tok_logp=lp)
