"""fp64 NumPy restatement of the wildcard CTC loss (contract: include/ds2hip.h, ds2_ctc_star_loss_f32) — test-only.

A target l[0..U) over the classes 1 .. C, where the value C is the wildcard, has S = 2U + 1 states: state 2u the blank (class 0), state
2u + 1 the label l[u].  The emission matrix is the row log-softmax of the logits with one further column, the constant star_penalty.
flag bit 0: a path may start in states 0 .. 3 instead of 0 .. 1; bit 1: it may end in states S-4 .. S-1 instead of S-2 .. S-1.
The likelihood is the sum over the legal STATE paths; `brute_force_nll` enumerates them for tiny problems."""
import numpy as np

NEG = -np.inf


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def extended_emissions(logits, star_penalty):
    """logits (T, C) -> (T, C + 1) fp64: log-softmax over the C classes, then the wildcard's constant column."""
    lp = log_softmax(logits)
    return np.concatenate([lp, np.full((lp.shape[0], 1), np.float64(star_penalty))], axis=1)


def _lse(vals):
    vals = np.asarray(vals, np.float64)
    m = vals.max() if vals.size else NEG
    if m == NEG:
        return NEG
    return m + np.log(np.exp(vals - m).sum())


def _classes(labels):
    cls = np.zeros(2 * len(labels) + 1, np.int64)
    cls[1::2] = labels
    return cls


def _skip(labels, s):
    """May state s be entered from state s - 2?"""
    return s >= 2 and (s & 1) == 1 and labels[s >> 1] != labels[(s >> 1) - 1]


def _lse_rows(*rows):
    """Elementwise log-sum-exp of equally long fp64 rows; -inf where every term is -inf."""
    stack = np.stack(rows)
    m = stack.max(axis=0)
    safe = np.where(m == NEG, 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(m == NEG, NEG, safe + np.log(np.exp(stack - safe).sum(axis=0)))


def lattice(em, labels, flag=0):
    """em (T, C + 1) extended emissions of the valid frames (T >= 1), labels in [1, C].  Returns (alpha, beta, nll): alpha[t][s] the
    log-sum of the path prefixes that are in state s at frame t (emission of t included), beta the same for suffixes."""
    T = em.shape[0]
    labels = [int(v) for v in labels]
    cls = _classes(labels)
    S = cls.size
    n0, n1 = (4 if flag & 1 else 2), (4 if flag & 2 else 2)
    skip = np.array([_skip(labels, s) for s in range(S)])          # state s may be entered from s - 2
    e = em[:, cls]                                                 # (T, S)
    alpha = np.full((T, S), NEG)
    beta = np.full((T, S), NEG)
    alpha[0, :min(S, n0)] = e[0, :min(S, n0)]
    pad = np.full(2, NEG)
    for t in range(1, T):
        p = np.concatenate([pad, alpha[t - 1]])
        alpha[t] = _lse_rows(p[2:], p[1:-1], np.where(skip, p[:-2], NEG)) + e[t]
    beta[T - 1, max(S - n1, 0):] = e[T - 1, max(S - n1, 0):]
    skip_up = np.concatenate([skip, [False, False]])[2:]         # state s may move on to s + 2
    for t in range(T - 2, -1, -1):
        p = np.concatenate([beta[t + 1], pad])
        beta[t] = _lse_rows(p[:-2], p[1:-1], np.where(skip_up, p[2:], NEG)) + e[t]
    ll = _lse([alpha[T - 1, s] for s in range(max(S - n1, 0), S)])
    return alpha, beta, -ll


def loss_and_grad(logits, targets, in_lens, star_penalty, flags=None, grad_scale=1.0):
    """logits (T, B, C); targets: B id lists; in_lens (B); flags (B) or None.  Returns (nll (B) fp64, grad (T, B, C) fp64):
    grad = grad_scale * (softmax * (1 - occ_star) - occ) for t < T_b, 0 beyond and for an infeasible utterance (nll = +inf)."""
    logits = np.asarray(logits, np.float64)
    T, B, C = logits.shape
    nll = np.zeros(B)
    grad = np.zeros((T, B, C))
    for b in range(B):
        labels = [int(v) for v in targets[b]]
        Tb = min(int(in_lens[b]), T)
        flag = int(flags[b]) if flags is not None else 0
        if Tb <= 0:
            nll[b] = 0.0 if not labels else np.inf
            continue
        if any(v < 1 or v > C for v in labels):
            nll[b] = np.inf
            continue
        em = extended_emissions(logits[:Tb, b], star_penalty)
        alpha, beta, nl = lattice(em, labels, flag)
        nll[b] = nl
        if not np.isfinite(nl):
            continue
        cls = _classes(labels)
        occ = np.zeros((Tb, C + 1))
        for s in range(cls.size):
            a = alpha[:, s] + beta[:, s]
            ok = a != NEG
            occ[ok, cls[s]] += np.exp(a[ok] - em[ok, cls[s]] + nl)
        grad[:Tb, b] = grad_scale * (np.exp(em[:, :C]) * (1.0 - occ[:, C:]) - occ[:, :C])
    return nll, grad


def brute_force_nll(em, labels, flag=0):
    """-log of the sum over every legal state path, by enumeration (tiny problems only)."""
    T = em.shape[0]
    labels = [int(v) for v in labels]
    cls = _classes(labels)
    S = cls.size
    n0, n1 = (4 if flag & 1 else 2), (4 if flag & 2 else 2)
    ends = set(range(max(S - n1, 0), S))
    total = []

    def walk(t, s, score):
        score = score + em[t, cls[s]]
        if t == T - 1:
            if s in ends:
                total.append(score)
            return
        walk(t + 1, s, score)
        if s + 1 < S:
            walk(t + 1, s + 1, score)
        if s + 2 < S and _skip(labels, s + 2):
            walk(t + 1, s + 2, score)

    for s in range(min(S, n0)):
        walk(0, s, 0.0)
    return -_lse(total)
