"""fp64 restatement of the word / character confidences (ds2_ctc_conf_f32, contract in include/ds2hip.h), and the fixtures its tests
share.  For a hypothesis y and a unit (labels [lo, hi), frames [ts, te)): the probability that the whole utterance spells y, given that
the frames outside the window spell the rest of y.  The lattices are ctc_star_loss_oracle.lattice (the plain loss: no wildcard, no
flags); what is added is the masked backward sweep beta' and the three log-sums num, A and Bq."""
import itertools

import numpy as np

import ctc_star_loss_oracle as S

NEG = -np.inf
MAX_UNIT_LABELS = 63


def unit_terms(em, labels, lo, hi, ts, te, lat=None):
    """em (T_b, C + 1) extended emissions of the valid frames, labels valid, the unit within its bounds.  Returns (num, A, Bq)."""
    labels = [int(v) for v in labels]
    Tb, U = em.shape[0], len(labels)
    Sn = 2 * U + 1
    alpha, beta, _ = lat if lat is not None else S.lattice(em, labels)
    cls = S._classes(labels)
    e = em[:, cls]
    skip = np.array([S._skip(labels, s) for s in range(Sn)])
    skip_up = np.concatenate([skip, [False, False]])[2:]           # state s may move on to s + 2
    pad = np.full(2, NEG)
    if te < Tb:
        bp = np.full(Sn, NEG)
        bp[2 * hi] = beta[te, 2 * hi]
        if 2 * hi + 1 < Sn:
            bp[2 * hi + 1] = beta[te, 2 * hi + 1]
        Bq = S._lse([beta[te, 2 * hi], beta[te, 2 * hi + 1] if 2 * hi + 1 < Sn else NEG])
        first = te - 1
    else:
        bp = beta[Tb - 1].copy()
        Bq = 0.0 if hi == U else NEG
        first = Tb - 2
    for t in range(first, ts - 1, -1):
        p = np.concatenate([bp, pad])
        bp = S._lse_rows(p[:-2], p[1:-1], np.where(skip_up, p[2:], NEG)) + e[t]
    if ts == 0:
        A = 0.0 if lo == 0 else NEG
        num = S._lse([bp[0], bp[1] if Sn > 1 else NEG])
    else:
        terms, ctx = [], []
        for s in (2 * lo - 1, 2 * lo):
            if s < 0:
                continue
            moves = [bp[s], bp[s + 1] if s + 1 < Sn else NEG, bp[s + 2] if skip_up[s] else NEG]
            with np.errstate(invalid="ignore"):
                terms.append(alpha[ts - 1, s] + S._lse(moves))
            ctx.append(alpha[ts - 1, s])
        num, A = S._lse(terms), S._lse(ctx)
    return num, A, Bq


def unit_logconf(num, A, Bq):
    if A == NEG or Bq == NEG:
        return np.nan
    if num == NEG:
        return NEG
    return min(0.0, num - (A + Bq))


def confidence(logits, hyps, in_lens, units, w_max=None, n_units=None, max_hyp_len=None):
    """logits (T, B, C); hyps: B id lists; in_lens (B); units: per utterance a list of (lo, hi, ts, te).  n_units overrides the counts
    (the refusal of a count outside [0, W_max]).  Returns (nll (B), logconf (B, W_max), mag (B, W_max)): mag is the largest magnitude
    among the finite num, A and Bq of a unit with a finite result (0 elsewhere), what the fp32 bar scales with."""
    logits = np.asarray(logits, np.float64)
    T, B, C = logits.shape
    W = max([len(u) for u in units] + [1]) if w_max is None else w_max
    nll = np.full(B, np.inf)
    out = np.full((B, W), np.nan)
    mag = np.zeros((B, W))
    for b in range(B):
        Tb, y = min(int(in_lens[b]), T), [int(v) for v in hyps[b]]
        U = len(y)
        good = all(1 <= v < C for v in y) and (max_hyp_len is None or U <= max_hyp_len)
        lat = None
        if good and Tb > 0:
            em = S.extended_emissions(logits[:Tb, b], 0.0)
            lat = S.lattice(em, y)
            nll[b] = lat[2]
        elif good and U == 0:
            nll[b] = 0.0
        nu = len(units[b]) if n_units is None else int(n_units[b])
        if lat is None or nu < 0 or nu > W:
            continue
        for w, (lo, hi, ts, te) in enumerate(units[b][:nu]):
            if not (0 <= lo < hi <= U and hi - lo <= MAX_UNIT_LABELS and 0 <= ts < te <= Tb):
                continue
            num, A, Bq = unit_terms(em, y, lo, hi, ts, te, lat)
            out[b, w] = unit_logconf(num, A, Bq)
            if np.isfinite(out[b, w]):
                mag[b, w] = max(abs(num), abs(A), abs(Bq))
    return nll, out, mag


def collapse(path):
    return [int(k) for k, _ in itertools.groupby(path) if k != 0]


def brute_force(lp, labels, lo, hi, ts, te):
    """lp (T, C) log-probabilities of a tiny problem.  By enumeration of all C^T frame labelings:
    P(the whole spells y, the frames before ts spell y[:lo] and the frames from te on spell y[hi:]) / P(the last two).  Returns
    (log joint, log context): -inf where the probability is 0."""
    T, C = lp.shape
    y = [int(v) for v in labels]
    joint, ctx = 0.0, 0.0
    for path in itertools.product(range(C), repeat=T):
        if collapse(path[:ts]) != y[:lo] or collapse(path[te:]) != y[hi:]:
            continue
        p = np.exp(sum(lp[t, c] for t, c in enumerate(path)))
        ctx += p
        if collapse(path) == y:
            joint += p
    with np.errstate(divide="ignore"):
        return np.log(joint), np.log(ctx)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def planted():
    """frames a a _ ' ' (a|b at 0.5) (a|b at 0.5) _ ; hypothesis "a a": word 1 in [0, 2) is certain, word 2 in [4, 6) is 0.25.
    Classes: 0 blank, 1 a, 2 b, 3 space.  Returns (probs (T, C), hypothesis ids, units, expected confidences)."""
    p = np.zeros((7, 4))
    p[0, 1] = p[1, 1] = p[2, 0] = p[3, 3] = p[6, 0] = 1.0
    p[4, 1] = p[4, 2] = p[5, 1] = p[5, 2] = 0.5
    return p, [1, 3, 1], [(0, 1, 0, 2), (2, 3, 4, 6)], [1.0, 0.25]


def fixture_a():
    """T = 12, B = 3, C = 5, in_lens [12, 7, 1], logits beyond in_lens NaN.  Utterance 0: a repeated label across unit boundaries,
    units at ts = 0 and te = T_b, one-frame windows, lo = 0 / hi = U, the whole hypothesis, overlaps, every kind of invalid unit, an
    impossible context, slots beyond n_units.  Utterance 1: infeasible (one label five times needs 9 frames of 7).  Utterance 2:
    the empty hypothesis on one frame."""
    rng = np.random.default_rng(20)
    T, B, C = 12, 3, 5
    in_lens = [12, 7, 1]
    logits = rng.normal(size=(T, B, C)) * 2.0
    for b, n in enumerate(in_lens):
        logits[n:, b] = np.nan
    hyps = [[1, 2, 2, 3, 1], [4, 4, 4, 4, 4], []]
    units = [
        [(0, 1, 0, 3), (1, 2, 3, 5), (2, 3, 5, 7), (3, 5, 7, 12),   # a tiling: ts = 0, the repeated label on both sides of a boundary, te = T_b
         (2, 3, 5, 6), (4, 5, 11, 12), (0, 1, 0, 1),                 # windows of one frame
         (0, 5, 0, 12), (0, 5, 2, 9), (0, 3, 0, 8), (2, 5, 4, 12),   # the whole hypothesis; lo = 0 and hi = U; overlapping units
         (1, 4, 2, 10), (1, 3, 3, 4),                                # (the second: "2 2" needs three frames, its window has one: -inf)
         (1, 2, 0, 4), (1, 3, 6, 12),                                # impossible contexts: ts = 0 with lo > 0, te = T_b with hi < U
         (-1, 2, 0, 4), (2, 2, 0, 4), (3, 2, 0, 4), (0, 6, 0, 4),    # label ranges: below 0, empty, reversed, beyond U
         (0, 2, -1, 4), (0, 2, 4, 4), (0, 2, 5, 4), (0, 2, 4, 13)],  # windows: below 0, empty, reversed, beyond T_b
        [(0, 1, 0, 2), (0, 5, 0, 7), (1, 2, 2, 4)],
        [(0, 1, 0, 1)],
    ]
    return dict(T=T, B=B, C=C, in_lens=in_lens, logits=logits, hyps=hyps, units=units, w_max=25, max_hyp_len=5)


def fixture_b():
    """T = 70, B = 2, C = 6: a 64-label hypothesis (129 states: the workgroup lattice), a unit of 63 labels and one of 64."""
    rng = np.random.default_rng(21)
    T, B, C = 70, 2, 6
    logits = rng.normal(size=(T, B, C))
    y = [1 + u % (C - 1) for u in range(64)]
    y[30] = y[29]                                                     # one repeated label: 65 of the 70 frames are needed
    for u in range(64):                                               # bias the frames towards the hypothesis: the result stays finite
        logits[u + 3, 0, y[u]] += 6.0
    logits[:3, 0, 0] += 6.0
    logits[67:, 0, 0] += 6.0
    hyps = [y, [2, 3]]
    units = [[(0, 63, 0, 66), (1, 64, 4, 70), (0, 64, 0, 70), (10, 20, 13, 23), (63, 64, 66, 70)], [(0, 1, 0, 30), (1, 2, 30, 70)]]
    return dict(T=T, B=B, C=C, in_lens=[70, 70], logits=logits, hyps=hyps, units=units, w_max=5, max_hyp_len=64)
