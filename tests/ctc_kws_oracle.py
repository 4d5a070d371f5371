"""NumPy restatement of the keyword-search contract of `ds2_ctc_kws_f32` (include/ds2hip.h), written from that text — TEST ORACLE, not the
product.  With float32 emissions every operation is the contract's single fp32 operation (one subtract for d, the max over the moves,
one add), so the per-frame arrays and the pick are pinned bit for bit; with float64 emissions the same code is the reference of the
probability-input tests."""
import numpy as np

NEG = -np.inf


def kws_lattice(e, labels):
    """e (T_b, C) log emissions (float32 or float64), labels: the keyword -> (v, s), each (T_b, 2U): the value and the start frame of
    every state in every frame (column 0, the state that does not exist, stays (-inf, -1)).  None for a keyword without a lattice
    (U = 0 or a label outside [1, C))."""
    e = np.asarray(e)
    dt = e.dtype.type
    Tb, C = e.shape
    U = len(labels)
    if U == 0 or any(not (1 <= int(c) < C) for c in labels):
        return None
    lab = np.asarray(labels, np.int64)
    S = 2 * U
    q = np.arange(S)
    cls = np.where(q & 1, lab[q >> 1], 0)
    can_step = q >= 2
    can_skip = np.zeros(S, bool)
    for u in range(1, U):
        can_skip[2 * u + 1] = lab[u] != lab[u - 1]
    g = e.max(axis=1) + dt(0) if Tb else np.zeros(0, e.dtype)
    with np.errstate(invalid="ignore"):
        d = e - g[:, None]                                   # ONE subtract
    d[e == NEG] = NEG
    v = np.full(S, NEG, e.dtype)
    s = np.full(S, -1, np.int64)
    V, St = np.full((Tb, S), NEG, e.dtype), np.full((Tb, S), -1, np.int64)
    for t in range(Tb):
        best, bs = v.copy(), s.copy()                        # stay
        step_v, step_s = np.full(S, NEG, e.dtype), np.full(S, -1, np.int64)
        step_v[1:], step_s[1:] = v[:-1], s[:-1]
        take = can_step & (step_v > best)                    # a strict >: the smaller move keeps a tie
        best, bs = np.where(take, step_v, best), np.where(take, step_s, bs)
        skip_v, skip_s = np.full(S, NEG, e.dtype), np.full(S, -1, np.int64)
        skip_v[2:], skip_s[2:] = v[:-2], s[:-2]
        take = can_skip & (skip_v > best)
        best, bs = np.where(take, skip_v, best), np.where(take, skip_s, bs)
        if dt(0) > best[1]:                                  # enter: state 1 only, loses every tie
            best[1], bs[1] = dt(0), t
        v = (best + d[t, cls]).astype(e.dtype)               # ONE add
        v[0] = NEG
        s = np.where(v == NEG, -1, bs)
        V[t], St[t] = v, s
    return V, St


def kws_frames(e, labels, T=None):
    """The per-frame outputs of one (utterance, keyword): (frame_score (T), frame_start (T) int32), (-inf, -1) for t >= T_b."""
    e = np.asarray(e)
    Tb = e.shape[0]
    T = Tb if T is None else T
    score, start = np.full(T, NEG, e.dtype), np.full(T, -1, np.int32)
    lat = kws_lattice(e, labels)
    if lat is not None:
        score[:Tb], start[:Tb] = lat[0][:, -1], lat[1][:, -1]
    return score, start


def kws_pick(score, start, thr, max_hits):
    """Greedy non-maximum suppression on one (utterance, keyword) -> (hit_start, hit_end (max_hits) int32, hit_score (max_hits), n_hits)."""
    score = np.asarray(score)
    hs, he = np.full(max_hits, -1, np.int32), np.full(max_hits, -1, np.int32)
    hv = np.full(max_hits, NEG, score.dtype)
    live = [t for t in range(len(score)) if np.isfinite(score[t]) and score[t] >= thr]
    n = 0
    while live:
        if n == max_hits:
            n = max_hits + 1
            break
        t = max(live, key=lambda i: (score[i], -i))          # the largest score, a tie to the smallest t
        hs[n], he[n], hv[n] = start[t], t + 1, score[t]
        n += 1
        live = [i for i in live if not (start[i] <= t and start[t] <= i)]
    return hs, he, hv, n


def kws_batch(x, in_lens, keywords, thr, max_hits, is_log=True, dtype=np.float32):
    """The whole entry: x (B,T,C), in_lens (B) or None, keywords a list of label lists, thr (K) -> the six outputs.  is_log=False: the
    emissions are log(x) taken in `dtype` (float64 for the probability-input tests)."""
    x = np.asarray(x)
    B, T, _ = x.shape
    K = len(keywords)
    fs, fst = np.full((B, K, T), NEG, dtype), np.full((B, K, T), -1, np.int32)
    hs, he = np.full((B, K, max_hits), -1, np.int32), np.full((B, K, max_hits), -1, np.int32)
    hv, nh = np.full((B, K, max_hits), NEG, dtype), np.zeros((B, K), np.int32)
    for b in range(B):
        Tb = T if in_lens is None else max(min(int(in_lens[b]), T), 0)
        xb = x[b, :Tb].astype(dtype)
        with np.errstate(divide="ignore"):
            e = xb if is_log else np.log(xb)
        for k, kw in enumerate(keywords):
            fs[b, k], fst[b, k] = kws_frames(e, kw, T)
            hs[b, k], he[b, k], hv[b, k], nh[b, k] = kws_pick(fs[b, k], fst[b, k], dtype(thr[k]) if dtype is np.float32 else thr[k], max_hits)
    return fs, fst, hs, he, hv, nh
