"""fp64 NumPy restatement of the minimum-error-rate loss on an n-best list (contract: include/ds2hip.h, ds2_ctc_mwer_f32) — test-only.

Per utterance b: K hypothesis slots with label sequences over the classes 1 .. C-1, a validity bit and a risk R_k.  nll_k is the plain
CTC lattice of ctc_star_loss_oracle.lattice (flag 0, no wildcard column in use), p the softmax of -nll over the finite slots, loss_b
the expected risk, w_k = p_k (R_k - loss_b) and grad = prior + grad_scale * sum_k w_k occ_k: the K softmax terms cancel."""
import numpy as np

import ctc_star_loss_oracle as S


def hyp_nll_occ(logits_b, labels, valid=True, max_hyp_len=None, want_occ=True):
    """logits_b (T_b, C) of the valid frames -> (nll, occ (T_b, C) or None) of one hypothesis; +inf / None when the slot is invalid, a
    label lies outside [1, C-1], the sequence is longer than max_hyp_len or has no alignment."""
    Tb, C = logits_b.shape
    labels = [int(v) for v in labels]
    if not valid or any(v < 1 or v >= C for v in labels) or (max_hyp_len is not None and len(labels) > max_hyp_len):
        return np.inf, None
    if Tb <= 0:
        return (0.0 if not labels else np.inf), None
    em = S.extended_emissions(logits_b, 0.0)                  # the last column is never addressed: labels < C
    alpha, beta, nl = S.lattice(em, labels, 0)
    if not np.isfinite(nl):
        return np.inf, None
    if not want_occ:
        return nl, None
    cls = S._classes(labels)
    occ = np.zeros((Tb, C))
    for s in range(cls.size):
        a = alpha[:, s] + beta[:, s]
        ok = a != S.NEG
        occ[ok, cls[s]] += np.exp(a[ok] - em[ok, cls[s]] + nl)
    return nl, occ


def posteriors(nll, risk):
    """nll, risk (K) -> (p (K), loss, w (K)) of one utterance."""
    nll = np.asarray(nll, np.float64)
    risk = np.asarray(risk, np.float64)
    fin = np.isfinite(nll)
    p = np.zeros(nll.size)
    if fin.any():
        e = np.exp(nll[fin].min() - nll[fin])
        p[fin] = e / e.sum()
    loss = float((p[fin] * risk[fin]).sum())
    w = np.zeros(nll.size)
    w[fin] = p[fin] * (risk[fin] - loss)
    return p, loss, w


def loss_and_grad(logits, hyps, valid, in_lens, risk, grad_scale=1.0, prior=None, max_hyp_len=None, want_grad=True):
    """logits (T, B, C); hyps[b][k] id lists; valid (B, K) or None; in_lens (B); risk (B, K).
    Returns (loss (B), nll_hyp (B, K), post (B, K), grad (T, B, C) or None), all fp64; prior (T, B, C) or None = zeros."""
    logits = np.asarray(logits, np.float64)
    T, B, C = logits.shape
    K = len(hyps[0])
    risk = np.asarray(risk, np.float64).reshape(B, K)
    loss, nll, post = np.zeros(B), np.full((B, K), np.inf), np.zeros((B, K))
    grad = None
    if want_grad:
        grad = np.zeros((T, B, C)) if prior is None else np.array(prior, np.float64)
    for b in range(B):
        Tb = min(int(in_lens[b]), T)
        occs = []
        for k in range(K):
            ok = True if valid is None else bool(valid[b][k])
            nll[b, k], occ = hyp_nll_occ(logits[:max(Tb, 0), b], hyps[b][k], ok, max_hyp_len, want_grad)
            occs.append(occ)
        post[b], loss[b], w = posteriors(nll[b], risk[b])
        if Tb <= 0:
            loss[b] = 0.0
            continue
        if want_grad:
            for k in range(K):
                if w[k] != 0.0 and occs[k] is not None:
                    grad[:Tb, b] += grad_scale * w[k] * occs[k]
    return loss, nll, post, grad


def edit_distance(a, b):
    """Levenshtein distance (unit costs) of two id lists."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


# Fixture A: repeated labels, an empty hypothesis, an invalid slot (whose one label is out of range too), a hypothesis that cannot
# fit its frames ([3, 3] in 2 frames), short utterances
def fixture_a():
    T, B, C, K = 12, 3, 5, 4
    logits = np.random.default_rng(7).normal(size=(T, B, C)) * 1.5
    in_lens = [12, 9, 2]
    refs = [[1, 2, 2, 3], [4, 1], [3, 3]]
    hyps = [[[1, 2, 2, 3], [1, 2, 3], [], [1, 2, 2, 3, 4, 4, 1]], [[4, 1], [4, 4, 1, 2], [2], [0]], [[3], [3, 3], [3, 4], []]]
    valid = [[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]]
    risk = np.array([[edit_distance(h, refs[b]) for h in hyps[b]] for b in range(B)], np.float64)
    return dict(T=T, B=B, C=C, K=K, logits=logits, in_lens=in_lens, refs=refs, hyps=hyps, valid=valid, risk=risk,
                loss=np.array([0.43316186, 1.69563818, 1.37284125]))
