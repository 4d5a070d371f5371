"""fp64 / integer restatement of the tempo and gain perturbation's contract (include/ds2hip.h, `ds2_tempo_gain_f32`) — TEST
INFRASTRUCTURE ONLY.  Written from the contract, not from asr_amd's code.  Parity with sox's `tempo` effect itself is unpinned.

  sizes   S, R, O = int(sr * ms / 1000 + 0.5) for 82, 14.68, 12 ms; H = S - O
  length  n_out = floor(n / f + 0.5); K = ceil(n_out / H); p_k = floor(k * f * H + 0.5) (fp64); reads of x outside [0, n) give 0
  search  s = clip(rint(x * 32768), -32768, 32767) as integers; q_0 = 0; for k >= 1, t[i] = s[q_{k-1} + H + i], i < O, and d_k in [0, R)
          minimises sum_i (s[p_k + d + i] - t[i])^2 exactly (int64), lowest d on ties; q_k = p_k + d_k
  output  segment k at y[k H ...]: O samples a + w_i (b - a), a = x[q_{k-1} + H + i], b = x[q_k + i], w_i = (i + 0.5) / O (k = 0: x[i]),
          then H - O samples x[q_k + O + j]; cut to n_out; y = clip(G y, -1, 1) with the float32 G the kernel is given
"""
import math

import numpy as np

SEGMENT_MS, SEARCH_MS, OVERLAP_MS = 82.0, 14.68, 12.0


def sizes(sr, segment_ms=SEGMENT_MS, search_ms=SEARCH_MS, overlap_ms=OVERLAP_MS):
    return tuple(int(sr * ms / 1000 + 0.5) for ms in (segment_ms, search_ms, overlap_ms))


def out_samples(n, f):
    return int(math.floor(n / f + 0.5))


def _read(a, lo, m):
    out = np.zeros(m, a.dtype)
    s, e = max(lo, 0), min(lo + m, len(a))
    if e > s:
        out[s - lo:e - lo] = a[s:e]
    return out


def tempo_gain(x, f, G=1.0, sr=16000, segment_ms=SEGMENT_MS, search_ms=SEARCH_MS, overlap_ms=OVERLAP_MS):
    """(y (n_out,) float64, d (K,) int64) of one utterance x (float32 samples), tempo factor f, linear gain G."""
    S, R, O = sizes(sr, segment_ms, search_ms, overlap_ms)
    H = S - O
    x32 = np.asarray(x, dtype=np.float32)
    n_out = out_samples(len(x32), f)
    K = -(-n_out // H)
    s = np.clip(np.rint(x32.astype(np.float64) * 32768), -32768, 32767).astype(np.int64)
    xd = x32.astype(np.float64)
    w = (np.arange(O) + 0.5) / O
    y, d, q_prev = np.zeros(K * H), np.zeros(K, np.int64), 0
    lag = np.arange(R)[:, None] + np.arange(O)[None, :]
    for k in range(K):
        q = 0
        if k > 0:
            p = int(math.floor(k * f * H + 0.5))
            ssd = ((_read(s, p, R + O)[lag] - _read(s, q_prev + H, O)[None, :]) ** 2).sum(axis=1)
            d[k] = int(np.argmin(ssd))                   # numpy's argmin returns the first (lowest) index of the minimum
            q = p + int(d[k])
            a, b = _read(xd, q_prev + H, O), _read(xd, q, O)
            y[k * H:k * H + O] = a + w * (b - a)
        else:
            y[:O] = _read(xd, 0, O)
        y[k * H + O:(k + 1) * H] = _read(xd, q + O, H - O)
        q_prev = q
    return np.clip(float(G) * y[:n_out], -1.0, 1.0), d
