"""Sample-rate conversion oracle: the contract of ds2_wave_resample_f32 (include/ds2hip.h) restated as the direct fp64 sum.  Written from
the contract; it does not import asr_amd.

    g = gcd(fs, ft), L = ft / g, M = fs / g, n_out = ceil(n L / M)
    output m: i0 = (m M) div L, p = (m M) mod L,  y[m] = sum_{j < P} tab[p][j] x[i0 - J + 1 + j],  x = 0 outside [0, n)
    tab[p][j] = fp32(s sinc(s tau) w(tau)),  tau = p / L + J - 1 - j,  s = rolloff min(1, L / M),  J = ceil(zeros / s),  P = 2 J
    w(tau) = I0(beta sqrt(1 - (tau s / zeros)^2)) / I0(beta) for |tau| <= zeros / s, else 0
"""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 32, 0.945, 9.0


def ratio(fs, ft, zeros=ZEROS, rolloff=ROLLOFF):
    """(L, M, s, J)."""
    g = math.gcd(int(fs), int(ft))
    L, M = int(ft) // g, int(fs) // g
    s = rolloff * min(1.0, L / M)
    return L, M, s, int(math.ceil(zeros / s))


def out_samples(n, fs, ft):
    L, M, _, _ = ratio(fs, ft)
    return -(-int(n) * L // M)


def kernel(tau, s, zeros=ZEROS, beta=BETA):
    """The continuous interpolation filter s sinc(s tau) w(tau), fp64."""
    tau = np.asarray(tau, dtype=np.float64)
    r = tau * s / zeros
    w = np.where(np.abs(r) <= 1.0, np.i0(beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / np.i0(beta), 0.0)
    return s * np.sinc(s * tau) * w


def taps(fs, ft, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA, rounded=True):
    """(L, P) table; rounded=True: fp32 values (held in fp64), what the device is handed."""
    L, M, s, J = ratio(fs, ft, zeros, rolloff)
    tau = np.arange(L, dtype=np.float64)[:, None] / L + (J - 1 - np.arange(2 * J, dtype=np.float64))[None, :]
    tab = kernel(tau, s, zeros, beta)
    return tab.astype(np.float32).astype(np.float64) if rounded else tab


def full_filter(fs, ft, rounded=True, **kw):
    """The filter on the grid of the L-times upsampled signal: h[k + J L] = h_c(k / L), k in [-J L, J L]; y[m] = sum_i h[m M - i L] x[i].
    Every entry but the last (tau = J, where the window has ended) is one entry of `taps`."""
    L, M, s, J = ratio(fs, ft, kw.get("zeros", ZEROS), kw.get("rolloff", ROLLOFF))
    tab = taps(fs, ft, rounded=rounded, **kw)
    h = np.zeros(2 * J * L + 1)
    for p in range(L):                                   # tau = p / L + J - 1 - j  <->  k = p + (J - 1 - j) L
        h[p + (J - 1 - np.arange(2 * J)) * L + J * L] = tab[p]
    return h


def resample(x, fs, ft, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """(y, A): the fp64 sum over the fp32 table and A[m] = sum_j |tab[p][j]| |x[.]|, per output sample.  fs == ft: (x, |x|)."""
    x = np.asarray(x, dtype=np.float64)
    L, M, s, J = ratio(fs, ft, zeros, rolloff)
    if L == 1 and M == 1:
        return x.copy(), np.abs(x)
    tab = taps(fs, ft, zeros, rolloff, beta)
    n, P = len(x), 2 * J
    n_out = -(-n * L // M)
    y, A = np.zeros(n_out), np.zeros(n_out)
    j = np.arange(P, dtype=np.int64)[None, :]
    for lo in range(0, n_out, 8192):
        t = np.arange(lo, min(lo + 8192, n_out), dtype=np.int64) * M
        i0, p = t // L, t % L
        idx = (i0 - J + 1)[:, None] + j
        inside = (idx >= 0) & (idx < n)
        xs = np.where(inside, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, 0.0)
        y[lo:lo + len(t)] = (tab[p] * xs).sum(axis=1)
        A[lo:lo + len(t)] = (np.abs(tab[p]) * np.abs(xs)).sum(axis=1)
    return y, A
