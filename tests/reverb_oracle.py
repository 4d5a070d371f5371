"""Reverberation oracle: the contract of ds2_reverb_f32 (include/ds2hip.h), the preparation of an impulse-response bank and the draws of
asr_amd.data.draw_reverb restated in fp64.  Written from the contract; it does not import asr_amd.

    y[i] = sum_{k = 0 .. min(i, P - 1)} h[k] x[i - k],  i in [0, n)          (the tail beyond n is dropped)
    bank: d = argmax |h| (lowest index), h <- h[d:]; P = the smallest P >= 1 with sum_{k >= P} h^2 <= 10^(tail_db / 10) sum h^2, capped at
          int(max_seconds * sample_rate) and at max_taps; h <- h[:P] / sqrt(sum h[:P]^2); rounded to fp32 last.
"""
import numpy as np

MAX_TAPS = 16384


def reverb(x, h):
    """(y, A): the fp64 sum and A[i] = sum_k |h[k]| |x[i - k]|, per output sample; an empty h returns (x, |x|) (pass-through)."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n = len(x)
    if len(h) == 0:
        return x.copy(), np.abs(x)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    return np.convolve(x, h)[:n], np.convolve(np.abs(x), np.abs(h))[:n]


def reverb_direct(x, h):
    """The same sum written out tap by tap (what `reverb` is checked against)."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    y = np.zeros(len(x))
    for k in range(min(len(h), len(x))):
        y[k:] += h[k] * x[:len(x) - k]
    return y


def prepare(h, sample_rate=16000, max_seconds=0.5, tail_db=-60.0, max_taps=MAX_TAPS, rounded=True):
    """One raw response -> the prepared taps (fp64 values; rounded=True: fp32 numbers, what the device is handed)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    if h.size == 0 or not np.any(h):
        raise ValueError("all-zero impulse response")
    mag = np.abs(h)
    d = next(i for i in range(h.size) if mag[i] == mag.max())
    h = h[d:]
    total = float((h * h).sum())
    P = h.size
    for cut in range(1, h.size + 1):                     # the smallest cut whose tail is quiet enough
        if float((h[cut:] * h[cut:]).sum()) <= 10.0 ** (tail_db / 10.0) * total:
            P = cut
            break
    P = max(1, min(P, int(max_seconds * sample_rate), max_taps))
    h = h[:P] / np.sqrt((h[:P] * h[:P]).sum())
    return h.astype(np.float32).astype(np.float64) if rounded else h


def synthetic(count, sample_rate=16000, t60_range=(0.2, 0.8), drr_db_range=(-2.0, 12.0), seed=0, max_seconds=0.5, tail_db=-60.0):
    """h[0] = 1, h[k] = g N(0, 1) exp(-6.9078 k / (T60 sample_rate)), 2 T60 seconds long, g from the drawn direct-to-reverberant ratio;
    per response T60, then DRR, then the Gaussian block, from one default_rng(seed); then `prepare`.  A list of fp64 arrays."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        t60 = rng.uniform(*t60_range)
        drr_db = rng.uniform(*drr_db_range)
        n = max(int(2.0 * t60 * sample_rate), 2)
        tail = rng.standard_normal(n - 1) * np.exp(-6.9078 * np.arange(1, n) / (t60 * sample_rate))
        g = np.sqrt(10.0 ** (-drr_db / 10.0) / (tail * tail).sum())
        out.append(prepare(np.concatenate([[1.0], g * tail]), sample_rate, max_seconds, tail_db))
    return out


def draw_reverb(rng, B, starts, lengths, prob):
    """(file, base, taps): per utterance coin = rng.binomial(1, prob); if coin: file = rng.integers(len(bank))."""
    file, base, taps = [-1] * B, [0] * B, [0] * B
    for b in range(B):
        if rng.binomial(1, prob):
            i = int(rng.integers(len(lengths)))
            file[b], base[b], taps[b] = i, int(starts[i]), int(lengths[i])
    return np.array(file, np.int64), np.array(base, np.int64), np.array(taps, np.int32)
