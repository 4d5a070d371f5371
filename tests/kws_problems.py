"""Problems shared by tests/test_cpu_kws.py and tests/test_gpu_kws.py: constructed posteriors for the keyword search, each with the
oracle's result computed once (tests/ctc_kws_oracle.py)."""
import functools
import math

import numpy as np

import ctc_kws_oracle as K

PEAK = 0.9


def frame_probs(C, cls, p=PEAK, rival=None, q=0.0):
    """One frame over C classes: class `cls` has probability p, class `rival` (if any) q, every other class the same share of the rest."""
    n_rest = C - 1 - (rival is not None)
    f = np.full(C, (1.0 - p - q) / n_rest, np.float64)
    f[cls] = p
    if rival is not None:
        f[rival] = q
    return f


def planted(T, C, plants):
    """(T, C) float64 probabilities: the blank has PEAK in every frame but the planted ones.  plants: [(t0, [frame spec])], a spec
    being a class (that class has PEAK) or (cls, p, rival, q)."""
    x = np.tile(frame_probs(C, 0), (T, 1))
    for t0, seq in plants:
        for i, spec in enumerate(seq):
            x[t0 + i] = frame_probs(C, spec) if isinstance(spec, int) else frame_probs(C, *spec)
    assert np.allclose(x.sum(1), 1.0) and (x > 0).all()
    return x


def thr_of(keywords, threshold):
    return np.array([len(k) * math.log(threshold) for k in keywords], np.float64).astype(np.float32)


# the dyadic tie inputs (e * 8 as integers; every row's best class is 0, so d = e and fp32 is exact)
TIE_ENTER = dict(labels=[1], e8=[[-1, 0, -2], [-3, 0, -1], [0, -2, -2]])
TIE_STAY_STEP = dict(labels=[2, 2], e8=[[0, 0, -5, 0], [-5, -3, -1, 0], [-2, 0, 0, -3], [-5, 0, -1, -1], [-3, -3, 0, -5], [-3, -4, -5, 0]],
                     t=5, winner=1, loser=2)
TIE_STEP_SKIP = dict(labels=[1, 2], e8=[[0, -4, -4, -5], [0, -1, 0, -1], [0, -2, -5, -1], [0, -1, -1, -5], [-4, -1, 0, -5], [-2, 0, -1, -1]],
                     t=4, winner=1, loser=3)


def tie_e(tie):
    return np.asarray(tie["e8"], np.float32) / np.float32(8)


KW = [3, 3, 7, 5]                                 # its plant: 3, blank, 3, 7, 5
KW_PLANT = [3, 0, 3, 7, 5]
ABSENT = [9, 4, 11]


@functools.lru_cache(maxsize=None)
def planted_three():
    """T = 120, C = 29: KW planted at 10, 50 and 90 with PEAK on every frame; ABSENT is nowhere.  Threshold 0.5."""
    p = planted(120, 29, [(10, KW_PLANT), (50, KW_PLANT), (90, KW_PLANT)])[None]
    kws = [KW, ABSENT]
    return p, kws, thr_of(kws, 0.5)


PICK_KW = [3, 7, 5]


def _pick_plant(p, q, tail):
    """PICK_KW with probability p per label against a rival (class 1) of q; tail: the last label stays one more frame at (0.45 | 0.5),
    which makes a second, weaker candidate that the accepted one kills."""
    spec = (lambda c: c) if q == 0.0 else (lambda c: (c, p, 1, q))
    return [spec(3), spec(7), spec(5)] + ([(5, 0.45, 1, 0.5)] if tail else [])


@functools.lru_cache(maxsize=None)
def planted_five():
    """T = 200, C = 29: PICK_KW planted five times, path scores about (0, -0.67, -3.76, 0, -3.76) at frames 20, 60, 100, 140, 180; the
    plants at 20 and 60 carry a weaker rival candidate one frame later."""
    plants = [(20, _pick_plant(PEAK, 0.0, True)), (60, _pick_plant(0.4, 0.5, True)), (100, _pick_plant(0.2, 0.7, False)),
              (140, _pick_plant(PEAK, 0.0, False)), (180, _pick_plant(0.2, 0.7, False))]
    return planted(200, 29, plants)[None], [PICK_KW]


def as_log32(p):
    return np.log(p).astype(np.float32)


def prob_tol(n, M):
    """The bound of the probability-input tests: a span of n frames, M the largest finite |log p| of the utterance.  The aligner test's
    bound n M (2^-22 + n 2^-24) (the hardware log2 and its ln 2 multiply per emission, one rounding per add at magnitude <= n M) with a
    factor 2 for the second logarithm, the one inside g."""
    return 2 * n * M * (2.0 ** -22 + n * 2.0 ** -24)


def batch32(x, in_lens, kws, thr, max_hits):
    return K.kws_batch(np.asarray(x, np.float32), in_lens, kws, thr, max_hits, True, np.float32)
