"""The problems of tests/test_cpu_align_long.py (which checks with the oracle that they are what their docstrings say) and
tests/test_gpu_align_long.py (which runs the tiled lattice, `ds2_ctc_align_tiled_f32`, on them) — TEST code, not shipped.  Data come
from `det`; every oracle result is computed once and shared."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import det  # noqa: E402

import ctc_align_oracle as A  # noqa: E402


def log_softmax64(shape, seed, scale=4.0):
    z = det.uniform01(shape, seed).astype(np.float64) * scale
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def pack(targets):
    lens = np.array([len(t) for t in targets], np.int32)
    off = np.zeros(len(targets), np.int32)
    off[1:] = np.cumsum(lens)[:-1]
    flat = np.array([c for t in targets for c in t], np.int32)
    return flat, off, lens


def cyc(n, C, start=0, doubled=()):
    """n labels cycling through 1..C-1 (no adjacent repeat), then label i made equal to label i-1 for i in `doubled`."""
    lab = [1 + (start + i) % (C - 1) for i in range(n)]
    for i in doubled:
        lab[i] = lab[i - 1]
    return lab


def oracle(x, targets, in_lens):
    flat, off, lens = pack(targets)
    return A.align_batch(x, flat, off, in_lens, lens)


@functools.lru_cache(maxsize=None)
def ragged_problem():
    """B = 6, T = 150, C = 29, log-probabilities.  Under tiles of 8 frames x 64 pairs utterance 0 (U = 140, labels doubled at 4, 63, 64,
    127 and 139, T_b = 150: 145 frames needed) spans three pair tiles, the last with 13 pairs, and 19 frame blocks, the last partial,
    and has -inf emissions where it keeps slack; 1: U = 1, T_b = 1; 2: U = 0, T_b = 0; 3: U = 100 with six doubled labels at exactly the
    minimal T_b = 106 (the forced path crosses tile corners with -inf everywhere else); 4: U = 100, T_b = 99 (infeasible by length);
    5: U = 70 with its last label equal to C (a bad label), T_b = 150.  Finite scores for 0, 1 and 3, score 0 for 2, -inf for 4, 5."""
    T, C = 150, 29
    bad = cyc(70, C, 11)
    bad[-1] = C
    targets = [cyc(140, C, 3, doubled=(4, 63, 64, 127, 139)), [5], [], cyc(100, C, 1, doubled=(3, 31, 32, 64, 90, 99)), cyc(100, C, 7), bad]
    in_lens = [150, 1, 0, 106, 99, 150]
    x = log_softmax64((6, T, C), det.seed_of("align_long.ragged")).astype(np.float32)
    # -inf entries that leave utterance 0 feasible (5 frames of slack): its first label in frame 0 (the path starts in the blank), a blank
    # in the frames 5, 80 and 149 (a label is held there), and its doubled label 64 in frame 70
    x[0, 0, targets[0][0]] = x[0, 5, 0] = x[0, 80, 0] = x[0, 149, 0] = x[0, 70, targets[0][64]] = -np.inf
    unused = [c for c in range(1, C) if c not in targets[3]]
    if unused:
        x[3, :, unused[0]] = -np.inf
    x[1, 0, 0] = -np.inf
    return x, targets, in_lens, oracle(x, targets, in_lens)


@functools.lru_cache(maxsize=None)
def ties_problem():
    """B = 4, T = 96, C = 4, U = 70 with one doubled label at a different place per utterance (71 frames needed): emissions are
    -0.25 * {0, 1, 2}, so every sum is exact and ties are everywhere, across every seam of tiles of 8 frames x 64 pairs."""
    B, T, C, U = 4, 96, 4, 70
    x = (-0.25 * det.randint((B, T, C), det.seed_of("align_long.ties"), 0, 3)).astype(np.float32)
    targets = [cyc(U, C, b, doubled=(1 + 21 * b,)) for b in range(B)]
    return x, targets, [T] * B, oracle(x, targets, None)


@functools.lru_cache(maxsize=None)
def beyond_problem():
    """B = 1, T = 4000, C = 5, U = 3400 with doubled labels at 100, 2000 and 3399 (3403 frames needed): feasible, and beyond the
    3 275 labels at which variant 2 of ds2_ctc_align_f32 refuses the target."""
    T, C = 4000, 5
    targets = [cyc(3400, C, 0, doubled=(100, 2000, 3399))]
    x = log_softmax64((1, T, C), det.seed_of("align_long.beyond"), scale=2.0).astype(np.float32)
    return x, targets, [T], oracle(x, targets, [T])


@functools.lru_cache(maxsize=None)
def soft_problem():
    """B = 4, T = 400, C = 29, PROBABILITIES (softmax of 6 * uniform): U = 150 with two doubled labels at T_b = 400, U = 120 at T_b = 390,
    U = 0 at T_b = 17, U = 149 at T_b = 400; every utterance is feasible."""
    B, T, C = 4, 400, 29
    p = np.exp(log_softmax64((B, T, C), det.seed_of("align_long.soft"), scale=6.0)).astype(np.float32)
    targets = [cyc(150, C, 2, doubled=(63, 128)), cyc(120, C, 9), [], cyc(149, C, 17, doubled=(1,))]
    return p, targets, [400, 390, 17, 400]
