"""Problems shared by tests/test_cpu_align_star.py and tests/test_gpu_align_star.py — TEST code.  `planted` builds the issue's planted
problem: C = 6, the transcript [*, 1, 2, 2, *, 3, 1, *] (* = the wildcard, the label value C) with both flags, penalty log 0.5; every
frame of the transcript carries p = 0.9 on its class (a blank frame between the two 2s, two between 3 and 1), every garbage frame
carries 0.9 on a random class, the rest of a frame is spread evenly (0.02 each).  Garbage: a 7-frame intro, 5 frames after the third
token, a 6-frame outro; without_ends leaves intro and outro out, and the end wildcards are then skipped.
Why the planted path is the optimum: a wildcard frame scores log 0.45 whatever the frame holds, a frame on its own class log 0.9, on
any other class log 0.02.  The garbage classes are drawn from the classes that the transcript does not use (4 and 5) — garbage on the
blank or on a neighbouring token's class would belong to that state with 0.9 against 0.45 and the planted spans would not be the
answer — so a garbage frame is worth log 0.45 on a wildcard and log 0.02 anywhere else, and a transcript frame log 0.9 in its state and
at most log 0.45 anywhere else: every other legal path loses at least log 2 in at least one frame and gains nowhere."""
import math

import numpy as np

C = 6
STAR = C
PENALTY = math.log(0.5)
TRANSCRIPT = [STAR, 1, 2, 2, STAR, 3, 1, STAR]
FLAGS = 3


def planted(without_ends=False, seed=5):
    """-> (p (T,C) float32 probabilities, want_start, want_end (8) int32 planted spans, states (T) int32)."""
    rng = np.random.default_rng(seed)
    # (state, frames): odd state 2u + 1 is token u, even states are blanks
    runs = ([] if without_ends else [(1, 7)]) + [(3, 2), (5, 3), (6, 1), (7, 2), (9, 5), (11, 2), (12, 2), (13, 3)] + \
           ([] if without_ends else [(15, 6)])
    states = np.concatenate([np.full(n, s, np.int32) for s, n in runs])
    T = len(states)
    p = np.full((T, C), 0.1 / (C - 1), np.float32)
    for t, s in enumerate(states):
        lab = TRANSCRIPT[s >> 1] if s & 1 else 0
        p[t, int(rng.integers(4, 6)) if lab == STAR else lab] = 0.9
    ts, te = np.full(len(TRANSCRIPT), -1, np.int32), np.full(len(TRANSCRIPT), -1, np.int32)
    for u in range(len(TRANSCRIPT)):
        idx = np.nonzero(states == 2 * u + 1)[0]
        if len(idx):
            ts[u], te[u] = idx[0], idx[-1] + 1
    return p, ts, te, states
