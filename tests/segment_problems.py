"""Problems shared by tests/test_cpu_segment.py and tests/test_gpu_segment.py: constructed posteriors for the pause segmentation, every
one deterministic, each GPU case with the oracle's result computed once (tests/ctc_segment_oracle.py)."""
import functools
import math

import numpy as np

import det
import ctc_segment_oracle as O

SILENT, SOFT = -1, 0      # frame kinds: a silent frame (blank >= thr); a frame whose best class is the blank below every threshold (0.5);
                          # a kind k >= 1 is a frame whose best class is k (0.6), its blank between 0.05 and 0.3


def probs_from_kinds(kinds, C, thr, seed, blank=0):
    """(T, C) float32 probabilities, rows summing to 1 in float64 before the rounding.  The blank column is jittered, so that forced
    cuts have something to choose from; a class index k >= 1 counts the non-blank classes in order."""
    kinds = np.asarray(kinds, np.int64)
    T = len(kinds)
    u = det.uniform01((T,), seed).astype(np.float64)
    x = np.zeros((T, C), np.float64)
    for t, k in enumerate(kinds):
        if k == SILENT:
            pb, lab, pl = float(thr) + u[t] * (0.995 - float(thr)), None, 0.0
        elif k == SOFT:
            pb, lab, pl = 0.5, None, 0.0
        else:
            pb, lab, pl = 0.05 + 0.25 * u[t], int(k), 0.6
        others = [c for c in range(C) if c != blank]
        cls = None if lab is None else others[lab - 1]
        rest = [c for c in others if c != cls]
        x[t, rest] = (1.0 - pb - pl) / len(rest)
        x[t, blank] = pb
        if cls is not None:
            x[t, cls] = pl
    out = x.astype(np.float32)
    sil = kinds == SILENT
    assert (out[sil, blank] >= np.float32(thr)).all() and (out[~sil, blank] < np.float32(0.55)).all()
    return out


def random_kinds(T, C, seed, p_switch=0.25, same_ok=True):
    """A frame-kind sequence of alternating stretches: silent runs of 1 .. 7 frames, speech of 1 .. 24 frames (labels, soft blanks)."""
    r = det.uniform01((4 * T + 8,), seed).astype(np.float64)
    kinds, i, silent = [], 0, r[0] < 0.5
    while len(kinds) < T:
        n = 1 + int(r[i + 1] * (7 if silent else 24))
        for j in range(n):
            if silent:
                kinds.append(SILENT)
            else:
                q = r[(i + 2 + j) % len(r)]
                k = SOFT if q < 0.15 else 1 + int(q * 997) % (C - 1)
                if not same_ok and kinds and k >= 1 and kinds[-1] == k:
                    k = 1 + k % (C - 1)
                kinds.append(k)
        i = (i + n + 2) % (len(r) - 2)
        silent = not silent
    return kinds[:T]


def random_problem(n):
    """Problem n of the property tests: T in 1..199, min_gap 1..5, pad 0..3, max_len 2..39, thr in {0.55, 0.7, 0.9}, C = 5."""
    seed = det.seed_of(f"segment.random.{n}")
    T, min_gap, pad, max_len = (int(det.randint((1,), seed + k, lo, hi)[0]) for k, (lo, hi) in enumerate(((1, 200), (1, 6), (0, 4), (2, 40))))
    thr = (0.55, 0.7, 0.9)[n % 3]
    kinds = random_kinds(T, 5, seed + 9)
    return dict(x=probs_from_kinds(kinds, 5, thr, seed + 10), kinds=kinds, thr=thr, min_gap=min_gap, pad=pad, max_len=max_len)


def forced_problem(n):
    """A problem whose forced cuts meet the greedy equivalence's condition by construction: no two neighbouring frames share a
    non-blank best class, so every frame differs from the one before it or has the blank as its best class.  Long speech, short caps."""
    seed = det.seed_of(f"segment.forced.{n}")
    T = 80 + int(det.randint((1,), seed, 0, 120)[0])
    max_len = 5 + n % 9
    kinds = random_kinds(T, 5, seed + 1, same_ok=False)
    kinds = [k if k != SILENT or (t // 40) % 2 else 1 + t % 2 for t, k in enumerate(kinds)]       # 40 frames without a pause, in turns
    for t in range(1, T):
        if kinds[t] >= 1 and kinds[t] == kinds[t - 1]:
            kinds[t] = 1 + kinds[t] % 4
    thr = (0.55, 0.7, 0.9)[n % 3]
    return dict(x=probs_from_kinds(kinds, 5, thr, seed + 2), kinds=kinds, thr=thr, min_gap=1 + n % 4, pad=n % 3, max_len=max_len)


# ---- the GPU cases ---------------------------------------------------------------------------------------------------------------
MIN_GAP = 3


def _pattern(name, T, seed):
    k = [1 + t % 4 for t in range(T)]                                   # speech everywhere, no two neighbours alike
    def mute(a, b):
        for t in range(max(a, 0), min(b, T)):
            k[t] = SILENT
    if name == "all":
        mute(0, T)
    elif name == "none":
        pass
    elif name == "edges":                                               # a leading and a trailing run of one frame; runs of exactly
        mute(0, 1)                                                      # min_gap and min_gap - 1, on and off the 64-frame word seams
        mute(T - 1, T)
        mute(10, 10 + MIN_GAP)
        mute(20, 20 + MIN_GAP - 1)
        mute(62, 62 + MIN_GAP)                                          # straddles the seam at 64
        mute(126, 128)                                                  # min_gap - 1 frames that end on the seam at 128
        mute(128 + 60, 128 + 70)                                        # a long run across the seam at 192
        mute(250, 250 + MIN_GAP - 1)
    elif name == "seams":                                               # runs that begin or end exactly on a seam, and whole silent words
        mute(61, 64)
        mute(64 + 30, 64 + 33)
        mute(128, 192 + 2)
        mute(30, 32)
    elif name == "random":
        k = random_kinds(T, 5, seed)
    return k


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> dict(x (B,T,C) float32, in_lens or None, blank, thr, min_gap, pad, max_len, max_segs, is_log, want = the oracle's four
    arrays).  B = 3 ragged and C = 5 throughout."""
    cases = {}

    def add(name, x, in_lens, blank=0, thr=0.9, min_gap=MIN_GAP, pad=1, max_len=1000, max_segs=None, is_log=False):
        B, T, _ = x.shape
        if max_segs is None:
            max_segs = max(1, (T + min_gap) // (min_gap + 1) + T // ((max_len + 1) // 2))
        raw = np.float32(math.log(thr)) if is_log else np.float32(thr)
        want = O.segment_batch(x, in_lens, blank, raw, min_gap, pad, max_len, max_segs)
        cases[name] = dict(x=x, in_lens=in_lens, blank=blank, thr=thr, min_gap=min_gap, pad=pad, max_len=max_len, max_segs=max_segs,
                           is_log=is_log, want=want)

    def batch(T, names, tag, thr=0.9, blank=0):
        return np.stack([probs_from_kinds(_pattern(nm, T, det.seed_of(f"segment.gpu.{tag}.{T}.{b}")), 5, thr,
                                          det.seed_of(f"segment.gpu.x.{tag}.{T}.{b}"), blank) for b, nm in enumerate(names)])

    for T in (1, 63, 64, 65, 130, 257):
        add(f"edges.{T}", batch(T, ("edges", "all", "none"), "a"), None, pad=1)
        add(f"ragged.{T}", batch(T, ("seams", "random", "edges"), "b"), [T, (2 * T) // 3, 0], pad=2)
        add(f"random.{T}", batch(T, ("random", "random", "random"), "c"), [T - T // 5, T, T // 2], min_gap=2, pad=0, max_len=11)
    # forced cuts: a region of 3 x max_len frames with max_len = 8, and one planted tie (frames 15 and 17 share the greatest blank of the
    # first window [14, 18]: 15 wins)
    T = 65
    k = [[SILENT] * 10 + [1 + t % 4 for t in range(24)] + [SILENT] * (T - 34) for _ in range(3)]
    x = np.stack([probs_from_kinds(kb, 5, 0.9, det.seed_of(f"segment.gpu.forced.{b}")) for b, kb in enumerate(k)])
    x[0, 10:34, 0] = np.float32(0.1)
    x[0, 15, 0] = x[0, 17, 0] = np.float32(0.3)
    add("forced", x, [T, T, 30], pad=0, max_len=8)
    assert [tuple(v[0, :5]) for v in cases["forced"]["want"][:3]] == [(10, 15, 19, 23, 27), (15, 19, 23, 27, 34), (2, 3, 3, 3, 1)]
    add("forced.padded", x, [T, 34, 30], pad=3, max_len=8)
    full = int(cases["random.257"]["want"][3].max())
    add("overflow", cases["random.257"]["x"], cases["random.257"]["in_lens"], min_gap=2, pad=0, max_len=11, max_segs=full - 3)
    add("log", np.log(batch(130, ("edges", "random", "seams"), "d", thr=0.7)), [130, 101, 64], thr=0.7, is_log=True)
    add("blank2", batch(130, ("edges", "random", "seams"), "e", blank=2), [130, 130, 77], blank=2)
    return cases


# ---- the pipeline problem --------------------------------------------------------------------------------------------------------
LABELS = "_'abcdefghijklmnopqrstuvwxyz "
PIPE = dict(thr=0.9, min_gap=6, pad=2, max_len=60)
PHRASES = ["the cat", "a", "on the mat it sat and it purred all day long", "dog", "see the moon", "hello world", "we", "an apple a day",
           "go", "all good things", "zebra", "end of it"]


@functools.lru_cache(maxsize=None)
def pipeline_problem():
    """(T, 29) float32 probabilities, T about 600: a dozen phrases of mixed lengths between pauses of 6 .. 12 silent frames, two silent
    frames after every space (below min_gap: they stay inside the segment), a soft blank between doubled letters.  The third phrase is
    longer than max_len: its forced cuts land on blank frames."""
    kinds = [SILENT] * 7
    for n, ph in enumerate(PHRASES):
        prev = None
        for j, ch in enumerate(ph):
            c = LABELS.index(ch)
            if c == prev:
                kinds.append(SOFT)
            kinds += [c] * (3 + j % 2)
            if ch == " ":
                kinds += [SILENT] * 2
                c = None
            prev = c
        kinds += [SILENT] * (6 + n % 7)
    return probs_from_kinds(kinds, len(LABELS), PIPE["thr"], det.seed_of("segment.pipeline")), kinds
