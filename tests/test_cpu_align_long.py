"""CPU (-m "not gpu"): the window arithmetic of DeepSpeech.posteriors_long (asr_amd.functional.long_windows), the host side of the
tiled alignment entry (`ds2_ctc_align_tiled_f32`: its workspace query and its argument checks, which return before any launch), and
the problems of tests/test_gpu_align_long.py checked with the oracle alone."""
import numpy as np
import pytest

import align_long_problems as P
from asr_amd.functional import long_windows


@pytest.mark.parametrize("window,overlap", [(128, 16), (64, 0), (200, 98), (32, 2)])
def test_long_windows_partition_the_output_frames(window, overlap):
    hop = window - 2 * overlap
    for n in range(1, 900):
        wins = long_windows(n, window, overlap)
        pos = 0
        for i, (start, length, out_start, keep_from, keep_to) in enumerate(wins):
            own = (length - 1) // 2 + 1
            assert start == i * hop and length == min(window, n - start) and length > 0, (n, i)
            assert 0 <= keep_from < keep_to <= own, (n, i)                       # non-empty, inside the window's own output
            assert out_start == pos == start // 2 + keep_from, (n, i)            # in order, no gap and no overlap
            assert (start + window >= n) == (i == len(wins) - 1), (n, i)         # the last window is the first that reaches the end
            pos += keep_to - keep_from
        assert pos == (n - 1) // 2 + 1, n


def test_long_windows_example_and_errors():
    assert long_windows(437, 128, 16) == [(0, 128, 0, 0, 56), (96, 128, 56, 8, 56), (192, 128, 104, 8, 56), (288, 128, 152, 8, 56),
                                          (384, 53, 200, 8, 27)]
    assert long_windows(100, 128, 16) == [(0, 100, 0, 0, 50)]
    for bad in ((437, 127, 16), (437, 128, 15), (437, 32, 16), (437, 30, 16), (0, 128, 16), (-3, 128, 16)):
        with pytest.raises(ValueError):
            long_windows(*bad)


def test_ragged_problem_is_what_the_docstring_says():
    x, targets, in_lens, want = P.ragged_problem()
    assert x.shape == (6, 150, 29) and [len(t) for t in targets] == [140, 1, 0, 100, 100, 70]
    assert np.isfinite(want["score"][[0, 1, 3]]).all() and want["score"][2] == 0 and np.isneginf(want["score"][[4, 5]]).all()
    assert (want["states"][4] == -1).all() and (want["states"][5] == -1).all() and (want["states"][2] == -1).all()
    assert want["states"][1, 0] == 1
    assert want["states"][0, 0] == 0 and want["states"][0, 149] == 279 and np.isneginf(x[0]).sum() == 5
    # the forced path: first label at frame 0, last at T_b - 1, one frame per label and one blank per doubled label
    assert want["states"][3, 0] == 1 and want["states"][3, 105] == 199 and (want["states"][3, 106:] == -1).all()
    assert (np.diff(want["states"][3, :106]) >= 1).all()
    assert sum(a == b for a, b in zip(targets[3], targets[3][1:])) == 6 and targets[5][-1] == 29
    assert sum(a == b for a, b in zip(targets[0], targets[0][1:])) == 5


def test_ties_problem_is_what_the_docstring_says():
    x, targets, in_lens, want = P.ties_problem()
    assert set(np.unique(x)) == {-0.5, -0.25, 0.0} and np.isfinite(want["score"]).all()
    for b, t in enumerate(targets):
        assert len(t) == 70 and sum(a == c for a, c in zip(t, t[1:])) == 1 and t[1 + 21 * b] == t[21 * b]
        assert P.A.check_path(want["states"][b], t)
        assert not P.A.align(x[b, :70], t)["feasible"] and P.A.align(x[b, :71], t)["feasible"]


def test_beyond_problem_is_what_the_docstring_says():
    x, targets, in_lens, want = P.beyond_problem()
    assert len(targets[0]) == 3400 and (5 * (3400 + 1) + 2) * 4 > 65536          # the LDS rows that variant 2 refuses
    assert np.isfinite(want["score"]).all() and P.A.check_path(want["states"][0], targets[0])
    assert sum(a == b for a, b in zip(targets[0], targets[0][1:])) == 3


def test_soft_problem_is_what_the_docstring_says():
    p, targets, in_lens = P.soft_problem()
    assert p.shape == (4, 400, 29) and np.allclose(p.sum(-1), 1, atol=1e-5) and (p > 0).all()
    want = P.oracle(np.log(p), targets, in_lens)
    assert np.isfinite(want["score"]).all() and [len(t) for t in targets] == [150, 120, 0, 149]


def test_tiled_entry_sizes_its_workspace_and_rejects_bad_arguments_before_any_launch():
    from asr_amd import _lib
    lib = _lib.load()
    wsb = lib.ds2_ctc_align_tiled_workspace_bytes
    # back-pointers B ceil(T/8) Wp + columns B K T + carries B K P 2 + end values 2 B, in dwords
    assert wsb(6, 150, 140, 8, 64) == 4 * (6 * 19 * 141 + 6 * 3 * 150 + 6 * 3 * 64 * 2 + 12)
    assert wsb(1, 4000, 3400, 0, 0) == wsb(1, 4000, 3400, 64, 64) == 4 * (500 * 3401 + 54 * 4000 + 54 * 64 * 2 + 2)     # the defaults
    assert wsb(1, 180000, 50000, 256, 1024) == 4 * (22500 * 50001 + 49 * 180000 + 49 * 1024 * 2 + 2)        # 4.5 GB: no 32-bit size
    for tf, tp in ((12, 64), (-8, 64), (8, 100), (8, 2048), (8, -64), (8, 32)):
        assert wsb(2, 10, 3, tf, tp) == 0, (tf, tp)
    assert wsb(0, 10, 3, 0, 0) == 0 and wsb(2, 0, 3, 0, 0) == 0 and wsb(2, 10, -1, 0, 0) == 0
    p = 4096                                                           # any non-null address: every call below returns before a launch
    ok = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, targets=p, off=p, in_lens=None, lens=p, max_u=3, tf=8, tp=64, score=p,
              states=p, ts=p, te=p, lp=p, ws=p, wsb=1 << 20, stream=None)
    for bad in (dict(x=None), dict(B=0), dict(T=0), dict(C=0), dict(max_u=-1), dict(is_log=2), dict(tf=12), dict(tf=-8), dict(tp=100),
                dict(tp=2048), dict(tp=32), dict(wsb=wsb(2, 10, 3, 8, 64) - 1), dict(ws=None), dict(score=None), dict(states=None),
                dict(ts=None), dict(targets=None), dict(lens=None)):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_align_tiled_f32(*a.values()) != 0, bad
        assert b"ds2_ctc_align_tiled_f32" in lib.ds2_last_error()
