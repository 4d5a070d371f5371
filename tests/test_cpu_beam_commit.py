"""Commit and compaction of the streaming beam search without a GPU: the exported entries and the size query, BeamStream's new
arguments and refusals (before any device call), the host's commit and growth plan, and the oracle of tests/ctc_beam_commit_oracle.py:
compact against chain read-outs, live_nodes against a brute force, the frame-by-frame search against ctc_beam_oracle.beam_search."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_commit_oracle as CO   # noqa: E402
import ctc_beam_oracle as O           # noqa: E402
import ctc_beam_stream_oracle as SO   # noqa: E402

LABELS = "_ABCDE "
NEW = ("ds2_ctc_beam_stream_commit", "ds2_ctc_beam_stream_commit_workspace_bytes", "ds2_ctc_beam_stream_feed_committed_f32")


def _decoder(**kw):
    from asr_amd.decoders import BeamCTCDecoder
    return BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, **kw)


def _probs(T, C, seed, scale=16.0, blank_bias=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((T, C), generator=g) * scale
    z[..., 0] += blank_bias
    return torch.softmax(z, dim=-1).float().double().numpy()


def test_commit_symbols_are_exported():
    from asr_amd import _lib, ops
    from asr_amd.decoders import BeamStream, commit_capacity, commit_due
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ds2hip.h")).read()
    assert all(name + "(" in header for name in NEW)
    assert callable(ops.ctc_beam_stream_commit) and callable(ops.ctc_beam_stream_feed_committed) and callable(ops.commit_unpack)
    assert callable(commit_due) and callable(commit_capacity) and BeamStream.finish


def test_workspace_query_is_monotone_and_refuses_bad_sizes():
    from asr_amd import _lib
    lib = _lib.load()
    ws = lib.ds2_ctc_beam_stream_commit_workspace_bytes
    for bad in ((0, 10, 7), (3, 0, 7), (3, 10, 0), (-1, 10, 7), (3, 10, lib.ds2_ctc_beam_max_width() + 1), (3, 1 << 20, 7)):
        assert ws(*bad) == 0
    assert ws(3, 32, 8) == 0 and ws(1, 2621, 100) == 0           # a bitmap of up to 262144 nodes lives in LDS: no workspace
    big = ws(1, 2622, 100)
    assert big == 16 * ((2622 * 100 + 63) // 64)                 # past it: a bitmap word and a prefix slot per 64 nodes
    assert ws(2, 2622, 100) == 2 * big and ws(1, 5000, 100) > big and ws(1, 2622, 101) > big
    prev = 0
    for rows in (4096, 8192, 30000, (1 << 20) - 1):
        cur = ws(2, rows, 256)
        assert cur > prev
        prev = cur


def test_open_stream_refuses_bad_commit_arguments():
    d = _decoder(beam_width=4)
    for name in ("commit_every", "max_lag"):
        for bad in (0, -1, 2.5, "3", True):
            with pytest.raises(ValueError, match=name):
                d.open_stream(commit=True, **{name: bad})
        with pytest.raises(ValueError, match=f"{name} needs commit=True"):
            d.open_stream(**{name: 5})
    s = d.open_stream(batch=2, capacity=32, commit=True)
    assert (s.commit, s.commit_every, s.max_lag, s.commits, s.live_nodes, s.forced, s.capacity) == (True, 32, None, 0, [0, 0], [0, 0], 0)
    assert s.committed == [([], []), ([], [])]
    s = d.open_stream(commit=True, commit_every=7, max_lag=40.0)
    assert (s.commit_every, s.max_lag) == (7, 40)
    s = d.open_stream()
    assert (s.commit, s.commit_every, s.max_lag) == (False, None, None)


def test_finish_index_refusals_need_no_device():
    d = _decoder(beam_width=4)
    for commit in (False, True):
        s = d.open_stream(batch=3, commit=commit)
        for bad in (3, -1, 1.5, "0", True):
            with pytest.raises(ValueError, match="index"):
                s.finish(bad)
        s.closed = True
        with pytest.raises(ValueError, match="closed"):
            s.finish(1)


def test_stream_long_takes_the_commit_arguments():
    import inspect
    from asr_amd import DeepSpeech
    from asr_amd.decoders import BeamCTCDecoder
    p = inspect.signature(DeepSpeech.stream_long).parameters
    assert p["commit"].default is False and p["max_lag"].default is None
    p = inspect.signature(BeamCTCDecoder.open_stream).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("batch", 1), ("nbest", 1), ("capacity", 256), ("commit", False),
                                                          ("commit_every", None), ("max_lag", None)]


def test_commit_plan_is_a_pure_function():
    from asr_amd.decoders import commit_capacity, commit_due, stream_capacity
    assert not commit_due(32, 0, 20, 0, 32) and not commit_due(32, 12, 20, 31, 32)      # fits, and not yet due
    assert commit_due(32, 13, 20, 0, 32) and commit_due(32, 0, 20, 32, 32) and commit_due(32, 0, 33, 0, 32)
    assert commit_capacity(32, [7, 0], 8, 20) == (1, 32)                # seven nodes: one row, and the chunk fits
    assert commit_capacity(32, [8 * 12, 5], 8, 20) == (12, 32) and commit_capacity(32, [8 * 12 + 1, 5], 8, 20) == (13, 64)
    assert commit_capacity(1, [0], 100, 1) == (0, 1) and commit_capacity(1, [1], 100, 1) == (1, 2) and commit_capacity(1, [101], 100, 3) == (2, 8)
    for cap, nodes, K, chunk in itertools.product((1, 32, 100), ([0], [5, 900], [4096]), (1, 8, 100), (1, 20, 250)):
        rows, new = commit_capacity(cap, nodes, K, chunk)
        assert rows == max(-(-m // K) for m in nodes) and new == stream_capacity(cap, rows + chunk) and new >= cap
        assert not commit_due(new, rows, chunk, 0, 10 ** 9)             # after the plan the chunk fits


def _hand_tree():
    #  ids:      0    1    2    3    4    5    6    7
    parent = [-1,   0,   0,   1,  -1,   3,   3,   2]
    label = [1,    2,   3,   4,   5,   1,   2,   6]
    frame = [0,    2,   2,   5,   5,   7,   7,   8]
    return parent, label, frame


def test_compact_preserves_every_chain_on_hand_written_trees():
    parent, label, frame = _hand_tree()
    # beams at 5, 6 and 3 share the chain 0 -> 1 -> 3; with the stable node 1 the tree is {1, 3, 5, 6}
    p, l, f, beams, stable = CO.compact(parent, label, frame, [5, 6, 3], 1)
    assert (p, l, f, beams, stable) == ([-1, 0, 1, 1], [2, 4, 1, 2], [2, 5, 7, 7], [2, 3, 1], 0)
    for old, new in zip([5, 6, 3], beams):
        want = CO.chain(parent, label, frame, old)
        assert CO.chain(p, l, f, new) == (want[0][1:], want[1][1:])          # what lay below the stable node left; the rest is the same
    # no stable node: every chain is kept down to its first label, the dead branches (4, 7 -> 2) leave
    p, l, f, beams, stable = CO.compact(parent, label, frame, [5, 6, 3, -1], -1)
    assert len(p) == 5 and stable == -1 and beams[3] == -1
    for old, new in zip([5, 6, 3], beams):
        assert CO.chain(p, l, f, new) == CO.chain(parent, label, frame, old)
    assert all(q < i for i, q in enumerate(p))                              # parents stay below their children
    # one beam that IS the stable node
    assert CO.compact(parent, label, frame, [7], 7) == ([-1], [6], [8], [0], 0)
    assert CO.compact(parent, label, frame, [], -1) == ([], [], [], [], -1)


@pytest.mark.parametrize("seed,scale,K", [(1, 16.0, 8), (2, 4.0, 4), (3, 1.0, 5)])
def test_compact_and_live_nodes_on_the_oracles_trees(seed, scale, K):
    """At every cut of a stream the tree the frame-by-frame search has built, compacted, spells every beam from the stable pair on, and
    its size is live_nodes of the beams, which also equals a brute-force count over explicit (prefix, frame) nodes."""
    probs = _probs(60, 7, seed, scale)
    s = CO.ForcedSearch(beam_width=K)
    for t0 in range(0, 60, 5):
        s.feed(probs[t0:t0 + 5])
        beams, stable = s.beams, s.stable
        assert stable == SO.stable_prefix(beams)
        p, l, f, nodes, stable_node = s.live_tree()
        assert len(p) == CO.live_nodes(beams, stable)
        assert all(q < i for i, q in enumerate(p)) and (stable == 0) == (stable_node == -1)
        for (pr, off, _), x in zip(beams, nodes):
            lo = max(stable - 1, 0)
            assert CO.chain(p, l, f, x) == (pr[lo:], off[lo:])
        brute = set()                                                       # every node on a live chain, as (its pairs' frames and labels)
        for pr, off, _ in beams:
            for n in range(1, len(pr) + 1):
                if n >= stable:
                    brute.add((pr[:n], off[:n]))
        assert len(brute) == len(p)


def test_live_nodes_by_hand():
    beams = [((1, 2, 3), (0, 4, 6), 0.0), ((1, 2), (0, 4), 0.0), ((1, 2, 4), (0, 4, 6), 0.0), ((1, 2, 3), (0, 4, 7), 0.0)]
    assert SO.stable_prefix(beams) == 2
    assert CO.live_nodes(beams, 2) == 4          # the stable node (1,2), and three different third pairs
    assert CO.live_nodes(beams, 0) == 5 and CO.live_nodes(beams, 1) == 5
    assert CO.live_nodes([((), (), 0.0)], 0) == 0 and CO.live_nodes([], 0) == 0
    assert CO.live_nodes([((1,), (3,), 0.0), ((), (), 0.0)], 0) == 1


@pytest.mark.parametrize("seed,scale,K,top_n,cut", [(1, 16.0, 8, 40, 1.0), (2, 4.0, 4, 40, 1.0), (3, 1.0, 5, 3, 1.0), (4, 2.0, 6, 40, 0.9),
                                                    (5, 8.0, 4, 40, 1.0)])
def test_frame_by_frame_search_without_a_cut_is_beam_search(seed, scale, K, top_n, cut):
    """The restatement's beams (labels, offsets) and totals equal ctc_beam_oracle.beam_search's EXACTLY at every cut, with its margins."""
    probs = _probs(40, 7, seed, scale)
    s = CO.ForcedSearch(0, K, top_n, cut)
    for t0, n in ((0, 1), (1, 6), (7, 13), (20, 20)):
        s.feed(probs[t0:t0 + n])
        assert s.cut(-1) == 0
        want = O.beam_search(probs, t0 + n, 0, K, top_n, cut)
        got = s.result()
        assert got["beams"] == want["beams"] and got["frame_margins"] == want["frame_margins"]
        assert got["final_gaps"] == want["final_gaps"] and got["cutoff_margin"] == want["cutoff_margin"]
    again, commits = CO.run(probs, 7, None, beam_width=K, cutoff_top_n=top_n, cutoff_prob=cut)
    assert again.result()["beams"] == want["beams"] and [c[0] for c in commits] == [7, 14, 21, 28, 35]


def test_forced_cut_rule_on_the_oracle():
    """A cut at or below the stable prefix changes nothing; one above it keeps exactly the beams that share the first slot's pairs before
    the cut, in order and with their totals, and makes those pairs the stable prefix."""
    probs = _probs(60, 7, 11, 2.0)
    s = CO.ForcedSearch(beam_width=8)
    s.feed(probs[:40])
    before, stable = s.beams, s.stable
    first = before[0]
    assert stable < len(first[0]) and len(before) == 8
    low = first[1][stable - 1] + 1 if stable else 0                         # a cut that reaches no pair above the stable prefix
    assert s.cut(low) == 0 and s.beams == before and s.stable == stable
    cut = first[1][-1] + 1                                                  # a cut above every pair of the first slot
    m = len(first[0])
    dropped = s.cut(cut)
    want = [b for b in before if (b[0][:m], b[1][:m]) == (first[0], first[1])]
    assert s.beams == want and dropped == len(before) - len(want) > 0 and s.stable == m and s.forced == 1
    s.feed(probs[40:])
    for pr, off, _ in s.beams:                                              # every later beam starts with the forced text
        assert (pr[:m], off[:m]) == (first[0], first[1])
    assert SO.stable_prefix(s.beams) >= m
    forced, commits = CO.run(probs, 20, 10, beam_width=8)
    plain, _ = CO.run(probs, 20, None, beam_width=8)
    assert forced.forced >= 1 and len(commits) == 2 and forced.t == plain.t == 60
    assert CO.live_nodes(forced.beams, forced.stable) <= CO.live_nodes(plain.beams, plain.stable)


def test_seeds_of_the_forced_cut_gpu_test_are_decisive():
    """The GPU test compares with the oracle exactly where every decision cleared 1e-4 and needs 90 % of its utterances compared so: the
    oracle alone must clear that share for the seeds the test uses (test_gpu_beam_commit.FORCED)."""
    import test_gpu_beam_commit as G
    B, T, C, K, chunk, lag, every, seed, scale = G.FORCED
    probs = G._probs(B, T, C, seed, 0, scale).double().numpy()
    decisive = forced = 0
    for b in range(B):
        s, _ = CO.run(probs[b], chunk, lag, every, beam_width=K)
        res = s.result()
        decisive += O.decisive(res) and 0 in O.decisive_ranks(res)
        forced += s.forced
    assert decisive >= 0.9 * B and forced >= B, (decisive, forced)
