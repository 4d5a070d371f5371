"""CPU: the streaming keyword-search contract (include/ds2hip.h, ds2_ctc_kws_stream_feed_f32) as tests/ctc_kws_stream_oracle.py restates
it — the prefix property against the one-call pick of tests/ctc_kws_oracle.py for cuts at every frame, at random places and not at all,
ties included; what a forced cut keeps — and the host half: the exported entries, the size of the state, and every refusal of the
entry, of the ops and of KeywordSpotter.open_stream / KeywordStream.feed that needs no GPU."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import det
import ctc_kws_oracle as K
import ctc_kws_stream_oracle as S
import kws_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = "_'abcdefghijklmnopqrstuvwxyz "
MAX_HITS = 64


@functools.lru_cache(maxsize=None)
def random_problems():
    """60 problems, T in 1..90, C in 3..5, U in 1..4, every third with emissions rounded to integers so that scores tie; the threshold a
    quantile of the problem's own finite frame scores -> [(e, labels, thr, frame_score, frame_start)]"""
    rng = np.random.default_rng(det.seed_of("kws.stream.rule") % (1 << 32))
    out = []
    for i in range(60):
        T, C, U = int(rng.integers(1, 91)), int(rng.integers(3, 6)), int(rng.integers(1, 5))
        z = rng.random((T, C)) * 4
        e = z - np.log(np.exp(z).sum(-1, keepdims=True))
        e = (np.round(e) if i % 3 == 0 else e).astype(np.float32)
        labels = [int(v) for v in rng.integers(1, C, U)]
        fs, fst = K.kws_frames(e, labels)
        finite = fs[np.isfinite(fs)]
        thr = np.float32(np.quantile(finite, (0.3, 0.6, 0.9)[i % 3])) if finite.size else np.float32(-1)
        out.append((e, labels, thr, fs, fst))
    return out


def plan(kind, T, rng):
    if kind == "every":
        return [1] * T
    if kind == "one":
        return [T]
    cuts = []
    while sum(cuts) < T:
        cuts.append(int(min(rng.integers(0, 12), T - sum(cuts))))     # (0: an empty feed)
    return cuts


def triples(hits, final=None):
    return [(int(s), int(e), np.float32(v).tobytes()) for s, e, v, f in hits if final is None or bool(f) == final]


def one_call(fs, fst, thr, n):
    hs, he, hv, nh = K.kws_pick(fs[:n], fst[:n], thr, MAX_HITS)
    assert nh <= MAX_HITS
    return sorted((int(s), int(e), np.float32(v).tobytes()) for s, e, v in zip(hs[:nh], he[:nh], hv[:nh]))


def test_the_lattice_is_causal():
    """what the oracle (and a stream) relies on: the first n rows of the lattice on T frames are the lattice on the first n frames"""
    e, labels, _, _, _ = next(p for p in random_problems() if p[0].shape[0] >= 40)
    V, St = K.kws_lattice(e, labels)
    for n in (1, 17, 39):
        v, s = K.kws_lattice(e[:n], labels)
        assert np.array_equal(v, V[:n]) and np.array_equal(s, St[:n])


@pytest.mark.parametrize("kind", ["every", "random", "one"])
def test_finals_plus_tentatives_are_the_one_call_pick_on_every_prefix(kind):
    rng = np.random.default_rng(7)
    n_ties = n_withheld = 0
    for e, labels, thr, fs, fst in random_problems():
        st = S.KwsStream(e, labels, thr, MAX_HITS)
        finals = []
        for frames in plan(kind, e.shape[0], rng):
            r = st.feed(frames)
            new = triples(r["hits"], True)
            assert not set(new) & set(finals)                            # a final detection is reported once
            finals += new
            tentative = triples(r["hits"], False)
            n_withheld += bool(tentative)
            assert sorted(finals + tentative) == one_call(fs, fst, thr, st.n)
            assert r["forced"] == 0 and r["dropped"] == 0 and r["frames"] == st.n and r["tail"] <= st.n
            assert all(t >= r["tail"] for t, _, _ in st.pend) and all(e_ <= r["tail"] for _, e_, _ in new)
        r = st.feed(0, finish=True)
        assert all(f for _, _, _, f in r["hits"]) and not st.pend and r["tail"] == st.n
        finals += triples(r["hits"])
        assert sorted(finals) == one_call(fs, fst, thr, st.n) and len(set(finals)) == len(finals)
        sc = fs[np.isfinite(fs) & (fs >= thr)]
        n_ties += sc.size != np.unique(sc).size
    assert n_ties >= 5 and (kind == "one" or n_withheld > 0)             # the problems do hold ties and withheld detections


def test_the_two_passes_select_what_one_pass_would():
    pend = [(5, 2, np.float32(-1)), (6, 2, np.float32(-0.5)), (9, 8, np.float32(-2)), (12, 10, np.float32(-0.25)), (13, 10, np.float32(-0.25))]
    hits, n = S.pick_two_pass(pend, 8, 8)
    assert [(h[0], h[1], h[3]) for h in hits] == [(2, 7, 1), (10, 13, 0), (8, 10, 0)] and n == 3
    hits, n = S.pick_two_pass(pend, 8, 2)                                # the final one takes its slot first
    assert [(h[0], h[1], h[3]) for h in hits] == [(2, 7, 1), (10, 13, 0)] and n == 3
    assert S.pick_two_pass(pend, 8, 3)[1] == 3 and S.pick_two_pass([], 0, 1) == ([], 0)


@pytest.mark.parametrize("max_lag", [0, 3, 20])
def test_with_max_lag_finals_never_overlap_and_the_lag_is_bounded(max_lag):
    rng = np.random.default_rng(11)
    n_forced = 0
    for e, labels, thr, fs, fst in random_problems():
        st = S.KwsStream(e, labels, thr, MAX_HITS, max_lag=max_lag)
        spans = []
        for frames in plan("random", e.shape[0], rng):
            r = st.feed(frames)
            assert r["frames"] - r["tail"] <= max_lag and r["tail"] >= 0
            spans += [(s, e_) for s, e_, _, f in r["hits"] if f]
        spans += [(s, e_) for s, e_, _, f in st.feed(0, finish=True)["hits"]]
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
        n_forced += st.forced
    assert n_forced > 0


def test_a_full_pending_list_drops_and_counts():
    p, kws = P.planted_five()
    e = P.as_log32(p)[0]
    thr = P.thr_of(kws, 0.02)[0]
    fs, _ = K.kws_frames(e, kws[0])
    n_cand = int((np.isfinite(fs) & (fs >= thr)).sum())
    st = S.KwsStream(e, kws[0], thr, 8, pending=2)
    r = st.feed(e.shape[0])
    assert n_cand > 2 and r["dropped"] == n_cand - 2 and len(st.pend) <= 2


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_sized():
    from asr_amd import _lib, ops
    from asr_amd.decoders import KeywordSpotter, KeywordStream
    from asr_amd import DeepSpeech
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in ("ds2_ctc_kws_stream_feed_f32", "ds2_ctc_kws_stream_state_bytes", "ds2_ctc_kws_stream_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_ctc_kws_stream_feed_f32"][1]) == 35
    assert callable(ops.ctc_kws_stream_state) and callable(ops.ctc_kws_stream_feed) and callable(KeywordSpotter.open_stream)
    assert KeywordStream.feed and KeywordStream.finish and callable(DeepSpeech.spot_stream)
    assert lib.ds2_ctc_kws_stream_state_bytes(1, 1, 1) == 4 * (264 + 3)
    assert lib.ds2_ctc_kws_stream_state_bytes(64, 16, 1024) == 4 * 64 * 16 * (264 + 3 * 1024)
    assert lib.ds2_ctc_kws_stream_state_bytes(4096, 4096, 65536) == 4 * 4096 * 4096 * (264 + 3 * 65536)     # sized in 64 bits
    for bad in ((0, 1, 1), (1, 0, 1), (-1, 1, 1), (1, 1, 0), (1, 1, 65537), (1, 1, -1), (1 << 20, 1 << 12, 1)):
        assert lib.ds2_ctc_kws_stream_state_bytes(*bad) == 0, bad
    assert lib.ds2_ctc_kws_stream_workspace_bytes(4, 50, 3, 0) == 4 * 4 * 50 * 7
    assert lib.ds2_ctc_kws_stream_workspace_bytes(4, 50, 3, 1) == 4 * 4 * 50 and lib.ds2_ctc_kws_stream_workspace_bytes(4, 0, 3, 0) == 0


def test_entry_rejects_bad_arguments_before_any_launch():
    from asr_amd import _lib
    lib = _lib.load()
    p = 4096                                                           # any non-null address: every call below returns before a launch
    need, ws = lib.ds2_ctc_kws_stream_state_bytes(2, 3, 16), lib.ds2_ctc_kws_stream_workspace_bytes(2, 10, 3, 0)
    ok = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, in_lens=None, labels=p, off=p, lens=p, K=3, max_u=5, thr=p, max_hits=4,
              max_lag=-1, finish=0, pending=16, bound=0, state=p, state_bytes=need, fs=None, fst=None, hs=p, he=p, hv=p, hf=p, nh=p, tail=p,
              frames=p, forced=p, dropped=p, ws=p, wsb=ws, stream=None)
    for bad in (dict(x=None), dict(state=None), dict(labels=None), dict(off=None), dict(lens=None), dict(thr=None), dict(hs=None),
                dict(he=None), dict(hv=None), dict(hf=None), dict(nh=None), dict(tail=None), dict(frames=None), dict(forced=None),
                dict(dropped=None), dict(fs=p), dict(fst=p), dict(ws=None), dict(wsb=ws - 1), dict(B=0), dict(T=-1), dict(C=0), dict(K=0),
                dict(ld_b=0), dict(ld_t=0), dict(is_log=2), dict(finish=2), dict(finish=-1), dict(max_u=64), dict(max_hits=0),
                dict(max_hits=1025), dict(pending=0), dict(pending=65537), dict(state_bytes=need - 1), dict(state_bytes=0),
                dict(bound=-1), dict(bound=(1 << 31) - 10), dict(bound=1 << 40), dict(B=1 << 20, K=1 << 12)):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_kws_stream_feed_f32(*a.values()) != 0, bad
        assert lib.ds2_last_error().startswith(b"ds2_ctc_kws_stream_feed_f32: "), (bad, lib.ds2_last_error())
    assert b"state too small" in (lib.ds2_ctc_kws_stream_feed_f32(*dict(ok, state_bytes=need - 1).values()), lib.ds2_last_error())[1]
    assert b"2^31" in (lib.ds2_ctc_kws_stream_feed_f32(*dict(ok, bound=(1 << 31) - 10).values()), lib.ds2_last_error())[1]


def test_ops_refuse_on_the_host():
    from asr_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    x, state, thr = torch.zeros((1, 4, 5)), torch.zeros(4 * (264 + 3 * 8), dtype=torch.uint8), torch.zeros(1)
    for bad in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (1, 1, 65537), (1.5, 1, 8)):
        with pytest.raises(ValueError, match="ctc_kws_stream_state"):
            ops.ctc_kws_stream_state(*bad, "cpu")
    with pytest.raises(ValueError, match="GPU"):
        ops.ctc_kws_stream_feed(x, None, state, i32(1), i32(0), i32(1), 1, thr, 8, 0)
    with pytest.raises(ValueError, match="classes"):
        ops.ctc_kws_stream_feed(None, None, state, i32(1), i32(0), i32(1), 1, thr, 8, 0, finish=True)
    for kw, match in ((dict(max_hits=0), "max_hits"), (dict(max_hits=1025), "max_hits"), (dict(max_lag=-1), "max_lag"), (dict(max_lag=0.5), "max_lag")):
        with pytest.raises(ValueError, match=match):
            ops.ctc_kws_stream_feed(x, None, state, i32(1), i32(0), i32(1), 1, thr, 8, 0, **kw)
    with pytest.raises(ValueError, match="pending"):
        ops.ctc_kws_stream_feed(x, None, state, i32(1), i32(0), i32(1), 1, thr, 0, 0)
    with pytest.raises(ValueError, match="max_kw_len"):
        ops.ctc_kws_stream_feed(x, None, state, i32(1), i32(0), i32(1), 64, thr, 8, 0)


def test_open_stream_and_feed_refuse_on_the_host():
    from asr_amd.decoders import KeywordSpotter, KeywordStream
    sp = KeywordSpotter(LABELS, ["cat", "to"], threshold=0.25, max_hits=5)
    for kw, match in ((dict(batch=0), "batch"), (dict(batch=1.5), "batch"), (dict(max_lag=-1), "max_lag"), (dict(max_lag=2.5), "max_lag"),
                      (dict(pending=0), "pending"), (dict(pending=65537), "pending")):
        with pytest.raises(ValueError, match=match):
            sp.open_stream(**kw)
    st = sp.open_stream(batch=2, max_lag=30, pending=16)
    assert isinstance(st, KeywordStream) and (st.batch, st.max_lag, st.pending, st.max_hits) == (2, 30, 16, 5)
    assert st.frames == [0, 0] and st.detections == [[], []] and not st.closed and st.forced.shape == (2, 2) and not st.dropped.any()
    sp.set_keywords(["dog"], threshold=0.9)                             # the stream keeps its own packed image
    assert st.keywords == ["cat", "to"] and st.kw_ids == [[4, 2, 21], [21, 16]]
    assert st._image.tolist()[:4] == [0, 3, 3, 2] and st._image.tolist()[6:] == [4, 2, 21, 21, 16]
    assert st._image[4:6].view(np.float32).tolist() == [np.float32(3 * np.log(0.25)), np.float32(2 * np.log(0.25))]
    p = torch.full((2, 9, 29), 1 / 29)
    for args, match in (((p[0],), r"\(2, T, C\)"), ((p[:1],), r"\(2, T, C\)"), ((p[:, :0],), "at least one frame"), ((p, [9]), "sizes"),
                        ((p, [9, 10]), "outside"), ((p, [-1, 3]), "outside"), ((p, torch.tensor([1.0, 2.0])), "integers")):
        with pytest.raises(ValueError, match=match):
            st.check_feed(*args)
    assert st.C is None
    probs, n = st.check_feed(p, [9, 0])
    assert n == [9, 0] and st.C == 29
    with pytest.raises(ValueError, match="29 classes"):
        st.check_feed(torch.full((2, 9, 30), 1 / 30))
    st.frames = [(1 << 31) - 5, 0]
    with pytest.raises(ValueError, match="2\\^31"):
        st.check_feed(p)
    st.closed = True
    with pytest.raises(ValueError, match="closed"):
        st.check_feed(p)
    with pytest.raises(ValueError, match="closed"):
        st.finish()
    one = sp.open_stream()
    assert one.check_feed(torch.full((9, 29), 1 / 29))[0].shape == (1, 9, 29)


def test_stream_records_carry_final_and_sort_as_search_sorts():
    from asr_amd.decoders import assemble_stream_detections
    hs = np.array([[[30, 5, -1], [7, -1, -1]]], np.int32)
    he = np.array([[[34, 9, -1], [9, -1, -1]]], np.int32)
    hv = np.array([[[0.0, -1.5, -np.inf], [-0.5, -np.inf, -np.inf]]], np.float32)
    hf = np.array([[[0, 1, 0], [1, 0, 0]]], np.int32)
    recs, over = assemble_stream_detections(hs, he, hv, hf, np.array([[4, 1]], np.int32), ["cat", "at"], [3, 2], 2)
    assert over == [(0, "cat")]
    assert [(r["keyword"], r["start"], r["end"], r["final"]) for r in recs[0]] == [("cat", 5, 9, True), ("at", 7, 9, True), ("cat", 30, 34, False)]


def test_spot_stream_has_spot_longs_arguments():
    import inspect
    from asr_amd import DeepSpeech
    sig = inspect.signature(DeepSpeech.spot_stream).parameters
    assert list(sig) == list(inspect.signature(DeepSpeech.spot_long).parameters) + ["max_lag"] and sig["max_lag"].default is None
