"""GPU (-m gpu): streaming keyword search (csrc/ctc_kws_stream.h, `ds2_ctc_kws_stream_feed_f32`).  With log-probability input every output
of every feed is compared bit for bit: the per-frame arrays, concatenated over the feeds, with `ops.ctc_keyword_search` on the
concatenated frames; hits, tail, frames and the two counters with tests/ctc_kws_stream_oracle.py; and, after every feed, the finals so
far plus the tentatives with the one-call pick on the frames consumed.  Then KeywordSpotter.open_stream and DeepSpeech.spot_stream end
to end.  Shapes are the smallest at which each path can still go wrong; a feed is three launches and one copy back."""
import functools
import os
import tempfile
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import det
import ctc_kws_oracle as K
import ctc_kws_stream_oracle as S
import kws_problems as P

pytestmark = pytest.mark.gpu

LABELS = "_'abcdefghijklmnopqrstuvwxyz "


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def log_softmax64(shape, seed, scale=4.0):
    z = det.uniform01(shape, seed).astype(np.float64) * scale
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def pack(kws, dev):
    lens = np.array([len(k) for k in kws], np.int32)
    off = np.zeros(len(kws), np.int32)
    off[1:] = np.cumsum(lens)[:-1]
    t = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    return t([c for k in kws for c in k]), t(off), t(lens), int(lens.max(initial=0))


def cyc(n, C, start=0):
    return [1 + (start + i) % (C - 1) for i in range(n)]


def bits(a):
    a = np.asarray(a)
    return (a + np.float32(0)).view(np.int32) if a.dtype == np.float32 else a


class Run:
    """One stream over a batch at the level of ops, with the oracle's streams beside it.  x (B,T,C) on the host, lens (B) the frames of
    every utterance; feed(chunk) gives every utterance its next min(chunk, what is left) frames (`starved`: utterances that get none),
    as a strided view of the device tensor, and returns the outputs on the host."""

    def __init__(self, dev, x, kws, thr, lens, max_hits=8, pending=1024, max_lag=None, is_log=True, xd=None, oracle=True, dtype=np.float32):
        from asr_amd import ops
        self.ops, self.dev, self.x, self.kws, self.thr = ops, dev, np.asarray(x), kws, np.asarray(thr, np.float32)
        B, T, _ = self.x.shape
        self.lens = [T] * B if lens is None else list(lens)
        self.xd = torch.from_numpy(np.ascontiguousarray(self.x)).to(dev) if xd is None else xd
        self.labels, self.off, self.kwl, self.max_u = pack(kws, dev)
        self.thr_d = torch.from_numpy(self.thr).to(dev)
        self.max_hits, self.pending, self.max_lag, self.is_log = max_hits, pending, max_lag, is_log
        self.state = ops.ctc_kws_stream_state(B, len(kws), pending, dev)
        self.cur, self.t0 = [0] * B, 0
        self.frames = [[[] for _ in kws] for _ in range(B)]                     # the per-frame outputs of every feed, per (b, k)
        self.oracle = None
        if oracle:
            with np.errstate(divide="ignore"):
                e = self.x.astype(dtype) if is_log else np.log(self.x.astype(dtype))
            self.oracle = [[S.KwsStream(e[b, :self.lens[b]], kw, self.thr[k] if dtype is np.float32 else float(self.thr[k]), max_hits,
                                        pending, max_lag) for k, kw in enumerate(kws)] for b in range(B)]

    def feed(self, chunk, finish=False, starved=(), return_frames=True):
        B = len(self.lens)
        n = [0 if b in starved else min(chunk, self.lens[b] - self.cur[b]) for b in range(B)]
        view = self.xd[:, self.t0:self.t0 + max(chunk, 1)]                       # (an empty feed: one frame that no utterance takes)
        assert view.shape[1] >= max(n)
        out = self.ops.ctc_kws_stream_feed(view, torch.tensor(n, dtype=torch.int32), self.state, self.labels, self.off, self.kwl, self.max_u,
                                           self.thr_d, self.pending, max(self.cur), self.is_log, self.max_hits, self.max_lag, finish,
                                           return_frames)
        torch.cuda.synchronize()
        names = ("hit_start", "hit_end", "hit_score", "hit_final", "n_hits", "tail", "frames", "forced", "dropped", "frame_score", "frame_start")
        got = {k: None if v is None else v.cpu().numpy() for k, v in zip(names, out)}
        for b in range(B):
            for k in range(len(self.kws)):
                if return_frames:
                    assert not np.isfinite(got["frame_score"][b, k, n[b]:]).any() and (got["frame_start"][b, k, n[b]:] == -1).all()
                    self.frames[b][k].append((got["frame_score"][b, k, :n[b]], got["frame_start"][b, k, :n[b]]))
            self.cur[b] += n[b]
        self.t0 = min(self.t0 + chunk, self.x.shape[1])
        got["n"] = n
        return got

    def flush(self):
        out = self.ops.ctc_kws_stream_feed(None, None, self.state, self.labels, self.off, self.kwl, self.max_u, self.thr_d, self.pending,
                                           max(self.cur), self.is_log, self.max_hits, self.max_lag, True, classes=self.x.shape[2],
                                           batch=len(self.lens))
        torch.cuda.synchronize()
        names = ("hit_start", "hit_end", "hit_score", "hit_final", "n_hits", "tail", "frames", "forced", "dropped")
        got = {k: v.cpu().numpy() for k, v in zip(names, out)}
        got["n"] = [0] * len(self.lens)
        return got

    def check_against_oracle(self, got, finish=False, what=""):
        """every hit, tail, frames and counter of this feed equal the oracle's, to the integer and the bit"""
        for b, row in enumerate(self.oracle):
            for k, st in enumerate(row):
                w = st.feed(got["n"][b], finish)
                nh = min(w["n_hits"], self.max_hits)
                where = (what, b, k, st.n)
                assert got["n_hits"][b, k] == w["n_hits"], where + (got["n_hits"][b, k], w["n_hits"])
                assert [got[f][b, k] for f in ("tail", "frames", "forced", "dropped")] == [w[f] for f in ("tail", "frames", "forced", "dropped")], where
                hits = list(zip(got["hit_start"][b, k, :nh].tolist(), got["hit_end"][b, k, :nh].tolist(),
                                bits(got["hit_score"][b, k, :nh]).tolist(), got["hit_final"][b, k, :nh].tolist()))
                assert hits == [(s, e, int(bits(np.float32(v))), f) for s, e, v, f in w["hits"][:nh]], where
                assert (got["hit_start"][b, k, nh:] == -1).all() and (got["hit_end"][b, k, nh:] == -1).all(), where
                assert (got["hit_score"][b, k, nh:] == -np.inf).all() and (got["hit_final"][b, k, nh:] == 0).all(), where

    def all_frames(self, b, k):
        return (np.concatenate([f[0] for f in self.frames[b][k]] or [np.zeros(0, np.float32)]),
                np.concatenate([f[1] for f in self.frames[b][k]] or [np.zeros(0, np.int32)]))


def one_call(dev, x, kws, thr, lens, max_hits=8, xd=None):
    """ops.ctc_keyword_search on the whole batch: the yardstick of the per-frame arrays and of the finished stream"""
    from asr_amd import ops
    labels, off, kwl, max_u = pack(kws, dev)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev) if xd is None else xd
    out = ops.ctc_keyword_search(xd, labels, off, kwl, max_u, torch.from_numpy(np.asarray(thr, np.float32)).to(dev),
                                 None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev), True, max_hits)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def hit_set(hs, he, hv, n):
    return sorted(zip(hs[:n].tolist(), he[:n].tolist(), bits(np.asarray(hv[:n], np.float32)).tolist()))


# ---- frames ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_problem():
    """B = 4, T_b = (150, 129, 64, 37), C = 7; keywords of U = 1, U = 63 (the last lane) and U = 3 with a doubled label; a threshold
    per keyword read off the oracle's frame scores so that the pick has work (the 0.8 quantile of the finite ones)"""
    T, C = 150, 7
    kws = [[5], cyc(63, C, 3), [4, 4, 2]]
    x = log_softmax64((4, T, C), det.seed_of("kws.stream.ragged")).astype(np.float32)
    lens = [150, 129, 64, 37]
    thr = np.full(3, -1.0, np.float32)
    for k, kw in enumerate(kws):
        f = np.concatenate([K.kws_frames(x[b, :lens[b]], kw)[0] for b in range(4)])
        f = np.sort(f[np.isfinite(f)])
        thr[k] = f[int(0.8 * (f.size - 1))]
    return x, kws, thr, lens


def three():
    p, kws, thr = P.planted_three()
    return P.as_log32(p), kws, thr, None


PLANS = {"one frame per feed": None, "63, 1, 64, rest": (63, 1, 64, 1000), "7, 8, 9, rest": (7, 8, 9, 1000), "a single feed": (1000,),
         "empty feeds in between": (0, 10, 0, 0, 50, 0, 1000, 0)}


def frames_check(dev, problem, plan, chunks, starved=()):
    """the per-frame arrays of all feeds, concatenated, against ops.ctc_keyword_search on the frames every utterance got; every feed's
    hits and counters against the stream oracle; after the flush everything is consumed and settled"""
    x, kws, thr, lens = problem
    B, T, _ = x.shape
    run = Run(dev, x, kws, thr, lens)
    for c in chunks or (1,) * T:
        run.check_against_oracle(run.feed(c, starved=starved), what=plan)
    want_lens = [0 if b in starved else (T if lens is None else lens[b]) for b in range(B)]
    assert run.cur == want_lens
    fs, fst, hs, he, hv, nh = one_call(dev, x, kws, thr, want_lens)
    for b in range(B):
        for k in range(len(kws)):
            gs, gst = run.all_frames(b, k)
            assert np.array_equal(bits(gs), bits(fs[b, k, :want_lens[b]])) and np.array_equal(gst, fst[b, k, :want_lens[b]]), (plan, b, k)
    got = run.flush()
    run.check_against_oracle(got, True, plan + ", flush")
    for b in range(B):
        for k in range(len(kws)):
            assert got["frames"][b, k] == want_lens[b] and got["tail"][b, k] == want_lens[b]


@pytest.mark.parametrize("problem", ["three", "ragged"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_frames_over_any_cuts_have_the_bits_of_the_one_call_search(dev, problem, plan):
    frames_check(dev, three() if problem == "three" else ragged_problem(), plan, PLANS[plan])


def test_an_utterance_that_never_gets_a_frame(dev):
    frames_check(dev, ragged_problem(), "utterance 1 starved", (40, 1000), starved=(1,))


def test_one_plan_against_the_oracle_directly(dev):
    """the per-frame arrays of the (7, 8, 9, rest) plan against tests/ctc_kws_oracle.py itself, not against the device's one-call search"""
    x, kws, thr, lens = ragged_problem()
    run = Run(dev, x, kws, thr, lens, oracle=False)
    for c in (7, 8, 9, 1000):
        run.feed(c)
    for b in range(4):
        for k, kw in enumerate(kws):
            ws, wst = K.kws_frames(x[b, :lens[b]], kw)
            gs, gst = run.all_frames(b, k)
            assert np.array_equal(bits(gs), bits(ws)) and np.array_equal(gst, wst), (b, k)


# ---- the prefix property ---------------------------------------------------------------------------------------------------------
def five():
    p, kws = P.planted_five()
    return P.as_log32(p), kws, P.thr_of(kws, 0.02)


def prefix_check(dev, x, kws, thr, chunks, max_hits=8):
    """after every feed: finals so far + tentatives == the one-call pick on the frames consumed; a final is reported once; the flush
    leaves exactly the one-call search's hits"""
    fs, fst = K.kws_frames(x[0], kws[0])
    run = Run(dev, x, kws, thr, None, max_hits)
    finals, n_tentative = [], 0
    for c in chunks:
        got = run.feed(c, return_frames=False)
        run.check_against_oracle(got)
        n = run.cur[0]
        nh = int(got["n_hits"][0, 0])
        assert nh <= max_hits
        fin = got["hit_final"][0, 0, :nh].astype(bool)
        new = hit_set(got["hit_start"][0, 0, :nh][fin], got["hit_end"][0, 0, :nh][fin], got["hit_score"][0, 0, :nh][fin], int(fin.sum()))
        tent = hit_set(got["hit_start"][0, 0, :nh][~fin], got["hit_end"][0, 0, :nh][~fin], got["hit_score"][0, 0, :nh][~fin], int((~fin).sum()))
        assert not set(new) & set(finals), (n, new, finals)
        finals += new
        n_tentative += len(tent)
        whs, whe, whv, wn = K.kws_pick(fs[:n], fst[:n], thr[0], max_hits)
        assert sorted(finals + tent) == hit_set(whs, whe, whv, wn), (n, finals, tent)
    got = run.flush()
    run.check_against_oracle(got, True)
    nh = int(got["n_hits"][0, 0])
    assert got["hit_final"][0, 0, :nh].all()
    finals += hit_set(got["hit_start"][0, 0], got["hit_end"][0, 0], got["hit_score"][0, 0], nh)
    _, _, hs, he, hv, wn = one_call(dev, x, kws, thr, None, max_hits)
    assert sorted(finals) == hit_set(hs[0, 0], he[0, 0], hv[0, 0], int(wn[0, 0])) and len(finals) == 5
    return n_tentative


def test_prefix_property_cut_at_every_frame(dev):
    x, kws, thr = five()
    assert prefix_check(dev, x, kws, thr, (1,) * 200) > 0


def test_a_rival_that_arrives_in_a_later_feed_is_killed_by_the_carried_list(dev):
    x, kws, thr = five()
    fs, fst = K.kws_frames(x[0], kws[0])
    hs, he, hv, n = K.kws_pick(fs, fst, thr[0], 8)
    ends = sorted(int(e) for e in he[:n])[:2]                                  # the accepted candidates of the plants at 20 and 60 ...
    for e in ends:                                                           # ... and their rivals, one frame later and weaker
        assert fs[e] >= thr[0] and fs[e] < fs[e - 1] and fst[e] <= e - 1
    cuts = sorted({21, 61, *ends})                                           # frames 20 | 21 and 60 | 61, and each candidate | its rival
    chunks = [b - a for a, b in zip([0] + cuts, cuts)] + [1000]
    prefix_check(dev, x, kws, thr, chunks)


# ---- ties, a keyword across a cut --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TIE_ENTER", "TIE_STAY_STEP", "TIE_STEP_SKIP"])
def test_tie_rules_across_a_cut(dev, name):
    tie = getattr(P, name)
    x, kws, thr = P.tie_e(tie)[None], [tie["labels"]], np.array([-100.0], np.float32)
    T = x.shape[1]
    want = P.batch32(x, None, kws, thr, 4)
    # a cut one frame before the tie frame, at it (the tie frame is the next feed's first) and after it (it is this feed's last)
    cuts = range(1, T) if "t" not in tie else (tie["t"] - 1, tie["t"], tie["t"] + 1)
    for cut in cuts:
        run = Run(dev, x, kws, thr, None, 4)
        for c in (cut, 1000):
            run.check_against_oracle(run.feed(c), what=(name, cut))
        gs, gst = run.all_frames(0, 0)
        assert np.array_equal(bits(gs), bits(want[0][0, 0])) and np.array_equal(gst, want[1][0, 0]), (name, cut)
        if "t" in tie:
            assert gst[tie["t"]] == tie["winner"]
        got = run.flush()
        run.check_against_oracle(got, True)


def test_a_keyword_planted_across_a_cut(dev):
    x, kws, thr, _ = three()                                                  # plants at 10 .. 14, 50 .. 54, 90 .. 94
    run = Run(dev, x, kws, thr, None)
    finals = []
    for c in (12, 40, 41, 1000):                                              # cuts inside the first plant, inside the second, after the third's first label
        got = run.feed(c)
        run.check_against_oracle(got)
        nh = int(got["n_hits"][0, 0])
        finals += [(int(s), int(e)) for s, e, f in zip(got["hit_start"][0, 0, :nh], got["hit_end"][0, 0, :nh], got["hit_final"][0, 0, :nh]) if f]
    got = run.flush()
    nh = int(got["n_hits"][0, 0])
    finals += list(zip(got["hit_start"][0, 0, :nh].tolist(), got["hit_end"][0, 0, :nh].tolist()))
    assert sorted(finals) == [(10, 15), (50, 55), (90, 95)] and int(got["n_hits"][0, 1]) == 0


# ---- forced cuts -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def withheld_problem():
    """T = 100, C = 29.  KW whole at 30 .. 34 with the blank a close second (0.45 against 0.5) in its label frames: in frame 34 the path
    that makes the hit [30, 35) at score 0 also stays behind in the blank before the last label, at log(0.45 / 0.5) = -0.105, and waits
    there through the silence at that value: the keyword up to its last label but one, a path above the threshold that began no
    later than the hit.  The last label alone at frame 80 lets it end: a candidate [30, 81) that the hit kills, or, after a forced cut,
    one that began before the tail."""
    close = lambda c: (c, 0.5, 0, 0.45)
    p = P.planted(100, 29, [(30, [close(3), 0, close(3), close(7), close(5)]), (80, [5])])[None]
    return P.as_log32(p), [P.KW], P.thr_of([P.KW], 0.5)


def test_a_hit_is_withheld_while_an_older_path_lives(dev):
    x, kws, thr = withheld_problem()
    run = Run(dev, x, kws, thr, None)
    for c in (40, 30):                                                       # 35 frames of silence after the hit, and it is still tentative
        got = run.feed(c)
        run.check_against_oracle(got)
        assert got["n_hits"][0, 0] == 1 and got["hit_final"][0, 0, 0] == 0 and got["tail"][0, 0] == 30
        assert (got["hit_start"][0, 0, 0], got["hit_end"][0, 0, 0]) == (30, 35) and got["forced"][0, 0] == 0 and got["dropped"][0, 0] == 0
    got = run.feed(30)                                                       # frame 80 ends the waiting path: the hit kills its candidate
    run.check_against_oracle(got)
    assert got["n_hits"][0, 0] == 1 and got["hit_final"][0, 0, 0] == 1 and got["hit_end"][0, 0, 0] == 35 and got["tail"][0, 0] == 100
    got = run.flush()
    run.check_against_oracle(got, True)
    assert got["n_hits"][0, 0] == 0 and got["dropped"][0, 0] == 0


def lagged_run(dev, max_lag, chunk):
    """the withheld problem in feeds of `chunk` frames under max_lag, every feed equal to the oracle (forced, dropped and every hit, to the
    integer) -> (the frames consumed when the hit [30, 35) was reported final, or None; the last feed's outputs)"""
    x, kws, thr = withheld_problem()
    run = Run(dev, x, kws, thr, None, max_lag=max_lag)
    final_at = None
    for _ in range(-(-100 // chunk)):
        got = run.feed(chunk)
        run.check_against_oracle(got, what=(max_lag, chunk))
        n = run.cur[0]
        assert n - got["tail"][0, 0] <= max_lag
        nh = int(got["n_hits"][0, 0])
        if any(got["hit_final"][0, 0, h] and got["hit_end"][0, 0, h] == 35 for h in range(nh)):
            assert final_at is None
            final_at = n
    run.check_against_oracle(run.flush(), True)
    return final_at, got


@pytest.mark.parametrize("max_lag,chunk", [(20, 5), (25, 5), (20, 10)])
def test_max_lag_makes_it_final_within_that_many_frames(dev, max_lag, chunk):
    """What max_lag bounds is frames - tail after every feed (lagged_run asserts it).  The hit ends at 35, so it is final in the first
    feed that ends at or after 35 + max_lag: exactly max_lag frames after its end where a feed ends there (the first two cases), and up
    to chunk - 1 frames later where none does (the third: 25 frames at max_lag = 20 in feeds of 10)."""
    final_at, got = lagged_run(dev, max_lag, chunk)
    assert final_at is not None and final_at == -(-(35 + max_lag) // chunk) * chunk
    assert final_at - 35 == (max_lag if (35 + max_lag) % chunk == 0 else 25)
    assert got["forced"][0, 0] > 0 and got["dropped"][0, 0] == 1              # the candidate of frame 80 began before the tail


def test_a_forced_cut_inside_a_candidate_loses_it(dev):
    """the price of the rule as the contract states it: while the older path lives, feeds of one frame sweep the forced cut through every
    frame, the hit's own among them, and the hit is dropped and counted instead of reported"""
    final_at, got = lagged_run(dev, 20, 1)
    assert final_at is None and got["forced"][0, 0] > 0 and got["dropped"][0, 0] == 2


# ---- overflow ----------------------------------------------------------------------------------------------------------------------
def test_a_full_pending_list_is_counted(dev):
    x, kws, thr = five()
    fs, _ = K.kws_frames(x[0], kws[0])
    n_cand = int((np.isfinite(fs) & (fs >= thr[0])).sum())
    run = Run(dev, x, kws, thr, None, pending=4)
    got = run.feed(1000)
    run.check_against_oracle(got)
    assert n_cand > 4 and got["dropped"][0, 0] == n_cand - 4
    run.check_against_oracle(run.flush(), True)


def test_final_detections_take_the_slots_before_tentative_ones(dev):
    x, kws, _ = five()                                                        # scores about (0, -0.67, -3.76, 0, -3.76) at 20, 60, 100, 140, 180
    thr = P.thr_of(kws, 0.5)                                                  # (the plants at 20, 60 and 140 pass it)
    run = Run(dev, x, kws, thr, None, max_hits=1)
    got = run.feed(30)
    run.check_against_oracle(got)
    assert got["n_hits"][0, 0] == 1 and got["hit_final"][0, 0, 0] == 1 and got["hit_start"][0, 0, 0] == 20
    got = run.feed(113)                                                       # 143 frames: a final at 60 (-0.67), the plant at 140 tentative at score 0
    run.check_against_oracle(got)
    assert got["n_hits"][0, 0] == 2 and got["hit_final"][0, 0, 0] == 1 and got["hit_start"][0, 0, 0] == 60
    assert np.float32(got["hit_score"][0, 0, 0]) < -0.5                       # a one-pass pick would have given the slot to the tentative 0


def test_keyword_stream_warns_on_both_overflows(dev):
    from asr_amd.decoders import KeywordSpotter
    p, kws = P.planted_five()
    word = "".join(LABELS[c] for c in kws[0])
    probs = torch.from_numpy(p.astype(np.float32))
    with pytest.warns(RuntimeWarning, match="pending=4"):
        KeywordSpotter(LABELS, [word], threshold=0.02, max_hits=8).open_stream(pending=4).feed(probs)
    with pytest.warns(RuntimeWarning, match="max_hits=1 "):
        KeywordSpotter(LABELS, [word], threshold=0.02, max_hits=1).open_stream().feed(probs)


# ---- input forms -------------------------------------------------------------------------------------------------------------------
def test_strided_input_gives_identical_results(dev):
    x, kws, thr, lens = ragged_problem()
    B, T, C = x.shape
    xt = torch.from_numpy(x).to(dev)
    tbc = xt.transpose(0, 1).contiguous()                                       # (T,B,C) storage, as the model's eval output
    padded = torch.full((B, T, C + 3), float("nan"), device=dev)
    padded[..., :C] = xt
    for name, view in (("(T,B,C)-backed", tbc.transpose(0, 1)), ("row pitch C + 3", padded[..., :C])):
        run = Run(dev, x, kws, thr, lens, xd=view)
        for c in (50, 37, 1000):
            run.check_against_oracle(run.feed(c), what=name)
        for b in range(B):
            for k, kw in enumerate(kws):
                ws, wst = K.kws_frames(x[b, :lens[b]], kw)
                gs, gst = run.all_frames(b, k)
                assert np.array_equal(bits(gs), bits(ws)) and np.array_equal(gst, wst), (name, b, k)


@pytest.mark.parametrize("which", ["three", "five"])
def test_probability_input_within_the_derived_bound(dev, which):
    """is_log = 0 on the planted problems, cut inside the second plant: the hits and their final flags are the float64 stream oracle's on
    the logs of the same float32 probabilities, and every score is within kws_problems.prob_tol of it, n the frames of its span"""
    if which == "three":
        p, kws, thr = P.planted_three()
    else:
        p, kws = P.planted_five()
        thr = P.thr_of(kws, 0.02)
    x = p.astype(np.float32)
    T = x.shape[1]
    M = np.abs(np.log(x.astype(np.float64))).max()
    run = Run(dev, x, kws, thr, None, is_log=False, dtype=np.float64)
    for c, finish in ((52 if which == "three" else 62, False), (1000, False), (0, True)):   # (the second plant's third frame begins the next feed)
        got = run.flush() if finish else run.feed(c)
        for k in range(len(kws)):
            w = run.oracle[0][k].feed(got["n"][0], finish)
            nh = int(got["n_hits"][0, k])
            assert nh == w["n_hits"] and got["tail"][0, k] == w["tail"] and got["dropped"][0, k] == 0
            for h, (s, e, v, f) in enumerate(w["hits"]):
                assert (got["hit_start"][0, k, h], got["hit_end"][0, k, h], got["hit_final"][0, k, h]) == (s, e, f)
                err, tol = abs(float(got["hit_score"][0, k, h]) - v), P.prob_tol(e - s, M)
                print("hit", (s, e), "score error", err, "bound", tol)
                assert err <= tol
    assert run.oracle[0][0].n == T and sum(len(f[0]) for f in run.frames[0][0]) == T


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_unchanged(dev):
    from asr_amd import _lib
    x, kws, thr, _ = three()
    run = Run(dev, x, kws, thr, None, oracle=False)
    run.feed(60)
    lib = _lib.load()
    before = run.state.clone()
    assert before.any()
    B, K_, mh = 1, 2, 8
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    hits, tail = i32(4, B, K_, mh), i32(5, B, K_)
    wsb = lib.ds2_ctc_kws_stream_workspace_bytes(B, 60, K_, 0)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    chunk = run.xd[:, 60:120]
    ok = dict(x=chunk.data_ptr(), ld_b=chunk.stride(0), ld_t=chunk.stride(1), B=B, T=60, C=x.shape[2], is_log=1, in_lens=None,
              labels=run.labels.data_ptr(), off=run.off.data_ptr(), lens=run.kwl.data_ptr(), K=K_, max_u=run.max_u, thr=run.thr_d.data_ptr(),
              max_hits=mh, max_lag=-1, finish=0, pending=run.pending, bound=60, state=run.state.data_ptr(), state_bytes=run.state.numel(),
              fs=None, fst=None, hs=hits[0].data_ptr(), he=hits[1].data_ptr(), hv=hits[2].data_ptr(), hf=hits[3].data_ptr(),
              nh=tail[0].data_ptr(), tail=tail[1].data_ptr(), frames=tail[2].data_ptr(), forced=tail[3].data_ptr(), dropped=tail[4].data_ptr(),
              ws=ws.data_ptr(), wsb=wsb, stream=None)
    for bad, text in ((dict(state_bytes=run.state.numel() - 1), b"state too small"), (dict(max_hits=0), b"max_hits"), (dict(max_hits=1025), b"max_hits"),
                      (dict(state=None), b"null pointer"), (dict(bound=(1 << 31) - 60), b"2^31")):
        assert lib.ds2_ctc_kws_stream_feed_f32(*dict(ok, **bad).values()) != 0, bad
        assert text in lib.ds2_last_error(), (bad, lib.ds2_last_error())
        torch.cuda.synchronize()
        assert torch.equal(run.state, before), bad
    assert lib.ds2_ctc_kws_stream_feed_f32(*ok.values()) == 0                 # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert tail[2].tolist() == [[120, 120]] and not torch.equal(run.state, before)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def strip(records):
    return [{k: v for k, v in r.items() if k != "final"} for r in records]


def test_spotter_stream_over_a_ragged_batch_of_two(dev):
    from asr_amd.decoders import KeywordSpotter
    p0 = P.planted_three()[0][0]
    p1 = P.planted(120, 29, [(30, P.KW_PLANT), (70, P.KW_PLANT)])
    x = torch.from_numpy(np.stack([p0, p1]).astype(np.float32))
    sizes = [120, 100]
    words = ["".join(LABELS[c] for c in kw) for kw in (P.KW, P.ABSENT)]
    spotter = KeywordSpotter(LABELS, words, threshold=0.5, max_hits=8)
    want = spotter.search(x, sizes, frame_seconds=0.02)
    assert [len(w) for w in want] == [3, 2]
    stream = spotter.open_stream(batch=2)
    spotter.set_keywords(["zzz"])                                              # the open stream keeps the keywords it was opened with
    cur, seen = [0, 0], [[], []]
    for T, n in ((50, [50, 20]), (40, [40, 40]), (40, [30, 40])):
        chunk = torch.zeros((2, T, 29))
        for b in range(2):
            chunk[b, :n[b]] = x[b, cur[b]:cur[b] + n[b]]
            cur[b] += n[b]
        recs = stream.feed(chunk, n, frame_seconds=0.02)
        for b in range(2):
            assert recs[b] == sorted(recs[b], key=lambda r: (r["start"], r["end"]))
            new = strip(r for r in recs[b] if r["final"])
            assert all(r not in seen[b] for r in new)
            seen[b] += new
    assert stream.frames == sizes and sum(len(s) for s in seen) > 0
    last = stream.finish(frame_seconds=0.02)
    for b in range(2):
        assert all(r["final"] for r in last[b])
        assert seen[b] + strip(last[b]) == want[b] and strip(stream.detections[b]) == want[b]
    assert stream.closed and not stream.forced.any() and not stream.dropped.any()
    with pytest.raises(ValueError, match="closed"):
        stream.feed(x[:, :5])


def test_model_spot_stream_equals_spot_long(dev):
    import pandas as pd
    from asr_amd import DeepSpeech
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                           spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    torch.manual_seed(3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": chars}).to_csv(path, index=False)
        model = DeepSpeech(audio_conf=conf, decoder=None, label_path=path, rnn_type="gru", rnn_hidden_size=32, rnn_hidden_layers=2,
                           bidirectional=True)
    model.to(dev).eval()
    spect = torch.from_numpy(det.unitvar((161, 80), det.seed_of("kws.stream.e2e"))).to(dev)
    keywords = ["ab", "it's", "q"]
    args = dict(window=40, overlap=8, batch_size=2, threshold=0.5, max_hits=64)   # (40 output frames hold at most 40 hits of one label)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # no overflow: the stream is then exactly the one-call search
        want = model.spot_long(spect, keywords, **args)
        items = list(model.spot_stream(spect, keywords, **args))
    assert len(want) > 0 and len(items) == 3                                    # three windows in batches of two, then the flush
    assert [i["final"] for i in items] == [False, False, True] and items[-1]["tentative"] == [] and items[-1]["frames"] == 40
    assert items[0]["frames"] < items[1]["frames"] == 40 and items[1]["seconds"] == 40 * 0.02
    key = lambda r: (r["start"], r["end"], keywords.index(r["keyword"]))
    got = [r for i in items for r in i["detections"]]
    assert sorted(got, key=key) == want and all("final" not in r and "start_s" in r for r in got)
    assert len({(r["keyword"], r["start"], r["end"]) for r in got}) == len(got)   # each final record in exactly one item
