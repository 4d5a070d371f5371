"""CPU: the keyword-search contract (include/ds2hip.h, ds2_ctc_kws_f32) as tests/ctc_kws_oracle.py restates it — against a brute
force, on constructed ties, the pick, planted keywords — and the host half of it: KeywordSpotter, the ctypes signatures and the
argument checks of the entry, none of which needs a GPU."""
import math
import re
import os

import numpy as np
import pytest
import torch

import det
import ctc_kws_oracle as K
import kws_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -np.inf


# ---- (a) the recurrence against a brute force ------------------------------------------------------------------------------------
def brute_scores(d, labels):
    """max over the start frames of a plain Viterbi that begins in state 1 at that frame: (T) values of the end state"""
    T, U = d.shape[0], len(labels)
    S = 2 * U
    cls = [0 if q % 2 == 0 else labels[q >> 1] for q in range(S)]
    best = np.full(T, NEG)
    for t0 in range(T):
        v = np.full(S, NEG)
        v[1] = d[t0, cls[1]]
        best[t0] = max(best[t0], v[S - 1])
        for t in range(t0 + 1, T):
            n = np.full(S, NEG)
            for q in range(1, S):
                m = v[q]
                if q >= 2:
                    m = max(m, v[q - 1])
                if q % 2 == 1 and q >= 3 and labels[q >> 1] != labels[(q >> 1) - 1]:
                    m = max(m, v[q - 2])
                n[q] = m + d[t, cls[q]]
            v = n
            best[t] = max(best[t], v[S - 1])
    return best


def test_oracle_equals_brute_force_on_dyadic_inputs():
    T, C = 12, 5
    for n in range(30):
        seed = det.seed_of(f"kws.brute.{n}")
        e = -(det.randint((T, C), seed, 0, 24).astype(np.float32)) / np.float32(8)
        e[np.arange(T), det.randint((T,), seed + 1, 0, C)] = 0           # the best class of most frames is 0 (d = e); d is dyadic always
        if n % 5 == 0:
            e[det.randint((3,), seed + 2, 0, T), det.randint((3,), seed + 3, 1, C)] = NEG
        U = 1 + n % 3
        labels = [int(c) for c in det.randint((U,), seed + 4, 1, C)]
        score, start = K.kws_frames(e, labels)
        d = e.astype(np.float64) - e.astype(np.float64).max(1, keepdims=True)
        want = brute_scores(d, labels)
        assert np.array_equal(score.astype(np.float64), want), (n, labels, score, want)
        assert np.array_equal(start >= 0, np.isfinite(score)) and (start <= np.arange(T)).all()
        # a start is the start of a path with that value: the plain Viterbi from that frame alone reaches it
        for t in np.flatnonzero(start >= 0):
            s = start[t]
            assert brute_scores(np.concatenate((np.full((s, C), NEG), d[s:])), labels)[t] == score[t]


# ---- (b) the tie rules -----------------------------------------------------------------------------------------------------------
def test_enter_loses_a_tie_with_stay():
    score, start = K.kws_frames(P.tie_e(P.TIE_ENTER), P.TIE_ENTER["labels"])
    assert score.tolist() == [0.0, 0.0, -0.25] and start.tolist() == [0, 0, 0]


@pytest.mark.parametrize("tie,moves", [(P.TIE_STAY_STEP, (0, 1)), (P.TIE_STEP_SKIP, (1, 2))])
def test_smaller_move_wins_a_tie(tie, moves):
    V, S = K.kws_lattice(P.tie_e(tie), tie["labels"])
    t, q = tie["t"], 2 * len(tie["labels"]) - 1
    a, b = V[t - 1][q - moves[0]], V[t - 1][q - moves[1]]
    allowed = (0, 1, 2) if tie["labels"][-1] != tie["labels"][-2] else (0, 1)
    assert set(moves) <= set(allowed) and np.isfinite(a) and a == b and all(V[t - 1][q - m] <= a for m in allowed)   # a real tie at the max
    assert (S[t - 1][q - moves[0]], S[t - 1][q - moves[1]]) == (tie["winner"], tie["loser"])
    assert S[t][q] == tie["winner"] and K.kws_frames(P.tie_e(tie), tie["labels"])[1][t] == tie["winner"]


# ---- (c) the pick ----------------------------------------------------------------------------------------------------------------
def test_pick_kills_overlaps_breaks_ties_and_counts():
    f = np.float32
    #               t: 0     1     2     3     4     5     6     7
    score = np.array([-1.0, -0.5, -0.5, NEG, -2.0, -0.25, -3.0, -0.25], f)
    start = np.array([0, 0, 2, -1, 4, 3, 6, 7], np.int32)
    hs, he, hv, n = K.kws_pick(score, start, f(-2.5), 4)
    # -0.25 twice: the smaller t (5, span [3, 5]) first, which kills 4; then 7; then -0.5 twice: t = 1 (span [0, 1]) kills 0; then 2
    assert n == 4 and hs.tolist() == [3, 7, 0, 2] and he.tolist() == [6, 8, 2, 3] and hv.tolist() == [-0.25, -0.25, -0.5, -0.5]
    hs, he, hv, n = K.kws_pick(score, start, f(-2.5), 3)                  # t = 2 is still live
    assert n == 4 and hs.tolist() == [3, 7, 0]
    hs, he, hv, n = K.kws_pick(score, start, f(-3.0), 6)                  # the threshold is inclusive; unused slots
    assert n == 5 and hs.tolist() == [3, 7, 0, 2, 6, -1] and he.tolist() == [6, 8, 2, 3, 7, -1] and hv[5] == NEG
    hs, he, hv, n = K.kws_pick(score, start, f(-0.1), 2)
    assert n == 0 and hs.tolist() == [-1, -1] and he.tolist() == [-1, -1] and (hv == NEG).all()
    assert K.kws_pick(np.full(4, NEG, f), np.full(4, -1, np.int32), f(NEG), 2)[3] == 0       # -inf is no candidate, whatever the threshold


# ---- (d) planted keywords --------------------------------------------------------------------------------------------------------
def test_planted_keywords_are_found_and_absent_ones_are_not():
    p, kws, thr = P.planted_three()
    assert thr.tolist() == [np.float32(4 * math.log(0.5)), np.float32(3 * math.log(0.5))]
    fs, fst, hs, he, hv, nh = P.batch32(P.as_log32(p), None, kws, thr, 8)
    assert nh.tolist() == [[3, 0]]
    assert hs[0, 0, :3].tolist() == [10, 50, 90] and he[0, 0, :3].tolist() == [15, 55, 95] and (hv[0, 0, :3] == 0).all()
    assert (hs[0, 0, 3:] == -1).all() and (hs[0, 1] == -1).all() and (hv[0, 1] == NEG).all()
    assert -17.0 < fs[0, 1].max() < -16.0 and thr[1] > -2.1               # 3 log((0.1 / 28) / 0.9) = -16.6 against -2.08


def test_five_plants_fill_the_slots_and_a_threshold_excludes_two():
    p, kws = P.planted_five()
    x = P.as_log32(p)
    fs, fst, hs, he, hv, nh = P.batch32(x, None, kws, P.thr_of(kws, 0.02), 3)
    assert nh.tolist() == [[4]] and hs[0, 0].tolist() == [20, 140, 60] and he[0, 0].tolist() == [23, 143, 63]
    fs, fst, hs, he, hv, nh = P.batch32(x, None, kws, P.thr_of(kws, 0.02), 8)
    assert nh.tolist() == [[5]] and hs[0, 0, :5].tolist() == [20, 140, 60, 100, 180]
    fs, fst, hs, he, hv, nh = P.batch32(x, None, kws, P.thr_of(kws, 0.5), 8)
    assert nh.tolist() == [[3]] and hs[0, 0, :3].tolist() == [20, 140, 60]
    assert np.allclose(hv[0, 0, :3], [0.0, 0.0, 3 * math.log(0.8)], atol=1e-5)


def test_planted_problems_keep_their_margins_for_probability_input():
    """What the probability-input GPU tests rely on: every accepted score is more than 2 tol away from the threshold and from every
    candidate it killed, and every frame that is no candidate is more than 2 tol below the threshold (float64 oracle on the logs)."""
    for (p, kws, thr), max_hits in ((P.planted_three(), 8), (P.planted_five() + (P.thr_of(P.planted_five()[1], 0.5),), 8),
                                    (P.planted_five() + (P.thr_of(P.planted_five()[1], 0.02),), 3)):
        x = p.astype(np.float32)
        M = np.abs(np.log(x.astype(np.float64))).max()
        fs, fst, hs, he, hv, nh = K.kws_batch(x, None, kws, thr, max_hits, False, np.float64)
        for k in range(len(kws)):
            tol_all = P.prob_tol(int((np.arange(x.shape[1]) + 1 - fst[0, k])[fst[0, k] >= 0].max(initial=1)), M)
            finite = np.isfinite(fs[0, k])
            assert (np.abs(fs[0, k][finite] - thr[k]) > 2 * tol_all).all()
            for h in range(min(int(nh[0, k]), max_hits)):
                s, t = hs[0, k, h], he[0, k, h] - 1
                rivals = [i for i in np.flatnonzero(finite & (fs[0, k] >= thr[k])) if i != t and fst[0, k, i] <= t and s <= i]
                assert all(hv[0, k, h] - fs[0, k, i] > 2 * tol_all for i in rivals), (k, h, rivals)
            # two accepted hits with scores closer than 2 tol must not depend on their order: they do not overlap
            acc = [(hs[0, k, h], he[0, k, h]) for h in range(min(int(nh[0, k]), max_hits))]
            assert all(a[1] <= b[0] or b[1] <= a[0] for i, a in enumerate(acc) for b in acc[i + 1:])


# ---- (e) KeywordSpotter's host logic ---------------------------------------------------------------------------------------------
LABELS = "_'abcdefghijklmnopqrstuvwxyz "


def test_spotter_encodes_keywords_and_thresholds():
    from asr_amd import KeywordSpotter
    sp = KeywordSpotter(LABELS, ["cat", "a b"], threshold=0.25, max_hits=5)
    assert sp.kw_ids == [[4, 2, 21], [2, 28, 3]] and sp.kw_lens == [3, 3] and sp.max_hits == 5
    assert sp.thr.dtype == np.float32 and sp.thr.tolist() == [np.float32(3 * math.log(0.25))] * 2
    sp.set_keywords(["it's"])
    assert sp.kw_ids == [[10, 21, 1, 20]] and sp.threshold == 0.25 and sp.thr.tolist() == [np.float32(4 * math.log(0.25))]
    sp.set_keywords(["z" * 63], threshold=1.0)
    assert sp.thr.tolist() == [0.0] and sp.kw_lens == [63]
    assert KeywordSpotter({c: i for i, c in enumerate(LABELS)}, ["hi"]).threshold == 0.5


@pytest.mark.parametrize("keywords,threshold,max_hits,match", [
    (["cat", ""], 0.5, 32, "empty"), (["cat", "dog", "cat"], 0.5, 32, "duplicate"), (["z" * 64], 0.5, 32, "63"), (["c4t"], 0.5, 32, "'4'"),
    ([], 0.5, 32, "no keyword"), ("cat", 0.5, 32, "list"), (["a_b"], 0.5, 32, "blank"), (["cat"], 0.0, 32, "threshold"),
    (["cat"], 1.5, 32, "threshold"), (["cat"], float("nan"), 32, "threshold"), (["cat"], 0.5, 0, "max_hits"), (["cat"], 0.5, 1025, "max_hits")])
def test_spotter_refusals(keywords, threshold, max_hits, match):
    from asr_amd import KeywordSpotter
    with pytest.raises(ValueError, match=match):
        KeywordSpotter(LABELS, keywords, threshold=threshold, max_hits=max_hits)


def test_spotter_keeps_its_keywords_on_a_refusal():
    from asr_amd import KeywordSpotter
    sp = KeywordSpotter(LABELS, ["cat"])
    with pytest.raises(ValueError):
        sp.set_keywords(["dog", ""])
    with pytest.raises(ValueError):
        KeywordSpotter(LABELS, ["cat"], blank_index=1)
    assert sp.keywords == ["cat"] and sp.kw_ids == [[4, 2, 21]]


def test_detections_are_assembled_sorted_with_confidence_and_seconds():
    from asr_amd.decoders import add_seconds, assemble_detections
    hs = np.array([[[30, 5, -1], [7, -1, -1]], [[-1, -1, -1], [1, 2, 3]]], np.int32)
    he = np.array([[[34, 9, -1], [9, -1, -1]], [[-1, -1, -1], [2, 3, 4]]], np.int32)
    hv = np.array([[[0.0, -1.5, NEG], [-0.5, NEG, NEG]], [[NEG, NEG, NEG], [-0.25, -0.25, -0.25]]], np.float32)
    nh = np.array([[2, 1], [0, 4]], np.int32)
    recs, over = assemble_detections(hs, he, hv, nh, ["cat", "at"], [3, 2], 3)
    assert over == [(1, "at")]
    assert [(r["keyword"], r["start"], r["end"], r["score"]) for r in recs[0]] == [("cat", 5, 9, -1.5), ("at", 7, 9, -0.5), ("cat", 30, 34, 0.0)]
    assert [r["confidence"] for r in recs[0]] == [math.exp(-0.5), math.exp(-0.25), 1.0]
    assert [(r["start"], r["end"]) for r in recs[1]] == [(1, 2), (2, 3), (3, 4)]
    out = add_seconds(recs, 0.02)
    assert out is recs and recs[0][0]["start_s"] == 5 * 0.02 and recs[0][0]["end_s"] == 9 * 0.02 and "start_s" in recs[1][2]


class _Recorder:
    """Stands in for asr_amd.ops: records what KeywordSpotter.search hands to the op and returns two hits for the first keyword."""

    def rnn_poison_seen(self, dev):
        return False

    def ctc_keyword_search(self, x, kw_labels, kw_off, kw_lens, max_kw_len, thr, in_lens, is_log, max_hits):
        self.call = (kw_labels.tolist(), kw_off.tolist(), kw_lens.tolist(), max_kw_len, thr.tolist(), in_lens.tolist(), is_log, max_hits)
        B, Kn = x.shape[0], kw_lens.numel()
        hs = torch.full((B, Kn, max_hits), -1, dtype=torch.int32)
        he, hv, nh = hs.clone(), torch.full((B, Kn, max_hits), float("-inf")), torch.zeros((B, Kn), dtype=torch.int32)
        hs[:, 0, :2], he[:, 0, :2], hv[:, 0, :2] = torch.tensor([6, 1]), torch.tensor([8, 4]), torch.tensor([0.0, -1.0])
        nh[:, 0] = max_hits + 1
        return None, None, hs, he, hv, nh


def test_spotter_packs_one_image_and_warns_on_overflow(monkeypatch):
    import asr_amd
    from asr_amd import decoders
    rec = _Recorder()
    monkeypatch.setattr(asr_amd, "ops", rec, raising=False)
    monkeypatch.setattr(decoders, "_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **{kk: v for kk, v in k.items() if kk != "pin_memory"}))
    sp = decoders.KeywordSpotter(LABELS, ["cat", "to"], threshold=0.5, max_hits=2)
    with pytest.warns(RuntimeWarning, match="max_hits=2"):
        recs = sp.search(torch.full((2, 9, 29), 1 / 29), [9, 40], frame_seconds=0.02)
    lab, off, lens, max_u, thr, in_lens, is_log, max_hits = rec.call
    assert lab == [4, 2, 21, 21, 16] and off == [0, 3] and lens == [3, 2] and max_u == 3 and in_lens == [9, 9] and not is_log and max_hits == 2
    assert thr == [np.float32(3 * math.log(0.5)), np.float32(2 * math.log(0.5))]
    assert [[(r["keyword"], r["start"], r["end"], r["start_s"]) for r in u] for u in recs] == [[("cat", 1, 4, 0.02), ("cat", 6, 8, 0.12)]] * 2
    with pytest.raises(ValueError, match="sizes"):
        sp.search(torch.full((2, 9, 29), 1 / 29), [9])


def test_model_methods_exist_with_their_defaults():
    import inspect
    from asr_amd import DeepSpeech
    sig = inspect.signature(DeepSpeech.spot).parameters
    assert list(sig) == ["self", "inputs", "input_sizes", "keywords", "threshold", "max_hits"] and sig["threshold"].default == 0.5
    sig = inspect.signature(DeepSpeech.spot_long).parameters
    assert list(sig)[:6] == ["self", "spect", "keywords", "window", "overlap", "batch_size"]
    assert (sig["window"].default, sig["overlap"].default, sig["batch_size"].default, sig["max_hits"].default) == (2000, 200, 32, 32)


# ---- (f) the entry points --------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_sized():
    from asr_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in ("ds2_ctc_kws_f32", "ds2_ctc_kws_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_ctc_kws_f32"][1]) == 24
    assert lib.ds2_ctc_kws_workspace_bytes(4, 37, 6, 32) == 4 * 4 * 37 * 7
    assert lib.ds2_ctc_kws_workspace_bytes(1, 180000, 16, 1024) == 4 * 180000 * 17         # no term in T x states: an hour is 12 MB
    assert lib.ds2_ctc_kws_workspace_bytes(64, 3000000, 128, 1) == 4 * 64 * 3000000 * 129  # sized in 64 bits
    for bad in ((0, 5, 1, 1), (1, 0, 1, 1), (1, 5, 0, 1), (1, 5, 1, 0), (1, 5, 1, 1025), (-1, 5, 1, 1)):
        assert lib.ds2_ctc_kws_workspace_bytes(*bad) == 0, bad


def test_entry_rejects_bad_arguments_before_any_launch():
    from asr_amd import _lib
    lib = _lib.load()
    p = 4096                                                           # any non-null address: every call below returns before a launch
    need = lib.ds2_ctc_kws_workspace_bytes(2, 10, 3, 4)
    ok = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, in_lens=None, labels=p, off=p, lens=p, K=3, max_u=5, thr=p, max_hits=4,
              fs=p, fst=p, hs=p, he=p, hv=p, nh=p, ws=p, wsb=need, stream=None)
    for bad in (dict(x=None), dict(labels=None), dict(off=None), dict(lens=None), dict(thr=None), dict(fs=None), dict(fst=None), dict(hs=None),
                dict(he=None), dict(hv=None), dict(nh=None), dict(ws=None), dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(C=0), dict(K=0),
                dict(K=-1), dict(ld_b=0), dict(ld_t=0), dict(is_log=2), dict(is_log=-1), dict(max_u=64), dict(max_u=-1), dict(max_hits=0),
                dict(max_hits=1025), dict(wsb=need - 1), dict(wsb=0), dict(B=1 << 20, K=1 << 12)):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_kws_f32(*a.values()) != 0, bad
        assert lib.ds2_last_error().startswith(b"ds2_ctc_kws_f32: "), (bad, lib.ds2_last_error())
    assert b"max_kw_len" in (lib.ds2_ctc_kws_f32(*dict(ok, max_u=64).values()), lib.ds2_last_error())[1]
    assert b"workspace too small" in (lib.ds2_ctc_kws_f32(*dict(ok, wsb=need - 1).values()), lib.ds2_last_error())[1]


def test_op_refuses_on_the_host():
    from asr_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    x = torch.zeros((1, 4, 5))
    with pytest.raises(ValueError, match="GPU"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, torch.zeros(1))
    with pytest.raises(ValueError, match="max_kw_len"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 64, torch.zeros(1))
    for mh in (0, 1025):
        with pytest.raises(ValueError):
            ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, torch.zeros(1), max_hits=mh)
