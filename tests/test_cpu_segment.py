"""CPU: the pause-segmentation contract (include/ds2hip.h, ds2_ctc_segment_f32 / ds2_ctc_segment_gather_f32) as
tests/ctc_segment_oracle.py restates it — brute-force properties on random problems, the greedy equivalence — and the host half:
plan_segment_batches, words_from_offsets, assemble_transcript, the ctypes signatures and the argument checks of the entries, none of
which needs a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ctc_segment_oracle as O
import segment_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM, N_FORCED = 300, 40


# ---- (a) the oracle against brute-force properties -------------------------------------------------------------------------------
def check_properties(x, thr, min_gap, pad, max_len, segs, what):
    col = x[:, 0]
    Tb = len(col)
    silent = col >= np.float32(thr)
    half = (max_len + 1) // 2
    covered = np.zeros(Tb, np.int64)
    prev_end, prev_flag = 0, 0
    for s, e, f in segs:
        assert prev_end <= s < e <= Tb, (what, "ascending, disjoint, inside [0, T_b)", s, e)
        assert 1 <= e - s <= max_len, (what, "length", s, e)
        covered[s:e] += 1
        if f & 2:
            assert e - s >= half, (what, "a piece that ends at a forced cut has (max_len + 1) // 2 frames", s, e)
        if f & 1:
            assert prev_flag & 2 and prev_end == s, (what, "a bit-0 flag follows a bit-1 flag", s)
        if prev_flag & 2:
            assert f & 1 and prev_end == s, (what, "a bit-1 flag is followed by a bit-0 flag", s)
        assert f in (0, 1, 2, 3)
        prev_end, prev_flag = e, f
    assert not prev_flag & 2, what
    assert (covered[~silent] == 1).all(), (what, "every non-silent frame lies in exactly one segment")
    assert silent[covered == 0].all(), (what, "every frame outside all segments is silent")
    assert covered.max(initial=0) <= 1


def test_oracle_keeps_the_invariants_on_random_problems():
    n_forced = 0
    for n in range(N_RANDOM):
        p = P.random_problem(n)
        segs = O.segment_one(p["x"][:, 0], np.float32(p["thr"]), p["min_gap"], p["pad"], p["max_len"])
        check_properties(p["x"], p["thr"], p["min_gap"], p["pad"], p["max_len"], segs, n)
        n_forced += any(f for _, _, f in segs)
    assert n_forced >= N_RANDOM // 10                                     # the random problems do reach the forced cuts


def test_pauses_are_what_the_text_says():
    sil = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1], bool)              # runs: [0,1) [2,4) [5,8) [10,11)
    assert O.silent_runs(sil) == [(0, 1), (2, 4), (5, 8), (10, 11)]
    assert O.pauses_of(sil, 3) == [(0, 1), (5, 8), (10, 11)]              # the ends at any length, inside only min_gap frames
    assert [r[:2] for r in O.regions_of(O.pauses_of(sil, 3), 11)] == [(1, 5), (8, 10)]
    col = np.where(sil, 0.95, 0.1).astype(np.float32)
    # pad 2: the first region may not enter the pause that starts at 0 beyond frame 0 and stops at m(5, 8) = 6; the second at 6 and T_b
    assert O.segment_one(col, 0.9, 3, 2, 100) == [(0, 6, 0), (6, 11, 0)]
    assert O.segment_one(col, 0.9, 3, 0, 100) == [(1, 5, 0), (8, 10, 0)]
    assert O.segment_one(col, 0.9, 1, 0, 100) == [(1, 2, 0), (4, 5, 0), (8, 10, 0)]
    assert O.segment_one(np.full(9, 0.95, np.float32), 0.9, 3, 2, 100) == [] and O.segment_one(np.zeros(0, np.float32), 0.9, 3, 2, 100) == []
    assert O.segment_one(np.array([np.nan, 0.1, np.nan], np.float32), 0.9, 1, 0, 100) == [(0, 3, 0)]        # NaN is not silent


def test_forced_cut_takes_the_smallest_frame_of_a_tie():
    col = np.full(20, 0.1, np.float32)
    col[[5, 7]] = 0.3
    assert O.segment_one(col, 0.9, 3, 0, 8) == [(0, 5, 2), (5, 9, 3), (9, 13, 3), (13, 20, 1)]
    assert O.segment_one(col, 0.9, 3, 0, 7) == [(0, 5, 2), (5, 9, 3), (9, 13, 3), (13, 20, 1)]              # windows [4,7] [9,12] [13,16]


# ---- (b) the greedy equivalence --------------------------------------------------------------------------------------------------
def cuts_meet_the_condition(x, segs):
    best = np.argmax(x, axis=1)
    return all(best[s] == 0 or best[s] != best[s - 1] for s, _, f in segs if f & 1)


def assert_greedy_equivalence(x, segs, what):
    ids, offs = [], []
    for s, e, _ in segs:
        i, o = O.greedy(x[s:e])
        ids += i
        offs += [s + t for t in o]
    assert (ids, offs) == O.greedy(x), what


def test_segmentwise_greedy_decode_equals_the_whole_decode():
    """Probability input, threshold > 0.5, every forced cut frame with the blank as its best class or another best class than the frame
    before it: the per-segment greedy decodes, concatenated, are the greedy decode of the whole utterance."""
    held = forced = 0
    for n in range(N_RANDOM):
        p = P.random_problem(n)
        segs = O.segment_one(p["x"][:, 0], np.float32(p["thr"]), p["min_gap"], p["pad"], p["max_len"])
        if cuts_meet_the_condition(p["x"], segs):
            assert_greedy_equivalence(p["x"], segs, n)
            held += 1
    for n in range(N_FORCED):
        p = P.forced_problem(n)
        segs = O.segment_one(p["x"][:, 0], np.float32(p["thr"]), p["min_gap"], p["pad"], p["max_len"])
        check_properties(p["x"], p["thr"], p["min_gap"], p["pad"], p["max_len"], segs, ("forced", n))
        assert cuts_meet_the_condition(p["x"], segs), ("the forced problems are built to meet the condition", n)
        assert_greedy_equivalence(p["x"], segs, ("forced", n))
        forced += any(f for _, _, f in segs)
    assert held >= N_RANDOM // 3 and forced == N_FORCED                   # every forced problem has a forced cut


def test_pipeline_problem_is_a_dozen_mixed_segments_that_decode_to_the_phrases():
    x, _ = P.pipeline_problem()
    segs = O.segment_one(x[:, 0], np.float32(P.PIPE["thr"]), P.PIPE["min_gap"], P.PIPE["pad"], P.PIPE["max_len"])
    assert 500 <= len(x) <= 700 and len(segs) >= 12 and any(f for _, _, f in segs)
    assert len({e - s for s, e, _ in segs}) >= 6
    assert cuts_meet_the_condition(x, segs)
    assert_greedy_equivalence(x, segs, "pipeline")
    ids, _ = O.greedy(x)
    assert "".join(P.LABELS[i] for i in ids) == "".join(P.PHRASES)        # (a pause emits no space: the phrases run together)


def test_gpu_cases_keep_the_invariants_and_report_the_full_count():
    cases = P.gpu_cases()
    for name, c in cases.items():
        if c["is_log"] or c["blank"] != 0 or name == "overflow":
            continue
        start, end, flags, n = c["want"]
        for b in range(3):
            Tb = c["x"].shape[1] if c["in_lens"] is None else c["in_lens"][b]
            assert n[b] <= c["max_segs"]
            segs = [(int(start[b, i]), int(end[b, i]), int(flags[b, i])) for i in range(n[b])]
            check_properties(c["x"][b, :Tb], c["thr"], c["min_gap"], c["pad"], c["max_len"], segs, (name, b))
            assert (start[b, n[b]:] == -1).all() and (end[b, n[b]:] == -1).all() and (flags[b, n[b]:] == 0).all()
    over, full = cases["overflow"], cases["random.257"]
    assert np.array_equal(over["want"][3], full["want"][3]) and over["want"][3].max() == over["max_segs"] + 3
    assert np.array_equal(over["want"][0], full["want"][0][:, :over["max_segs"]])
    assert cases["ragged.257"]["want"][3][2] == 0 and cases["edges.257"]["want"][3][1] == 0              # in_lens 0; all silent
    assert any(c["want"][2].any() for c in cases.values())


def test_gather_oracle_rejects_and_pads():
    x = np.arange(2 * 7 * 3, dtype=np.float32).reshape(2, 7, 3) + 1
    out, sizes = O.gather(x, [1, 0, 2, 0, 0, 0, 0, -1], [2, 0, 0, -1, 3, 5, 0, 0], [4, 7, 1, 2, -1, 3, 8, 1], 7)
    assert sizes.tolist() == [4, 7, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(out[0, :4], x[1, 2:6]) and not out[0, 4:].any() and np.array_equal(out[1], x[0]) and not out[2:].any()
    assert O.gather(x, [0], [0], [5], 4)[1].tolist() == [0]              # longer than t_max


# ---- (c) the host functions ------------------------------------------------------------------------------------------------------
def test_plan_segment_batches_is_a_longest_first_permutation_in_bounded_batches():
    from asr_amd.decoders import plan_segment_batches
    lengths = [5, 9, 5, 1, 30, 9, 2]
    batches = plan_segment_batches(lengths, 3)
    assert batches == [[4, 1, 5], [0, 2, 6], [3]]
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(7)) and all(1 <= len(b) <= 3 for b in batches)
    assert [lengths[i] for i in flat] == sorted(lengths, reverse=True)
    assert all(lengths[b[0]] == max(lengths[i] for i in b) for b in batches)
    assert plan_segment_batches([], 4) == [] and plan_segment_batches(np.array([3, 4], np.int32), 64) == [[1, 0]]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            plan_segment_batches(lengths, bad)


def test_words_from_offsets():
    from asr_amd.decoders import words_from_offsets
    assert words_from_offsets("", []) == []
    assert words_from_offsets("   ", [1, 2, 3]) == []
    text = " the  cat sat "
    offs = [0, 2, 3, 5, 7, 8, 10, 11, 14, 15, 17, 18, 20, 21]
    assert words_from_offsets(text, offs) == [("the", 2, 6), ("cat", 10, 15), ("sat", 17, 21)]
    assert words_from_offsets(text, torch.tensor(offs, dtype=torch.int), shift=100) == [("the", 102, 106), ("cat", 110, 115), ("sat", 117, 121)]
    assert words_from_offsets("a", [4]) == [("a", 4, 5)]
    with pytest.raises(ValueError, match="offsets"):
        words_from_offsets("ab", [1])
    assert "not spans" in inspect.getdoc(words_from_offsets) and "align()" in inspect.getdoc(words_from_offsets)


def test_assemble_transcript_restores_time_order():
    from asr_amd.decoders import assemble_transcript, plan_segment_batches
    start, end, flags = np.array([4, 20, 50, 58], np.int32), np.array([10, 31, 58, 60], np.int32), np.array([0, 0, 2, 1], np.int32)
    by_time = [("hi ", [1, 2, 4]), ("big  cat", [0, 1, 2, 4, 5, 7, 8, 9]), ("", []), (" x", [0, 1])]
    order = [i for b in plan_segment_batches(end - start, 3) for i in b]
    assert order == [1, 2, 0, 3]
    texts, offs = [by_time[i][0] for i in order], [torch.tensor(by_time[i][1], dtype=torch.int) for i in order]
    rec = assemble_transcript(texts, offs, start, end, flags, order, scores=[-1.0, -2.0, -0.0, -3.0], frame_seconds=0.02)
    assert rec["text"] == "hi big  cat x"
    assert [(s["start"], s["end"], s["text"], s["forced"], s["score"]) for s in rec["segments"]] == \
        [(4, 10, "hi ", 0, -0.0), (20, 31, "big  cat", 0, -1.0), (50, 58, "", 2, -2.0), (58, 60, " x", 1, -3.0)]
    assert rec["segments"][1]["words"] == [("big", 20, 23, 20 * 0.02, 23 * 0.02), ("cat", 27, 30, 27 * 0.02, 30 * 0.02)]
    assert rec["segments"][3]["words"] == [("x", 59, 60, 59 * 0.02, 60 * 0.02)] and rec["segments"][2]["words"] == []
    assert (rec["segments"][0]["start_s"], rec["segments"][0]["end_s"]) == (4 * 0.02, 10 * 0.02)
    plain = assemble_transcript(texts, offs, start, end, flags, order)
    assert "score" not in plain["segments"][0] and "start_s" not in plain["segments"][0] and plain["segments"][1]["words"][0] == ("big", 20, 23)
    assert set(rec["segments"][0]) == {"start", "end", "start_s", "end_s", "text", "words", "forced", "score"}
    assert assemble_transcript([], [], start[:0], end[:0], flags[:0], []) == {"text": "", "segments": []}
    with pytest.raises(ValueError):
        assemble_transcript(texts, offs, start, end, flags, [0, 1, 2, 2])


def test_model_methods_exist_with_their_defaults():
    from asr_amd import DeepSpeech
    sig = inspect.signature(DeepSpeech.transcribe).parameters
    assert list(sig) == ["self", "inputs", "input_sizes", "decoder"] and sig["decoder"].default is None
    sig = inspect.signature(DeepSpeech.transcribe_long).parameters
    assert list(sig) == ["self", "spect", "window", "overlap", "batch_size", "decoder", "threshold", "min_gap", "pad", "max_len", "decode_batch"]
    assert [sig[k].default for k in list(sig)[2:]] == [2000, 200, 32, None, 0.9, 25, 5, 1000, 64]
    doc = inspect.getdoc(DeepSpeech.transcribe_long)
    assert "unmeasured" in doc and "<s>" in doc


def test_segment_options_are_checked():
    from asr_amd.decoders import check_segment_options
    check_segment_options("t", 0.9, 25, 5, 1000, 64)
    for bad in (dict(threshold=0.0), dict(threshold=1.5), dict(threshold=float("nan")), dict(min_gap=0), dict(pad=-1), dict(max_len=1),
                dict(decode_batch=0), dict(min_gap=2.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            check_segment_options("t", **dict(dict(threshold=0.9, min_gap=25, pad=5, max_len=1000, decode_batch=64), **bad))


# ---- (d) the entry points --------------------------------------------------------------------------------------------------------
NAMES = ("ds2_ctc_segment_f32", "ds2_ctc_segment_gather_f32", "ds2_ctc_segment_workspace_bytes")


def test_entries_are_declared_exported_and_sized():
    from asr_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_ctc_segment_f32"][1]) == 20 and len(_lib.SIGNATURES["ds2_ctc_segment_gather_f32"][1]) == 14
    size = lambda B, T: B * (8 * ((T + 63) // 64) + 4 * (4 * (T // 2 + 1) + T))
    for B, T in ((1, 1), (3, 257), (1, 180000), (64, 3000000)):        # host-known sizes only; an hour is 2.2 MB; sized in 64 bits
        assert lib.ds2_ctc_segment_workspace_bytes(B, T) == size(B, T)
    assert size(1, 180000) < 2.5e6
    for bad in ((0, 5), (1, 0), (-1, 5)):
        assert lib.ds2_ctc_segment_workspace_bytes(*bad) == 0, bad


def test_segment_entry_rejects_bad_arguments_before_any_launch():
    from asr_amd import _lib
    lib = _lib.load()
    p = 4096                                                           # any non-null address: every call below returns before a launch
    need = lib.ds2_ctc_segment_workspace_bytes(2, 100)
    ok = dict(x=p, ld_b=1000, ld_t=10, B=2, T=100, C=10, in_lens=None, blank=0, thr=0.9, min_gap=25, pad=5, max_len=1000, max_segs=8,
              ss=p, se=p, sf=p, ns=p, ws=p, wsb=need, stream=None)
    for bad in (dict(min_gap=0), dict(max_len=1), dict(blank=10), dict(max_segs=0), dict(wsb=need - 1), dict(wsb=0), dict(ws=None),
                dict(x=None), dict(ss=None), dict(se=None), dict(sf=None), dict(ns=None), dict(B=0), dict(T=0), dict(T=-2), dict(C=0),
                dict(ld_b=0), dict(ld_t=0), dict(blank=-1), dict(pad=-1), dict(min_gap=-3), dict(max_segs=-1), dict(ws=p + 4)):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_segment_f32(*a.values()) != 0, bad
        assert lib.ds2_last_error().startswith(b"ds2_ctc_segment_f32: "), (bad, lib.ds2_last_error())
    for bad, word in ((dict(min_gap=0), b"min_gap"), (dict(max_len=1), b"max_len"), (dict(blank=10), b"blank"), (dict(max_segs=0), b"max_segs"),
                      (dict(wsb=need - 1), b"workspace too small")):
        assert word in (lib.ds2_ctc_segment_f32(*dict(ok, **bad).values()), lib.ds2_last_error())[1]


def test_gather_entry_rejects_bad_arguments_before_the_launch():
    from asr_amd import _lib
    lib = _lib.load()
    p = 4096
    ok = dict(x=p, ld_b=1000, ld_t=10, B=2, T=100, C=10, sb=p, ss=p, sl=p, S=3, T_max=40, out=p, sizes=p, stream=None)
    for bad in (dict(x=None), dict(sb=None), dict(ss=None), dict(sl=None), dict(out=None), dict(sizes=None), dict(B=0), dict(T=0), dict(C=0),
                dict(ld_b=0), dict(ld_t=0), dict(S=0), dict(S=-1), dict(T_max=0), dict(S=1 << 30, T_max=1 << 20)):
        assert lib.ds2_ctc_segment_gather_f32(*dict(ok, **bad).values()) != 0, bad
        assert lib.ds2_last_error().startswith(b"ds2_ctc_segment_gather_f32: "), (bad, lib.ds2_last_error())


def test_ops_refuse_on_the_host():
    from asr_amd import ops
    x = torch.full((1, 40, 5), 0.2)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.ctc_segment(x)
    for bad in (dict(min_gap=0), dict(pad=-1), dict(max_len=1), dict(threshold=0.0), dict(threshold=1.01)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ops.ctc_segment(x, **bad)
    with pytest.raises(ValueError, match="GPU"):
        ops.ctc_segment_gather(x, i32(0), i32(0), i32(4), 4)
    with pytest.raises(ValueError, match="t_max"):
        ops.ctc_segment_gather(x, i32(0), i32(0), i32(4), 0)
    assert ops.segment_max_segs(180000, 25, 1000) == (180000 + 25) // 26 + 180000 // 500
    assert ops.segment_max_segs(1, 1, 2) == 2
