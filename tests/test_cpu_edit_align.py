"""No GPU: the plain-Python restatement of the edit alignment (tests/edit_align_oracle.py) against the host DP and a brute-force
enumeration; hand-made ties that pin the rule; the host half of Decoder.align_batch (assemble_edit_alignments), ErrorReport and
reliability; the ABI of ds2_edit_align_* and what ops.edit_align refuses before any HIP call."""
import inspect
import math
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import edit_align_oracle as O
from asr_amd import _lib, ops
from asr_amd.decoders import ErrorReport, _edit_distance, assemble_edit_alignments, pack_scoring, reliability
from asr_amd.modules.deepspeech import DeepSpeech


def _pairs(seed, alphabets=(2, 30), max_len=12, count=150):
    rng = random.Random(seed)
    return [([rng.randrange(k) for _ in range(rng.randrange(max_len + 1))], [rng.randrange(k) for _ in range(rng.randrange(max_len + 1))])
            for k in alphabets for _ in range(count)]


def test_oracle_counts_and_maps():
    for a, b in _pairs(1):
        (hits, subs, dels, ins), a_map, b_map = O.align(a, b)
        assert subs + dels + ins == _edit_distance(a, b)
        assert hits + subs + ins == len(a) and hits + subs + dels == len(b)
        assert len(a_map) == len(a) and len(b_map) == len(b)
        pairs = [(i, j) for i, j in enumerate(a_map) if j >= 0]
        assert pairs == [(i, j) for j, i in enumerate(b_map) if i >= 0]            # mutually inverse
        assert all(p[0] < q[0] and p[1] < q[1] for p, q in zip(pairs, pairs[1:]))  # strictly increasing on both sides
        assert sum(a[i] == b[j] for i, j in pairs) == hits and len(pairs) == hits + subs


def _cheapest(a, b):
    """the cost of the cheapest of ALL alignments (every monotone set of pairs), by enumeration"""
    def go(i, j):
        if i == len(a):
            return len(b) - j
        if j == len(b):
            return len(a) - i
        return min(go(i + 1, j + 1) + (a[i] != b[j]), go(i + 1, j) + 1, go(i, j + 1) + 1)
    return go(0, 0)


def test_oracle_is_optimal_by_brute_force():
    n = 0
    for a, b in _pairs(2, max_len=5, count=200):
        if len(a) + len(b) <= 8:
            (_, subs, dels, ins), _, _ = O.align(a, b)
            assert subs + dels + ins == _cheapest(a, b)
            n += 1
    assert n > 100


def test_hand_made_ties_pin_the_rule():
    # option 1 (pair) before option 2 (delete): the LAST of equal reference symbols takes the hypothesis symbol
    assert O.align([0], [0, 0]) == ((1, 0, 1, 0), [1], [-1, 0])
    # ... and mirrored: the last of equal hypothesis symbols is paired, the first is an insertion
    assert O.align([0, 0], [0]) == ((1, 0, 0, 1), [-1, 0], [1])
    # option 2 (delete) before option 3 (insert): at (3, 3) no pairing is optimal, and both D[3][2] + 1 and D[2][3] + 1 equal D[3][3] = 2.
    # The rule deletes b[2] and ends with the insertion of a[0]; insertion first would give a_map [0, 1, -1], b_map [-1, 0, 1]
    assert O.align([0, 1, 0], [1, 0, 1]) == ((2, 0, 1, 1), [-1, 0, 1], [1, 2, -1])
    assert O.align([1, 0, 1], [0, 1, 0]) == ((2, 0, 1, 1), [-1, 0, 1], [1, 2, -1])
    # one substitution beats a deletion plus an insertion
    assert O.align([1], [2]) == ((0, 1, 0, 0), [0], [0])
    # where pairing the last symbols is not optimal, the unpaired symbol is at the end
    assert O.align([0, 1], [1]) == ((1, 0, 0, 1), [-1, 0], [1])
    assert O.align([1, 0], [1]) == ((1, 0, 0, 1), [0, -1], [0])
    assert O.align([1], [1, 0]) == ((1, 0, 1, 0), [0], [0, -1])
    assert O.align([], [5, 6]) == ((0, 0, 2, 0), [], [-1, -1])
    assert O.align([5, 6], []) == ((0, 0, 0, 2), [-1, -1], [])
    assert O.align([], []) == ((0, 0, 0, 0), [], [])
    assert O.align_padded([([0], [0, 0])], 3) == ([[1, 0, 1, 0]], [[1, -1, -1]], [[-1, 0, -1]])


def _oracle_arrays(hyps, refs):
    seq, a_off, a_len, b_off, b_len, _, _ = pack_scoring(hyps, refs)
    side = lambda off, ln, p: seq[off[p]:off[p] + ln[p]].tolist()   # noqa: E731
    pairs = [(side(a_off, a_len, p), side(b_off, b_len, p)) for p in range(len(a_off))]
    max_len = int(max(a_len.max(initial=0), b_len.max(initial=0)))
    return O.align_padded(pairs, max_len)


def test_assemble_edit_alignments():
    hyps = ["the cat sat", "", "a b", "x \U0001F600y", "same words"]
    refs = ["the bat sat down", "a b", "", "x \U0001F601y z", "same words"]
    recs = assemble_edit_alignments(hyps, refs, *_oracle_arrays(hyps, refs))
    assert len(recs) == 5 and all(set(r) == {"words", "chars"} for r in recs)
    w = recs[0]["words"]
    assert [o[0] for o in w["ops"]] == ["hit", "sub", "hit", "del"]
    assert w["ops"][1] == ("sub", "cat", "bat", 1, 1) and w["ops"][3] == ("del", None, "down", None, 3)
    assert (w["hits"], w["substitutions"], w["deletions"], w["insertions"], w["distance"], w["ref_len"]) == (2, 1, 1, 0, 2, 4)
    assert w["hyp_correct"] == [True, False, True]
    c = recs[0]["chars"]
    assert c["distance"] == _edit_distance("thecatsat", "thebatsatdown") and c["ref_len"] == 13 and len(c["hyp_correct"]) == 9
    assert c["hyp_correct"] == [True, True, True, False, True, True, True, True, True]
    # an empty hypothesis: all deletions; an empty reference: all insertions
    assert [o[0] for o in recs[1]["words"]["ops"]] == ["del", "del"] and recs[1]["words"]["hyp_correct"] == []
    assert recs[1]["chars"]["deletions"] == 2 and recs[1]["chars"]["ref_len"] == 2
    assert recs[2]["words"]["ops"] == [("ins", "a", None, 0, None), ("ins", "b", None, 1, None)]
    assert recs[2]["words"]["ref_len"] == 0 and recs[2]["words"]["hyp_correct"] == [False, False]
    # non-BMP characters are one token each
    c = recs[3]["chars"]
    assert ("sub", "\U0001F600", "\U0001F601", 1, 1) in c["ops"] and c["ops"][-1] == ("del", None, "z", None, 3)
    assert c["hyp_correct"] == [True, False, True]
    assert recs[4]["words"]["hyp_correct"] == [True, True] and recs[4]["chars"]["distance"] == 0
    # the units asked for
    only = assemble_edit_alignments(hyps, refs, *_oracle_arrays(hyps, refs), unit="word")
    assert all(set(r) == {"words"} for r in only) and only[0]["words"] == recs[0]["words"]
    only = assemble_edit_alignments(hyps, refs, *_oracle_arrays(hyps, refs), unit="char")
    assert all(set(r) == {"chars"} for r in only) and only[3]["chars"] == recs[3]["chars"]
    with pytest.raises(ValueError):
        assemble_edit_alignments(hyps, refs, *_oracle_arrays(hyps, refs), unit="phone")
    with pytest.raises(ValueError):
        assemble_edit_alignments(hyps, refs[:-1], *_oracle_arrays(hyps, refs))
    assert assemble_edit_alignments([], [], np.zeros((0, 4), np.int32), np.zeros((0, 0), np.int32), np.zeros((0, 0), np.int32)) == []


def test_assemble_on_random_strings_is_consistent():
    rng = random.Random(4)
    words = ["a", "bb", "a", "あ", "\U0001F600", "c"]
    hyps = [" ".join(rng.choice(words) for _ in range(rng.randrange(0, 9))) for _ in range(40)]
    refs = [" ".join(rng.choice(words) for _ in range(rng.randrange(0, 9))) for _ in range(40)]
    for h, r, rec in zip(hyps, refs, assemble_edit_alignments(hyps, refs, *_oracle_arrays(hyps, refs))):
        for key, hyp, ref in (("words", h.split(), r.split()), ("chars", list(h.replace(" ", "")), list(r.replace(" ", "")))):
            u = rec[key]
            assert u["distance"] == _edit_distance(hyp, ref) and u["ref_len"] == len(ref)
            assert [o[1] for o in u["ops"] if o[1] is not None] == hyp and [o[2] for o in u["ops"] if o[2] is not None] == ref
            assert u["hyp_correct"] == [o[0] == "hit" for o in u["ops"] if o[3] is not None]
            assert all((o[0] == "hit") == (o[1] == o[2]) for o in u["ops"] if o[0] in ("hit", "sub"))


def test_error_report():
    hyps1, refs1 = ["the cat sat", "a dog"], ["the bat sat down", "a dog ran"]
    hyps2, refs2 = ["the cat", "uh a b"], ["the bat", "a c"]
    one, two = (assemble_edit_alignments(h, r, *_oracle_arrays(h, r)) for h, r in ((hyps1, refs1), (hyps2, refs2)))
    rep = ErrorReport(top=2)
    assert rep.summary() == {} and rep.format() == ""
    rep.add(one)
    first = rep.summary()["words"]
    rep.add(two)
    s = rep.summary()
    assert list(s) == ["words", "chars"]
    w = s["words"]
    both = one + two
    for k in ("hits", "substitutions", "deletions", "insertions", "ref_len"):
        assert w[k] == sum(r["words"][k] for r in both) and s["chars"][k] == sum(r["chars"][k] for r in both)
    assert first["ref_len"] == 7 and w["ref_len"] == 11
    assert (w["hits"], w["substitutions"], w["deletions"], w["insertions"]) == (6, 3, 2, 1)
    assert w["rate"] == 6 / 11 and w["substitution_rate"] == 3 / 11 and w["deletion_rate"] == 2 / 11 and w["insertion_rate"] == 1 / 11
    # the most frequent first, equal counts by token; cut to `top`
    assert w["top_substitutions"] == [("bat", "cat", 2), ("c", "b", 1)]
    assert w["top_deletions"] == [("down", 1), ("ran", 1)] and w["top_insertions"] == [("uh", 1)]
    text = rep.format()
    assert f"{100 * 6 / 11:.2f}" in text and f"{100 * 3 / 11:.2f}" in text and f"{100 * s['chars']['rate']:.2f}" in text
    assert "'bat' -> 'cat'" in text and text.endswith("\n")
    # a report fed words only
    rep = ErrorReport().add(assemble_edit_alignments(hyps1, refs1, *_oracle_arrays(hyps1, refs1), unit="word"))
    assert list(rep.summary()) == ["words"] and rep.summary()["words"] == dict(first, top_substitutions=first["top_substitutions"])
    assert ErrorReport(top=0).add(one).summary()["words"]["top_deletions"] == []
    with pytest.raises(ValueError):
        ErrorReport(top=-1)


def test_reliability():
    # planted: 4 tokens at 0.15 of which 1 right, 10 at 0.85 of which 9 right, 2 at exactly 1.0 both right (the last bin is closed)
    conf = [0.15] * 4 + [0.85] * 10 + [1.0] * 2
    right = [True, False, False, False] + [True] * 9 + [False] + [True, True]
    out = reliability(conf, right, bins=10)
    assert out["skipped"] == 0 and len(out["bins"]) == 10
    lo, hi, cnt, mean, acc = out["bins"][1]
    assert (lo, hi, cnt) == (0.1, 0.2, 4) and mean == pytest.approx(0.15) and acc == 0.25
    assert out["bins"][8][2:] == (10, pytest.approx(0.85), 0.9)
    assert out["bins"][9][2:] == (2, 1.0, 1.0)
    assert out["bins"][0][2] == 0 and math.isnan(out["bins"][0][3]) and math.isnan(out["bins"][0][4])
    assert out["ece"] == pytest.approx((4 * 0.10 + 10 * 0.05 + 2 * 0.0) / 16)
    # NaN confidences (units that were not scored) are dropped and counted
    out2 = reliability(conf + [float("nan")] * 3, right + [True, False, True])
    assert out2["skipped"] == 3 and out2["bins"][1][2] == 4 and out2["ece"] == pytest.approx(out["ece"])
    two = reliability([0.2, 0.7], [False, True], bins=2)
    assert [b[:3] for b in two["bins"]] == [(0.0, 0.5, 1), (0.5, 1.0, 1)] and two["ece"] == pytest.approx(0.5 * 0.2 + 0.5 * 0.3)
    empty = reliability([], [])
    assert math.isnan(empty["ece"]) and empty["skipped"] == 0 and all(b[2] == 0 for b in empty["bins"])
    for bad in (lambda: reliability([0.5], [True, False]), lambda: reliability([1.5], [True]), lambda: reliability([0.5], [True], bins=0)):
        with pytest.raises(ValueError):
            bad()


def test_abi_and_workspace():
    lib = _lib.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "ds2hip.h").read_text()
    for name in ("ds2_edit_align_i32", "ds2_edit_align_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_edit_align_i32"][1]) == 14
    f, row = lib.ds2_edit_align_workspace_bytes, lib.ds2_edit_distance_workspace_bytes
    assert f(0, 300) == 0 and f(7, 0) == 0
    for P, L in ((1, 64), (128, 64), (5, 65), (128, 300)):
        assert f(P, L) == P * ((L + 63) // 64) * L * 16 + row(P, L), (P, L)
    assert f(1, 64) == 1024 and f(5, 65) == 5 * (2 * 65 * 16 + 128) and f(128, 300) == 128 * (5 * 300 * 16 + 320)
    assert f(1, 50000) == 782 * 50000 * 16 + 50048      # the square growth, stated in the header


def test_edit_align_refusals_need_no_gpu():
    z64, z32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.DS2LibraryError):
        ops.edit_align(torch.zeros(4, dtype=torch.int32), z64, z32, z64, z32)
    with pytest.raises(_lib.DS2LibraryError):
        ops.edit_align([1, 2, 3], z64, z32, z64, z32)
    with pytest.raises(_lib.DS2LibraryError):                     # (the same shared check still guards edit_distance)
        ops.edit_distance(torch.zeros(4, dtype=torch.int32), z64, z32, z64, z32)
    if torch.cuda.is_available():
        with pytest.raises(TypeError):
            ops.edit_align(torch.zeros(4, dtype=torch.int64, device="cuda"), z64, z32, z64, z32)
    else:
        with pytest.raises(TypeError):                            # the dtype check comes next: reached here by a tensor that claims a GPU
            ops.edit_align(_FakeGpuTensor.make(torch.int64), z64, z32, z64, z32)


class _FakeGpuTensor(torch.Tensor):
    """an int tensor that answers is_cuda with True, so that the checks behind the device check run without a GPU"""
    @staticmethod
    def make(dtype):
        return torch.zeros(4, dtype=dtype).as_subclass(_FakeGpuTensor)

    @property
    def is_cuda(self):
        return True


def test_evaluate_errors_default():
    assert inspect.signature(DeepSpeech.evaluate).parameters["errors"].default is None
    assert list(inspect.signature(ops.edit_align).parameters) == list(inspect.signature(ops.edit_distance).parameters)
