"""Batched edit alignment on the GPU (ops.edit_align, csrc/edit_align.h) and what is built on it (Decoder.align_batch,
DeepSpeech.evaluate(errors=...)): counts and maps equal to tests/edit_align_oracle.py to the integer, and S + D + I equal to
ops.edit_distance on the same packed input."""
import os
import random
import tempfile

import numpy as np
import pytest
import torch

import edit_align_oracle as O
from asr_amd import ops
from asr_amd.decoders import BeamCTCDecoder, ErrorReport, GreedyDecoder, assemble_edit_alignments, pack_scoring
from helpers import model_inputs
from test_gpu_model import make_model

pytestmark = pytest.mark.gpu


def _pack(pairs):
    seq, a_off, a_len, b_off, b_len, pos = [], [], [], [], [], 0
    for a, b in pairs:
        a_off.append(pos); a_len.append(len(a)); seq += a; pos += len(a)
        b_off.append(pos); b_len.append(len(b)); seq += b; pos += len(b)
    return (torch.tensor(seq, dtype=torch.int32, device="cuda"), torch.tensor(a_off, dtype=torch.int64),
            torch.tensor(a_len, dtype=torch.int32), torch.tensor(b_off, dtype=torch.int64), torch.tensor(b_len, dtype=torch.int32))


def _check(pairs):
    """the kernel on `pairs` against the oracle, entry for entry, and against the distance kernel; returns the raw outputs"""
    args = _pack(pairs)
    counts, a_map, b_map = ops.edit_align(*args)
    max_len = max([len(x) for p in pairs for x in p] + [0])
    assert counts.dtype == a_map.dtype == b_map.dtype == torch.int32 and counts.is_cuda and a_map.is_cuda and b_map.is_cuda
    assert tuple(counts.shape) == (len(pairs), 4) and tuple(a_map.shape) == tuple(b_map.shape) == (len(pairs), max_len)
    want_c, want_a, want_b = O.align_padded(pairs, max_len)
    got_c, got_a, got_b = counts.cpu().tolist(), a_map.cpu().tolist(), b_map.cpu().tolist()
    for p, (a, b) in enumerate(pairs):
        assert got_c[p] == want_c[p], (p, len(a), len(b))
        assert got_a[p] == want_a[p], (p, len(a), len(b))
        assert got_b[p] == want_b[p], (p, len(a), len(b))
    assert counts[:, 1:].sum(1).cpu().tolist() == ops.edit_distance(*args).cpu().tolist()
    return counts, a_map, b_map


def _rand(rng, n, k):
    return [rng.randrange(k) for _ in range(n)]


LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("alphabet", [2, 30])
def test_every_length_pair(alphabet):
    """both orientations (the hypothesis on the rows and on the columns), the strip and window edges; alphabet 2: ties at almost every cell"""
    rng = random.Random(alphabet)
    _check([(_rand(rng, m, alphabet), _rand(rng, n, alphabet)) for m in LENS for n in LENS])


def test_long_pair_in_both_orders():
    """300 x 1000: 5 strips whose columns and bottom rows go through the workspace, 16 windows per strip on the way back"""
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 3, 300).tolist(), rng.integers(0, 3, 1000).tolist()
    b[400:550] = a[100:250]      # a shared run
    _check([(a, b), (b, a)])


def test_identical_and_disjoint_sides():
    rng = random.Random(1)
    sides = [_rand(rng, n, 7) for n in LENS + [300]]
    counts, a_map, b_map = _check([(s, list(s)) for s in sides])
    for p, s in enumerate(sides):
        assert counts[p].tolist() == [len(s), 0, 0, 0]
        assert a_map[p, :len(s)].tolist() == list(range(len(s))) == b_map[p, :len(s)].tolist()
    disjoint = [(_rand(rng, m, 7), [7 + v for v in _rand(rng, n, 7)]) for m in LENS + [300] for n in (0, 1, 65, 300)]
    counts, a_map, b_map = _check(disjoint)     # where the n - m deletions lie is the oracle's word, checked entry for entry above
    for p, (a, b) in enumerate(disjoint):
        assert counts[p].tolist() == [0, min(len(a), len(b)), max(len(b) - len(a), 0), max(len(a) - len(b), 0)]


def test_batch_sizes_and_repeatability():
    rng = random.Random(5)
    _check([(_rand(rng, 90, 4), _rand(rng, 70, 4))])
    _check([(_rand(rng, rng.choice([0, 3, 70]), 3), _rand(rng, rng.choice([5, 64, 130]), 3)) for _ in range(5)])
    many = [(_rand(rng, rng.choice([0, 3, 40, 64, 100, 130]), 6), _rand(rng, rng.choice([0, 5, 64, 65, 130, 200]), 6)) for _ in range(600)]
    first = _check(many)
    again = ops.edit_align(*_pack(many))
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_empty_batch_and_zero_lengths():
    seq = torch.zeros(0, dtype=torch.int32, device="cuda")
    e64, e32 = torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    counts, a_map, b_map = ops.edit_align(seq, e64, e32, e64, e32)
    assert tuple(counts.shape) == (0, 4) and tuple(a_map.shape) == tuple(b_map.shape) == (0, 0)
    counts, a_map, b_map = _check([([], []), ([], [])])
    assert counts.tolist() == [[0, 0, 0, 0]] * 2 and tuple(a_map.shape) == (2, 0)
    with pytest.raises(ValueError):
        ops.edit_align(torch.zeros(3, dtype=torch.int32, device="cuda"), [0], [3], [1], [3])     # host ranges are checked against seq


def test_rejected_problem_among_good_ones():
    """device-side offsets past seq, and a side above max_len: -1 counts and -1 rows, the neighbours as the oracle has them"""
    rng = random.Random(9)
    pairs = [(_rand(rng, 70, 3), _rand(rng, 40, 3)), (_rand(rng, 20, 3), _rand(rng, 30, 3)), (_rand(rng, 5, 3), _rand(rng, 66, 3)),
             (_rand(rng, 10, 3), _rand(rng, 10, 3))]
    seq, a_off, a_len, b_off, b_len = _pack(pairs)
    b_off[1] = seq.numel() - 29          # the last symbol would lie one past the buffer
    a_off[3], a_len[3] = 0, 71           # a side above max_len, inside the buffer
    counts, a_map, b_map = ops.edit_align(seq, a_off.cuda(), a_len.cuda(), b_off.cuda(), b_len.cuda(), max_len=70)
    want_c, want_a, want_b = O.align_padded(pairs, 70)
    for p in (1, 3):
        want_c[p], want_a[p], want_b[p] = [-1] * 4, [-1] * 70, [-1] * 70
    assert counts.cpu().tolist() == want_c and a_map.cpu().tolist() == want_a and b_map.cpu().tolist() == want_b
    dist = ops.edit_distance(seq, a_off.cuda(), a_len.cuda(), b_off.cuda(), b_len.cuda(), max_len=70).cpu().tolist()
    assert dist[1] == -1 and [dist[0], dist[2]] == [sum(want_c[0][1:]), sum(want_c[2][1:])]


def _strings(rng, n):
    words = ["the", "a", "cat", "こんにちは", "\U0001F600", "the", "dog", "a"]
    return [" ".join(rng.choice(words) for _ in range(rng.randrange(0, 12))) + rng.choice(["", " "]) for _ in range(n)]


def test_align_batch_equals_assembled_oracle():
    rng = random.Random(11)
    hyps, refs = _strings(rng, 10), _strings(rng, 10)
    hyps[0], refs[1], hyps[2], refs[2] = "", "", "  ", ""
    hyps[3], refs[3] = "the the the cat", "the cat the the"
    hyps[4], refs[4] = "ab" * 40, "ba" * 45            # characters past one strip
    d = GreedyDecoder({"_": 0, "a": 1, " ": 2})
    got = d.align_batch(hyps, refs)
    seq, a_off, a_len, b_off, b_len, _, _ = pack_scoring(hyps, refs)
    side = lambda off, ln, p: seq[off[p]:off[p] + ln[p]].tolist()   # noqa: E731
    max_len = int(max(a_len.max(), b_len.max()))
    want = assemble_edit_alignments(hyps, refs, *O.align_padded([(side(a_off, a_len, p), side(b_off, b_len, p)) for p in range(20)], max_len))
    assert got == want
    scores = d.score_batch(hyps, refs).tolist()
    assert [[r["words"]["distance"], r["words"]["ref_len"], r["chars"]["distance"], r["chars"]["ref_len"]] for r in got] == scores
    assert d.align_batch(hyps, refs, unit="word") == [{"words": r["words"]} for r in want]
    assert d.align_batch(hyps, refs, unit="char") == [{"chars": r["chars"]} for r in want]
    assert d.align_batch([], []) == []
    with pytest.raises(ValueError):
        d.align_batch(hyps, refs, unit="phone")


class HostScoring(GreedyDecoder):
    def cer(self, s1, s2):
        return super().cer(s1, s2)


@pytest.mark.parametrize("beam", [False, True])
def test_evaluate_with_error_report(beam):
    cfg = dict(rnn="gru", hidden=40, layers=2, classes=29, t_ins=[140, 120, 90, 33])
    sd, x, targets, pct, tsz = model_inputs(cfg)
    model = make_model(cfg, sd)
    model.eval()
    model.decoder = BeamCTCDecoder(model.labels, beam_width=16) if beam else GreedyDecoder(model.labels)
    loader = lambda: [(x, targets, pct.clone(), tsz), (x[:2], targets[:int(tsz[:2].sum())], pct[:2].clone(), tsz[:2])]   # noqa: E731
    tmp = tempfile.mkdtemp()
    plain, full = os.path.join(tmp, "plain.txt"), os.path.join(tmp, "errors.txt")
    wer0, cer0, _ = model.evaluate(loader=loader(), device="cuda", output_file=plain)
    rep = ErrorReport()
    wer1, cer1, out1 = model.evaluate(loader=loader(), device="cuda", output_file=full, errors=rep)
    assert (wer0, cer0) == (wer1, cer1) and len(out1) == 2
    s = rep.summary()
    ref_strings = GreedyDecoder(model.labels).convert_to_strings([targets[int(tsz[:i].sum()):int(tsz[:i + 1].sum())] for i in range(len(tsz))])
    ref_strings = [r[0] for r in ref_strings] + [r[0] for r in ref_strings[:2]]
    for key, rate, n_ref in (("words", wer1, sum(len(r.split()) for r in ref_strings)), ("chars", cer1, sum(len(r.replace(" ", "")) for r in ref_strings))):
        u = s[key]
        assert u["ref_len"] == n_ref and u["hits"] + u["substitutions"] + u["deletions"] == n_ref
        assert float(u["substitutions"] + u["deletions"] + u["insertions"]) / max(n_ref, 1) * 100 == rate      # S + D + I is the total distance
    a, b = open(plain, "rb").read(), open(full, "rb").read()
    assert b.startswith(a) and b[len(a):].decode() == rep.format() and len(b) > len(a)
    model.decoder = HostScoring(model.labels)
    with pytest.raises(ValueError):
        model.evaluate(loader=loader(), device="cuda", errors=ErrorReport())
