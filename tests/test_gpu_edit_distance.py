"""Batched Levenshtein distance on the GPU (ops.edit_distance, csrc/edit_distance.h) and the WER / CER scoring built on it
(Decoder.score_batch, DeepSpeech.evaluate): exact integer equality with the host DP `_edit_distance` and Decoder.wer / cer."""
import os
import random
import tempfile

import numpy as np
import pytest
import torch

from asr_amd import ops
from asr_amd.decoders import BeamCTCDecoder, Decoder, GreedyDecoder, _edit_distance
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


def _gpu(pairs):
    return ops.edit_distance(*_pack(pairs)).cpu().tolist()


def _rand(rng, n, k):
    return [rng.randrange(k) for _ in range(n)]


LENS = [0, 1, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("alphabet", [2, 30, 1 << 20])
def test_edit_distance_equals_host_dp(alphabet):
    rng = random.Random(alphabet)
    pairs = [(_rand(rng, n, alphabet), _rand(rng, m, alphabet)) for n in LENS for m in LENS]
    pairs += [(_rand(rng, 1000, alphabet), _rand(rng, 200, alphabet)), (_rand(rng, 200, alphabet), _rand(rng, 1000, alphabet))]
    assert _gpu(pairs) == [_edit_distance(a, b) for a, b in pairs]


def test_edit_distance_long_pair():
    """5000 x 3000: 47 strips of 64 rows, each strip's bottom row of 5000 columns goes through the workspace"""
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 5, 5000).tolist(), rng.integers(0, 5, 3000).tolist()
    b[100:1100] = a[2000:3000]   # a long shared run, so the answer is well below the trivial bound
    want = _edit_distance(a, b)
    assert _gpu([(a, b), (b, a)]) == [want, want]


def test_edit_distance_identical_and_disjoint():
    rng = random.Random(1)
    same = [(s, list(s)) for s in (_rand(rng, n, 7) for n in LENS + [300])]
    assert _gpu(same) == [0] * len(same)
    disjoint = [(_rand(rng, n, 7), [7 + v for v in _rand(rng, m, 7)]) for n in LENS + [300] for m in (0, 1, 65, 300)]
    assert _gpu(disjoint) == [max(len(a), len(b)) for a, b in disjoint]


def test_edit_distance_batch_sizes_and_repeatability():
    rng = random.Random(5)
    one = [(_rand(rng, 90, 4), _rand(rng, 70, 4))]
    assert _gpu(one) == [_edit_distance(*one[0])]
    many = [(_rand(rng, rng.choice([0, 3, 40, 64, 100, 250]), 6), _rand(rng, rng.choice([0, 5, 64, 65, 130, 400]), 6)) for _ in range(600)]
    args = _pack(many)
    r1 = ops.edit_distance(*args).cpu()
    r2 = ops.edit_distance(*args).cpu()
    assert torch.equal(r1, r2)
    assert r1.tolist() == [_edit_distance(a, b) for a, b in many]


def test_edit_distance_aliased_sides_and_device_lengths():
    """both sides of a pair may point into the same symbols; device-resident offsets / lengths take the same path"""
    seq = torch.tensor(list(range(50)) * 3, dtype=torch.int32, device="cuda")
    a_off, a_len = torch.tensor([0, 10, 0], dtype=torch.int64), torch.tensor([150, 20, 70], dtype=torch.int32)
    b_off, b_len = torch.tensor([50, 60, 0], dtype=torch.int64), torch.tensor([100, 20, 70], dtype=torch.int32)
    host = seq.cpu().tolist()
    want = [_edit_distance(host[int(o):int(o) + int(n)], host[int(p):int(p) + int(m)]) for o, n, p, m in zip(a_off, a_len, b_off, b_len)]
    assert ops.edit_distance(seq, a_off, a_len, b_off, b_len).cpu().tolist() == want
    assert ops.edit_distance(seq, a_off.cuda(), a_len.cuda(), b_off.cuda(), b_len.cuda()).cpu().tolist() == want
    with pytest.raises(ValueError):
        ops.edit_distance(seq, a_off, a_len + 1, b_off, b_len)


def _strings(rng, n):
    words = ["the", "a", "cat", "こんにちは", "\U0001F600", "x\ty", "dog", "e　f", "g\xa0h"]
    return [" ".join(rng.choice(words) for _ in range(rng.randrange(0, 40))) + rng.choice(["", " ", "  "]) for _ in range(n)]


def test_score_batch_equals_wer_and_cer():
    rng = random.Random(11)
    hyps, refs = _strings(rng, 70), _strings(rng, 70)
    hyps[0], refs[1], hyps[2], refs[2] = "", "", "   ", "   "
    hyps[3] = "abc" * 200            # a long char side (> 64 rows in both problems' shorter sides elsewhere)
    refs[3] = "abd" * 150
    d = GreedyDecoder({"_": 0, "a": 1, " ": 2})
    got = d.score_batch(hyps, refs)
    assert got.dtype == torch.int64 and tuple(got.shape) == (70, 4) and not got.is_cuda
    want = [[d.wer(h, r), len(r.split()), d.cer(h, r), len(r.replace(" ", ""))] for h, r in zip(hyps, refs)]
    assert got.tolist() == want
    assert tuple(d.score_batch([], []).shape) == (0, 4)


class HostScoring(GreedyDecoder):
    """forces evaluate()'s per-utterance host scoring and records that it ran"""
    calls = 0

    def wer(self, s1, s2):
        return super().wer(s1, s2)

    def cer(self, s1, s2):
        type(self).calls += 1
        return super().cer(s1, s2)


class HostScoringBeam(BeamCTCDecoder):
    def wer(self, s1, s2):
        return super().wer(s1, s2)

    def cer(self, s1, s2):
        return super().cer(s1, s2)


@pytest.mark.parametrize("beam", [False, True])
def test_evaluate_gpu_scoring_matches_host_scoring(beam):
    cfg = dict(rnn="gru", hidden=40, layers=2, classes=29, t_ins=[140, 120, 90, 33])
    sd, x, targets, pct, tsz = model_inputs(cfg)
    model = make_model(cfg, sd)
    model.eval()
    labels = model.labels
    gpu_dec = BeamCTCDecoder(labels, beam_width=16) if beam else GreedyDecoder(labels)
    host_dec = HostScoringBeam(labels, beam_width=16) if beam else HostScoring(labels)
    res = {}
    for name, dec in (("gpu", gpu_dec), ("host", host_dec)):
        model.decoder = dec
        report = os.path.join(tempfile.mkdtemp(), "eval.txt")
        HostScoring.calls = 0
        wer, cer, out = model.evaluate(loader=[(x, targets, pct.clone(), tsz), (x[:2], targets[:int(tsz[:2].sum())], pct[:2].clone(), tsz[:2])],
                                       device="cuda", output_file=report)
        res[name] = (wer, cer, open(report, "rb").read(), HostScoring.calls)
    assert res["gpu"][:2] == res["host"][:2]
    assert res["gpu"][2] == res["host"][2]
    assert res["gpu"][3] == 0
    if not beam:
        assert res["host"][3] == len(cfg["t_ins"]) + 2     # the overriding decoder's cer ran once per utterance
