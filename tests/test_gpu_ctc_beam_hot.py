"""-m gpu: the hotword arm of the CTC beam search (ds2_ctc_beam_decode_hot_f32, csrc/ctc_beam.h, csrc/ctc_hot.h) against the fp64
restatement tests/ctc_beam_hot_oracle.py, by the rule of test_gpu_ctc_beam_lm.py::_compare: where every pruning and selection decision
of the oracle cleared 1e-4 the device's beams, offsets and lengths must be exact and its scores within 1e-4 relative; otherwise the
ranks clear of both neighbours by 1e-5 are compared."""
import math
import tempfile

import pytest
import torch

import ctc_beam_hot_oracle as HO
from test_gpu_ctc_beam_lm import _compare, _decoder, _probs, _sizes

pytestmark = pytest.mark.gpu
PHRASES = ["BAD", "DEAD", "ACE", "ABC", "BCD", "E A", "CC"]
WEIGHTS = [1.0, 0.5, 2.0, 1.0, 1.5, 0.75, 1.25]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lm_dir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _hot(chars, blank, phrases=PHRASES, weights=WEIGHTS, inner=None):
    from asr_amd.decoders.hotwords import Hotwords
    return (Hotwords(list(zip(phrases, weights)), chars, blank),
            HO.HotFusion([[chars.index(c) for c in p] for p in phrases], weights, inner))


HOT_GRID = [
    # labels, blank, B, T, K, cutoff_top_n, cutoff_prob
    ("_ABCDE ", 0, 7, 12, 1, 40, 1.0),
    ("_ABCDE ", 0, 7, 20, 10, 40, 1.0),
    (" ABCDE_", 6, 7, 16, 100, 4, 0.99),
    ("_ABCDE ", 0, 9, 24, 100, 40, 0.95),
]


@pytest.mark.parametrize("point", HOT_GRID, ids=[f"K{g[4]}-top{g[5]}-cut{g[6]}-blank{g[1]}" for g in HOT_GRID])
def test_hot_only_against_oracle_grid(dev, point):
    """On the CPU the oracle alone decides the best beam of 7/7, 7/7, 7/7 and 9/9 utterances of these points, and the hotwords change
    the best beam of 1, 4, 4 and 6 of them."""
    from asr_amd import ops
    chars, blank, B, T, K, top_n, cut = point
    hot, fusion = _hot(chars, blank)
    probs = _probs(B, T, len(chars), 100 + K + T, blank)
    sizes = _sizes(B, T, K)
    x = probs.transpose(0, 1).contiguous().to(dev).transpose(0, 1)     # strided (T,B,C) storage
    out = ops.ctc_beam_decode(x, sizes, blank, K, top_n, cut, hotwords=hot)
    n, exact = _compare(probs, sizes, out, fusion, blank, K, top_n, cut)
    assert exact >= 0.5 * n, f"{point}: the best beam of only {exact}/{n} utterances was decided"


LM_POINTS = [
    # mode, labels, blank, B, T, K, cutoff_top_n, cutoff_prob, alpha, beta, order
    ("word", "_ABCDE ", 0, 7, 20, 10, 40, 1.0, 0.8, 1.0, 3),
    ("char", " ABCDE_", 6, 7, 16, 100, 40, 0.99, 1.2, -0.3, 2),
]


@pytest.mark.parametrize("point", LM_POINTS, ids=[g[0] for g in LM_POINTS])
def test_hot_with_lm_against_oracle(dev, lm_dir, point):
    """The LM grid's points with their seeds (ARPA seed K + T, frames 100 + K + T, sizes K).  On the CPU the oracle alone decides the best
    beam of 7/7 utterances at the word-mode point and 7/7 at the character-mode point; beside the LM alone the hotwords change the
    best beam of 2 utterances at each."""
    from asr_amd import ops
    mode, chars, blank, B, T, K, top_n, cut, alpha, beta, order = point
    d, inner = _decoder(lm_dir, mode, chars, blank, K, top_n, cut, alpha, beta, seed=K + T, order=order)
    hot, fusion = _hot(chars, blank, inner=inner)
    probs = _probs(B, T, len(chars), 100 + K + T, blank)
    sizes = _sizes(B, T, K)
    out = ops.ctc_beam_decode(probs.to(dev), sizes, blank, K, top_n, cut, d.lm, alpha, beta, hotwords=hot)
    n, exact = _compare(probs, sizes, out, fusion, blank, K, top_n, cut)
    assert exact >= 0.5 * n, f"{point}: the best beam of only {exact}/{n} utterances was decided"
    d.set_hotwords(hot)
    d.decode(probs, sizes)                                                # the public path, host tensor in
    assert torch.equal(d.last_scores, out[3].cpu())


@pytest.mark.parametrize("T,C,seed", [(3, 4, 0), (4, 4, 1), (3, 5, 2), (5, 3, 3)])   # fewer than 256 labelings: an unbounded beam
def test_hot_exhaustive_matches_brute_force(dev, T, C, seed):
    from asr_amd import ops
    chars = "_ABCDE"[:C - 1] + " "
    names = ["AA", "A "] if C == 3 else ["AB", "BA", "B "]
    hot, fusion = _hot(chars, 0, names, [1.0, 0.5, 1.5][:len(names)])
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(torch.randn((1, T, C), generator=g) * 2, -1).float()
    want = HO.brute_force_best(probs[0].double().numpy(), fusion, 0)
    labels, offs, lens, scores = (x.cpu() for x in ops.ctc_beam_decode(probs.to(dev), None, 0, 256, C, 1.0, hotwords=hot))
    assert tuple(labels[0, 0, :lens[0, 0]].tolist()) == want[0]
    assert abs(float(scores[0, 0]) - want[1]) <= 1e-4 * max(1.0, abs(want[1]))


def _bits_equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("C,K,top_n,cut,blank", [(7, 1, 40, 1.0, 0), (7, 10, 40, 1.0, 0), (29, 100, 40, 1.0, 0), (29, 100, 8, 0.99, 28),
                                                 (29, 10, 29, 1.0, 5)])
def test_zero_weight_hot_only_is_bit_identical_to_the_plain_kernel(dev, C, K, top_n, cut, blank):
    """all weights 0: every term is 0.0f and the final re-sort finds the survivors in order"""
    from asr_amd import ops
    from asr_amd.decoders.hotwords import Hotwords
    nb = [i for i in range(C) if i != blank]
    hot = Hotwords([nb[:3], [nb[1], nb[2], nb[0], nb[1]], [nb[2], nb[2]], [nb[-1]]], [chr(65 + i) for i in range(C)], blank, 0.0)
    for scale in (16.0, 1.0):
        probs = _probs(8, 200, C, C + K, blank, scale).to(dev)
        sizes = _sizes(8, 200, C)
        _bits_equal(ops.ctc_beam_decode(probs, sizes, blank, K, top_n, cut), ops.ctc_beam_decode(probs, sizes, blank, K, top_n, cut, hotwords=hot))


@pytest.mark.parametrize("mode", ["word", "char"])
def test_zero_weight_hotwords_with_lm_are_bit_identical_to_the_lm_entry(dev, lm_dir, mode):
    from asr_amd import ops
    chars = "_ABCDE "
    d, _ = _decoder(lm_dir, mode, chars, 0, 100, 40, 1.0, 0.8, 1.0, seed=11)
    hot, _ = _hot(chars, 0, weights=[0.0] * len(PHRASES))
    probs = _probs(8, 60, 7, 7, 0).to(dev)
    sizes = _sizes(8, 60, 3)
    _bits_equal(ops.ctc_beam_decode(probs, sizes, 0, 100, 40, 1.0, d.lm, 0.8, 1.0),
                ops.ctc_beam_decode(probs, sizes, 0, 100, 40, 1.0, d.lm, 0.8, 1.0, hotwords=hot))


def _frames(rows, C=7):
    p = torch.zeros((1, len(rows), C))
    for t, row in enumerate(rows):
        for c, v in row.items():
            p[0, t, c] = v
    return p


def test_hot_known_answers(dev):
    """The acoustically ambiguous frames of test_lm_known_answers: the plain search reads "DAD", the hotword "BAD" alone flips it.  A
    hotword nobody completes ("BADE") leaves every hypothesis with its plain score: the end term takes the lead back."""
    from asr_amd.decoders import BeamCTCDecoder
    chars = "_ABCDE "
    labels = {c: i for i, c in enumerate(chars)}
    p = _frames([{4: 0.55, 2: 0.45}, {0: 1.0}, {1: 1.0}, {0: 1.0}, {4: 0.55, 2: 0.45}]).to(dev)
    plain = BeamCTCDecoder(labels, beam_width=10)
    assert plain.decode(p)[0][0][0] == "DAD"
    boosted = BeamCTCDecoder(labels, beam_width=10, hotwords=["BAD"], hotword_weight=1.0)
    assert boosted.decode(p)[0][0][0] == "BAD"
    assert abs(float(boosted.last_scores[0, 0]) - (math.log(0.45 * 0.55) + 3.0)) < 1e-5
    q = _frames([{4: 0.55, 2: 0.45}, {0: 1.0}, {1: 1.0}, {0: 1.0}, {4: 0.6, 2: 0.4}]).to(dev)   # four readings, no two tied
    want = plain.decode(q)[0][0][:4]
    want_scores = plain.last_scores[0, :4].clone()
    assert want == ["DAD", "BAD", "DAB", "BAB"]
    partial = BeamCTCDecoder(labels, beam_width=10, hotwords=[("BADE", 2.0)])
    assert partial.decode(q)[0][0][:4] == want
    assert torch.allclose(partial.last_scores[0, :4], want_scores, rtol=0, atol=1e-5)
    assert bool(torch.isinf(partial.last_scores[0, 4:]).all())


def test_hot_public_path(dev):
    from asr_amd import ops
    from asr_amd.decoders import BeamCTCDecoder
    chars = "_ABCDEFGHIJKLMNOPQRSTUVWXYZ' "
    labels = {c: i for i, c in enumerate(chars)}
    probs = _probs(16, 200, 29, 7, 0)
    d = BeamCTCDecoder(labels, beam_width=100, hotwords=["HELLO WORLD", ("QUIZ", 3.0), "AB"], hotword_weight=1.5)
    a = ops.ctc_beam_decode(probs.to(dev), None, 0, 100, 40, 1.0, hotwords=d.hotwords)
    b = ops.ctc_beam_decode(probs.to(dev), None, 0, 100, 40, 1.0, hotwords=d.hotwords)
    _bits_equal(a, b)
    first, _ = d.decode(probs)                                            # host tensor in
    assert torch.equal(d.last_scores, a[3].cpu())
    d.set_hotwords(["XYZ", "E"], 4.0)
    second, _ = d.decode(probs)
    assert [s[0] for s in first] != [s[0] for s in second]
    d.set_hotwords(None)
    d.decode(probs)
    assert torch.equal(d.last_scores, ops.ctc_beam_decode(probs.to(dev), None, 0, 100, 40, 1.0)[3].cpu())
    d.set_hotwords(["AB"])
    with pytest.raises(ValueError, match="4096"):                         # the full grid's limit holds without a language model too
        ops.ctc_beam_decode(probs.to(dev), None, 0, 256, 40, 1.0, hotwords=d.hotwords)
    ops.ctc_beam_decode(probs.to(dev), None, 0, 256, 14, 1.0, hotwords=d.hotwords)   # 256 * 16 slots: at the limit
