"""-m gpu: BeamCTCDecoder / ds2_ctc_beam_decode_f32 (csrc/ctc_beam.h) against the fp64 restatement tests/ctc_beam_oracle.py.
Where every pruning and selection decision of the oracle cleared 1e-4 (relative to the scores' magnitude) the device's strings,
offsets and lengths must be exact and its scores within 1e-4 relative; the rest is counted, and at least 90 % of the utterances
of each grid point must be compared exactly."""
import math
import os
import tempfile

import numpy as np
import pytest
import torch

import ctc_beam_oracle as O
from helpers import model_inputs
from oracle import ds2_oracle as O2
from test_gpu_model import make_model

pytestmark = pytest.mark.gpu
LABELS = "_ABCDE "


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _probs(B, T, C, seed, blank, scale=16.0):
    """peaked random per-frame distributions: softmax of scaled normal logits, the blank favoured as in a trained CTC model"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, T, C), generator=g) * scale
    z[..., blank] += 2.0
    return torch.softmax(z, dim=-1).float()


def _sizes(B, T, seed):
    g = torch.Generator().manual_seed(seed + 1)
    s = torch.randint(1, T + 1, (B,), generator=g)
    s[0] = T
    if B >= 3:
        s[1], s[2] = 0, 1
    return s.int()


def _compare(probs, sizes, out, blank, K, top_n, cut):
    """(number of utterances, number whose best beam was compared exactly).  An utterance whose every oracle decision cleared the
    margin is compared in full (the survivor set, every score and offset, the order of the decided ranks); otherwise (over hundreds
    of frames some boundary decision is nearly always close) the ranks whose final gaps to both neighbours exceed 1e-5 relative are
    compared."""
    labels, offs, lens, scores = (x.cpu() for x in out)
    B = probs.shape[0]
    exact = 0
    for b in range(B):
        n = int(sizes[b]) if sizes is not None else probs.shape[1]
        res = O.beam_search(probs[b].double().numpy(), n, blank, K, top_n, cut)
        beams = res["beams"]
        if O.decisive(res):
            got = {tuple(labels[b, k, :lens[b, k]].tolist()): k for k in range(K) if scores[b, k] > -math.inf}
            assert len(got) == len(beams), (b, len(got), len(beams))
            for k, (pr, off, s) in enumerate(beams):
                kk = got[pr]
                assert abs(float(scores[b, kk]) - s) <= 1e-4 * max(1.0, abs(s)), (b, k, float(scores[b, kk]), s)
                assert tuple(offs[b, kk, :lens[b, kk]].tolist()) == off, (b, k)
            for k in range(len(beams), K):
                assert int(lens[b, k]) == 0 and scores[b, k] == -math.inf
            ranks = O.decisive_ranks(res)
        else:
            ranks = O.decisive_ranks(res, 1e-5)
        for k in ranks:
            pr, off, s = beams[k]
            assert tuple(labels[b, k, :lens[b, k]].tolist()) == pr, (b, k)
            assert tuple(offs[b, k, :lens[b, k]].tolist()) == off, (b, k)
            assert abs(float(scores[b, k]) - s) <= 1e-4 * max(1.0, abs(s)), (b, k, float(scores[b, k]), s)
        exact += 0 in ranks
    return B, exact


GRID = [
    # B, T, C, K, cutoff_top_n, cutoff_prob, blank, input form
    (1, 1, 2, 1, 40, 1.0, 0, "plain"),
    (7, 5, 29, 10, 40, 1.0, 0, "strided"),
    (7, 5, 29, 256, 29, 0.99, 28, "host"),
    (7, 5, 2, 100, 2, 1.0, 1, "plain"),
    (7, 40, 29, 100, 40, 0.99, 0, "strided"),
    (7, 40, 29, 1, 29, 1.0, 28, "host"),
    (7, 20, 3000, 10, 40, 1.0, 0, "strided"),
    (1, 5, 3000, 100, 3000, 1.0, 2999, "plain"),
    (7, 5, 3000, 256, 40, 0.99, 2999, "host"),
    (64, 501, 29, 10, 40, 1.0, 0, "strided"),
    (7, 501, 29, 256, 29, 1.0, 28, "plain"),
]


def _grid_point(dev, B, T, C, K, top_n, cut, blank, form):
    from asr_amd import ops
    probs = _probs(B, T, C, 1000 + B + T + C + K, blank)
    sizes = _sizes(B, T, K) if B > 1 else None
    if form == "strided":
        x = probs.transpose(0, 1).contiguous().to(dev).transpose(0, 1)      # (T,B,C) storage viewed as (B,T,C)
        assert not x.is_contiguous()
        out = ops.ctc_beam_decode(x, sizes, blank, K, top_n, cut)
    elif form == "host":
        from asr_amd.decoders import BeamCTCDecoder
        labels = {chr(0x3041 + i) if i else "_": i for i in range(C)}
        d = BeamCTCDecoder(labels, beam_width=K, cutoff_top_n=top_n, cutoff_prob=cut, blank_index=blank)
        strings, offsets = d.decode(probs, sizes)          # host tensor in
        out = ops.ctc_beam_decode(probs.to(dev), sizes, blank, K, top_n, cut)
        lens = out[2].cpu()
        for b in range(B):
            for k in range(K):
                assert len(strings[b][k]) == int(lens[b, k]) and offsets[b][k].numel() == int(lens[b, k])
        assert torch.equal(d.last_scores, out[3].cpu())
    else:
        out = ops.ctc_beam_decode(probs.to(dev), sizes, blank, K, top_n, cut)
    return _compare(probs, sizes, out, blank, K, top_n, cut)


def test_beam_against_oracle_grid(dev):
    """every grid point against the oracle; at least 90 % of all the grid's utterances have their best beam compared exactly"""
    n_all = exact_all = 0
    for point in GRID:
        n, exact = _grid_point(dev, *point)
        assert exact >= 0.5 * n, f"{point}: the best beam of only {exact}/{n} utterances was decided"
        n_all += n
        exact_all += exact
    assert exact_all >= 0.9 * n_all, f"{exact_all}/{n_all}"


def _exact(probs, K, blank=0, top_n=None):
    """the device decode of quantised (B,T,C) probabilities whose tied totals tie bit for bit in fp32 and fp64: every slot's labels,
    offsets and length equal the oracle's, scores to fp32 rounding"""
    from asr_amd import ops
    probs = torch.as_tensor(probs, dtype=torch.float32)
    B, T, C = probs.shape
    top_n = C if top_n is None else top_n
    labels, offs, lens, scores = (x.cpu() for x in ops.ctc_beam_decode(probs.cuda(), None, blank, K, top_n, 1.0))
    for b in range(B):
        beams = O.beam_search(probs[b].double().numpy(), None, blank, K, top_n, 1.0)["beams"]
        for k in range(K):
            if k < len(beams):
                pr, off, s = beams[k]
                assert int(lens[b, k]) == len(pr), (b, k)
                assert tuple(labels[b, k, :len(pr)].tolist()) == pr, (b, k, labels[b, k, :len(pr)].tolist(), pr)
                assert tuple(offs[b, k, :len(pr)].tolist()) == off, (b, k)
                assert abs(float(scores[b, k]) - s) <= 1e-6 * max(1.0, abs(s)), (b, k, float(scores[b, k]), s)
            else:
                assert int(lens[b, k]) == 0 and scores[b, k] == -math.inf
            assert not labels[b, k, int(lens[b, k]):].any() and not offs[b, k, int(lens[b, k]):].any()
    return labels, lens


def test_beam_tie_rule_on_device(dev):
    """exact ties decided by the contract: shorter prefix first, then the smaller label sequence"""
    flat = [[[0.25] * 4]]
    labels, lens = _exact(flat, 2)                    # (), (1,) survive; (2,), (3,) lose the tie
    assert lens[0].tolist() == [0, 1] and int(labels[0, 1, 0]) == 1
    _exact(flat, 4)
    _exact(flat, 4, top_n=2)                          # the top-2 cut keeps the blank and class 1 (lower index wins a probability tie)
    q = [0.5, 0.25, 0.25]
    _exact([[q, q]], 3)                               # P(A) = P(B) > P(): A before B
    _exact([[q[::-1], q[::-1]]], 3, blank=2)


def test_beam_tie_rule_walks_the_chains(dev):
    """tied prefixes of equal length that differ at an early position, and at two positions in opposite order (ADBE vs BDAE): the
    earliest difference decides, so the chain walk must run several steps and keep the last difference it sees.  Every tied total is
    formed by the same additions of the same values, so the ties are exact in fp32 as well."""
    q = [0.5, 0.25, 0.25, 0, 0, 0]
    h = [0, 0.5, 0.5, 0, 0, 0]
    d, e = [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0]
    for K in (3, 5, 7, 9, 12):
        _exact([[q, d, q, e]], K)
        _exact([[h, d, h, d, h, e], [d, h, d, h, d, h]], K)
    labels, lens = _exact([[q, d, q, e]], 7)
    assert [tuple(labels[0, k, :lens[0, k]].tolist()) for k in (5, 6)] == [(1, 3, 1, 4), (1, 3, 2, 4)]
    labels, lens = _exact([[h, d, h, d, h, e]], 3)
    assert [tuple(labels[0, k, :lens[0, k]].tolist()) for k in range(3)] == [(1, 3, 1, 3, 1, 4), (1, 3, 1, 3, 2, 4), (1, 3, 2, 3, 1, 4)]


def test_sizes_must_cover_the_batch(dev):
    from asr_amd import ops
    probs = _probs(4, 10, 29, 3, 0).to(dev)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(probs, torch.tensor([10, 10, 10]), 0, 4, 40, 1.0)
    with pytest.raises(ValueError):
        ops.greedy_decode(probs, torch.tensor([10, 10, 10]), 0)


def test_beam_greedy_known_answers(dev):
    from asr_amd.decoders import BeamCTCDecoder, GreedyDecoder
    labels = {c: i for i, c in enumerate(LABELS)}
    d = BeamCTCDecoder(labels, beam_width=4)
    g = GreedyDecoder(labels)
    for path, want in (([1, 0, 1], "AA"), ([1, 6, 2], "A B"), ([1, 1, 0, 2, 2], "AB"), ([0, 0, 0], "")):
        p = torch.zeros((1, len(path), len(LABELS)))
        p[0, torch.arange(len(path)), torch.tensor(path)] = 1.0
        strings, offsets = d.decode(p.to(dev))
        gs, go = g.decode(p.to(dev))
        assert strings[0][0] == want == gs[0][0]
        assert offsets[0][0].tolist() == go[0][0].tolist()
        assert float(d.last_scores[0, 0]) == 0.0 and all(s == "" for s in strings[0][1:])


@pytest.mark.parametrize("T,C,blank", [(3, 3, 0), (4, 4, 0), (5, 3, 2)])
def test_beam_exhaustive_matches_ctc_loss(dev, T, C, blank):
    from asr_amd import ops
    g = torch.Generator().manual_seed(T * 10 + C)
    probs = torch.softmax(torch.randn((1, T, C), generator=g), -1).float()
    truth = O.brute_force_label_logprobs(probs[0].double().numpy(), blank)
    K = min(256, len(truth) + 2)
    labels, offs, lens, scores = (x.cpu() for x in ops.ctc_beam_decode(probs.to(dev), None, blank, K, C, 1.0))
    assert int((scores[0] > -math.inf).sum()) == len(truth)
    lp = torch.log(probs[0].double()).unsqueeze(1)
    for k in range(len(truth)):
        lab = labels[0, k, :lens[0, k]].long()
        nll = torch.nn.functional.ctc_loss(lp, lab.unsqueeze(0), torch.tensor([T]), torch.tensor([lab.numel()]), blank=blank,
                                           reduction="none")
        assert abs(float(scores[0, k]) + float(nll[0])) <= 1e-5 * max(1.0, float(nll[0]))


def test_beam_deterministic_and_limits(dev):
    from asr_amd import ops, _lib
    probs = _probs(16, 200, 29, 7, 0).to(dev)
    a = ops.ctc_beam_decode(probs, None, 0, 100, 40, 1.0)
    b = ops.ctc_beam_decode(probs, None, 0, 100, 40, 1.0)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    kmax = _lib.load().ds2_ctc_beam_max_width()
    with pytest.raises((ValueError, _lib.DS2LibraryError), match=str(kmax)):
        ops.ctc_beam_decode(probs, None, 0, kmax + 1, 40, 1.0)
    with pytest.raises((ValueError, _lib.DS2LibraryError)):
        ops.ctc_beam_decode(probs, None, 0, 0, 40, 1.0)


def test_beam_full_size(dev):
    from asr_amd import ops
    B, T, C, K = 64, 501, 29, 100
    probs = _probs(B, T, C, 64501, 0)
    out = ops.ctc_beam_decode(probs.to(dev), None, 0, K, 40, 1.0)
    n, exact = _compare(probs, None, out, 0, K, 40, 1.0)
    assert exact >= 0.9 * n, f"{exact}/{n}"


def test_evaluate_with_beam_decoder(dev):
    """DeepSpeech.evaluate with model.decoder = BeamCTCDecoder: the transcripts are the oracle's beam decode of the fp64 CPU oracle's
    eval probabilities where that decode's best beam is clear of the second, and WER/CER follow from them."""
    from asr_amd.decoders import BeamCTCDecoder
    cfg = dict(rnn="gru", hidden=40, layers=2, classes=29, t_ins=[140, 120, 90, 33])
    sd, x, targets, pct, tsz = model_inputs(cfg)
    model = make_model(cfg, sd)
    model.eval()
    model.decoder = BeamCTCDecoder(model.labels, beam_width=16)
    dec = model.decoder
    lens = O2.lengths_from_percentages(pct, x.size(3))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    probs_ref, out_lens_ref = O2.forward(sd64, x.double(), lens, training=False)
    probs_ref = probs_ref.numpy()
    report = os.path.join(tempfile.mkdtemp(), "eval.txt")
    wer, cer, output_data = model.evaluate(loader=[(x, targets, pct.clone(), tsz)], device="cuda", output_file=report)
    probs, out_sizes, target_strings = output_data[0]
    strings, _ = dec.decode(torch.from_numpy(probs).cuda(), torch.as_tensor(out_sizes))
    tot_w = tot_c = n_w = n_c = 0
    decisive = 0
    for b in range(len(cfg["t_ins"])):
        res = O.beam_search(probs_ref[b], int(out_lens_ref[b]), 0, 16, 40, 1.0)
        hyp = strings[b][0]
        if 0 in O.decisive_ranks(res, 1e-5):   # the best beam is clear of the second
            decisive += 1
            assert hyp == "".join(" " if i == dec.space_index else dec.int_to_char[i] for i in res["beams"][0][0]), b
        ref = target_strings[b][0]
        tot_w += dec.wer(hyp, ref); tot_c += dec.cer(hyp, ref)
        n_w += len(ref.split()); n_c += len(ref.replace(" ", ""))
    assert decisive >= 3
    assert abs(wer - 100.0 * tot_w / max(n_w, 1)) < 1e-9 and abs(cer - 100.0 * tot_c / max(n_c, 1)) < 1e-9
