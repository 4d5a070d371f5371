"""BeamCTCDecoder without a GPU: the public class, the C ABI's size query, and the fp64 oracle (tests/ctc_beam_oracle.py) checked
against brute-force alignment enumeration and torch's CTC loss, plus its tie and offset rules on hand-built cases."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_oracle as O   # noqa: E402

LABELS = "_ABCDE "   # index 0 is the blank, 6 the space


def test_beam_decoder_import_and_defaults():
    from asr_amd.decoders import BeamCTCDecoder
    import asr_amd
    assert asr_amd.BeamCTCDecoder is BeamCTCDecoder
    d = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)})
    assert (d.cutoff_top_n, d.cutoff_prob, d.beam_width, d.blank_index, d.lm_path) == (40, 1.0, 100, 0, None)
    assert (d.alpha, d.beta, d.num_processes) == (0, 0, 4)
    assert d.space_index == 6 and d.int_to_char[1] == "A"
    s = BeamCTCDecoder(LABELS, beam_width=8, blank_index=0)
    assert s.int_to_char[2] == "B" and s.beam_width == 8
    with pytest.raises(NotImplementedError):
        BeamCTCDecoder(LABELS, lm_path="lm.binary")


def test_beam_decoder_conversions():
    from asr_amd.decoders import BeamCTCDecoder
    d = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)})
    out = torch.tensor([[[1, 6, 2, 0], [3, 0, 0, 0]]], dtype=torch.int32)
    lens = torch.tensor([[3, 0]], dtype=torch.int32)
    assert d.convert_to_strings(out, lens) == [["A B", ""]]
    offs = d.convert_tensor(out, lens)
    assert offs[0][0].tolist() == [1, 6, 2] and offs[0][1].numel() == 0 and offs[0][1].dtype == torch.int32


def test_workspace_query_without_device():
    from asr_amd import _lib
    lib = _lib.load()
    assert lib.ds2_ctc_beam_workspace_bytes(64, 501, 100) == 12 * 64 * 501 * 100
    assert lib.ds2_ctc_beam_workspace_bytes(1, 1, 1) == 12
    assert lib.ds2_ctc_beam_max_width() >= 256


def _ctc_nll(probs, label, blank):
    lp = torch.log(torch.as_tensor(probs, dtype=torch.float64)).unsqueeze(1)    # (T, 1, C)
    T = lp.shape[0]
    tgt = torch.tensor([list(label)], dtype=torch.long) if label else torch.zeros((1, 0), dtype=torch.long)
    return float(torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([len(label)]), blank=blank, reduction="none",
                                              zero_infinity=False)[0])


@pytest.mark.parametrize("T,C,blank,seed", [(1, 3, 0, 0), (3, 3, 0, 1), (4, 3, 2, 2), (4, 4, 0, 3), (5, 3, 1, 4)])
def test_oracle_exhaustive_matches_enumeration_and_ctc_loss(T, C, blank, seed):
    rng = np.random.default_rng(seed)
    probs = rng.dirichlet(np.ones(C), size=T)
    truth = O.brute_force_label_logprobs(probs, blank)
    K = len(truth) + 3
    res = O.beam_search(probs, None, blank, K, C, 1.0)
    assert len(res["beams"]) == len(truth)
    want = sorted(truth.items(), key=lambda kv: (-kv[1], len(kv[0]), kv[0]))
    for (pr, off, s), (wpr, ws) in zip(res["beams"], want):
        assert pr == wpr
        assert abs(s - ws) < 1e-12
        assert abs(-_ctc_nll(probs, pr, blank) - s) < 1e-10
        assert len(off) == len(pr) and list(off) == sorted(off)


def _one_hot(path, C):
    p = np.zeros((len(path), C))
    p[np.arange(len(path)), path] = 1.0
    return p


def test_oracle_one_hot_paths_and_offsets():
    for path, want, offs in (([1, 0, 1], (1, 1), (0, 2)), ([1, 1, 2], (1, 2), (0, 2)), ([1, 6, 2], (1, 6, 2), (0, 1, 2)),
                             ([0, 0, 3, 3, 0], (3,), (2,))):
        res = O.beam_search(_one_hot(path, 7), None, 0, 4, 7, 1.0)
        assert len(res["beams"]) == 1
        pr, off, s = res["beams"][0]
        assert pr == want and off == offs and s == 0.0


def test_oracle_offsets_keep_first_entry():
    # "A" enters at frame 0 and stays a beam: its offset stays 0 although frame 1 also emits A
    p = np.array([[0.1, 0.9, 0.0], [0.2, 0.8, 0.0]])
    res = O.beam_search(p, None, 0, 4, 3, 1.0)
    top = res["beams"][0]
    assert top[0] == (1,) and top[1] == (0,)
    assert abs(top[2] - math.log(0.9 * 0.8 + 0.1 * 0.8 + 0.9 * 0.2)) < 1e-12
    assert res["beams"][1][:2] == ((), ()) and abs(res["beams"][1][2] - math.log(0.1 * 0.2)) < 1e-12
    assert len(res["beams"]) == 2       # "AA" needs a blank between the two A's: probability 0, dropped


def test_oracle_tie_rule_on_quantised_probabilities():
    # equal probabilities: equal totals are ordered shorter first, then by the smaller label sequence; the class order is
    # probability descending, lower index first, which decides which equal-probability class a top-n cut keeps
    p = np.array([[0.25, 0.25, 0.25, 0.25]])
    res = O.beam_search(p, None, 0, 4, 4, 1.0)
    assert [b[0] for b in res["beams"]] == [(), (1,), (2,), (3,)]
    assert all(b[2] == math.log(0.25) for b in res["beams"])
    assert res["frame_margins"] == [math.inf] and res["final_gaps"] == [0.0, 0.0, 0.0]
    res = O.beam_search(p, None, 0, 2, 4, 1.0)
    assert [b[0] for b in res["beams"]] == [(), (1,)] and res["frame_margins"] == [0.0]
    res = O.beam_search(p, None, 0, 4, 2, 1.0)        # top-2: the blank and class 1
    assert [b[0] for b in res["beams"]] == [(), (1,)]
    p2 = np.array([[0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])
    res = O.beam_search(p2, None, 0, 3, 3, 1.0)
    assert [b[0] for b in res["beams"]] == [(1,), (2,), ()]       # P(A) = P(B) = 0.3125 > P() = 0.25
    assert res["beams"][0][2] == res["beams"][1][2] and abs(res["beams"][0][2] - math.log(0.3125)) < 1e-12
    assert O.decisive_ranks(res) == [2]


def test_oracle_cutoff_prob_and_sizes():
    p = np.array([[0.6, 0.3, 0.1]])
    kept, m = O.prune(p[0], 40, 0.85)
    assert kept.tolist() == [0, 1] and abs(m - 0.05) < 1e-12
    kept, _ = O.prune(p[0], 1, 1.0)
    assert kept.tolist() == [0]
    res = O.beam_search(p, 0, 0, 3, 40, 1.0)
    assert res["beams"] == [((), (), 0.0)]
    res = O.beam_search(p, None, 0, 3, 40, 0.5)            # only the blank survives the cutoff
    assert [b[0] for b in res["beams"]] == [()]
