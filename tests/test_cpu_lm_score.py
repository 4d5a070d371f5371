"""N-best rescoring without a GPU: ds2_lm_score_seq_host, the host twin of the LM scoring kernel (the same token and score routines run
serially), against the plain-Python restatement tests/lm_score_oracle.py; its refusals; and the pure host parts of tune_lm_weights
(grid bookkeeping, tie rule, the reference forms it accepts)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_lm_oracle as LO   # noqa: E402
import lm_score_oracle as SO   # noqa: E402
from lm_fixtures import random_arpa   # noqa: E402

CASES = [(mode, order) for mode in ("word", "char") for order in (1, 2, 3, 6)]


def make_lm(tmp_path, mode, order):
    """-> (NgramLM bound to SO.LABELS, NaiveLM of the same file)"""
    from asr_amd.decoders.lm import NgramLM
    vocab = SO.WORDS if mode == "word" else list("ABCD")          # character mode: the label E and the space are out of vocabulary
    path = random_arpa(str(tmp_path / f"{mode}{order}.arpa"), vocab, order, 60, seed=10 * order + (mode == "word"))
    lm = NgramLM(path, dict(enumerate(SO.LABELS)), SO.BLANK, SO.SPACE)
    assert lm.mode_name == mode and lm.order == order
    return lm, LO.NaiveLM(path)


def host_score(lm, labels, max_len=None, packed=None, C=None, blank=None, space=None):
    """ds2_lm_score_seq_host on one sequence -> (rc, lm_sum float32, n_tok, n_oov)"""
    from asr_amd import _lib
    lab = np.ascontiguousarray(np.asarray(labels, np.int32))
    packed = lm.packed if packed is None else packed
    s, nt, no = ctypes.c_float(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.load().ds2_lm_score_seq_host(packed.ctypes.data, packed.nbytes, lab.ctypes.data if len(lab) else None, len(lab),
                                           len(lab) if max_len is None else max_len, lm.space if space is None else space,
                                           lm.C if C is None else C, lm.blank if blank is None else blank, ctypes.byref(s),
                                           ctypes.byref(nt), ctypes.byref(no))
    return rc, np.float32(s.value), nt.value, no.value


def sequential_f32(lm, tokens):
    """the float32 sum, in token order, of NgramLM.score's values (the library's host scorer), OOV scores left out"""
    total = np.float32(0.0)
    for i, w in enumerate(tokens):
        s = np.float32(lm.score(tokens[max(0, i - (lm.order - 1)):i], w))
        if s != np.float32(LO.OOV):
            total = np.float32(total + s)
    return total


@pytest.mark.parametrize("mode,order", CASES)
def test_host_twin_matches_the_oracle(tmp_path, mode, order):
    lm, ref = make_lm(tmp_path, mode, order)
    seen_oov = seen_tok = 0
    for name, labels in SO.sequences(mode, order):
        want = SO.score_sequence(ref, SO.LABELS, SO.BLANK, SO.SPACE, labels)
        rc, got, nt, no = host_score(lm, labels)
        assert rc == 0 and (nt, no) == (want["n_tok"], want["n_oov"]), (name, nt, no, want["n_tok"], want["n_oov"])
        assert got.tobytes() == sequential_f32(lm, want["tokens"]).tobytes(), name
        assert abs(float(got) - want["lm_sum"]) <= SO.bound(ref, want), (name, float(got), want["lm_sum"], SO.bound(ref, want))
        seen_oov += no
        seen_tok = max(seen_tok, nt)
    assert seen_oov > 0 and seen_tok > 64


@pytest.mark.parametrize("mode,order", CASES)
def test_special_sequences(tmp_path, mode, order):
    lm, ref = make_lm(tmp_path, mode, order)
    by_name = dict(SO.sequences(mode, order))
    score = lambda labels: host_score(lm, labels)[1:]   # noqa: E731
    if mode == "word":
        # empty runs score nothing; the last run is scored with or without a space behind it
        assert score(by_name["leading"]) == score(by_name["plain"]) == score(by_name["trailing"])
        assert score(by_name["spaces"]) == (0.0, 0, 0) and score([]) == (0.0, 0, 0)
        assert score(by_name["doubled"]) == score(SO.spell("AB CAB DE"))
        # the context recovers `order` words behind an OOV word: the last two words are scored again
        s, nt, no = score(by_name["oov then in-vocabulary"])
        assert nt == order + 4 and no == min(order, order + 3) and no >= 1
        # the 70-label word is one in-vocabulary token; cut short it is none
        assert score(by_name["long word alone"])[1:] == (1, 0) and score(by_name["long word"])[1:] == (3, 0)
        assert score(by_name["long word cut"])[1:] == (2, 2 if order > 1 else 1)
        assert score(by_name["many short words"])[1:] == (70, 0) and score(by_name["many words"])[1] == 150
    else:
        assert score([]) == (0.0, 0, 0)
        s, nt, no = score(SO.spell("AB CD"))     # the space is a token, out of this model's vocabulary, and poisons order-1 contexts
        assert nt == 5 and no == min(order, 3)
        assert score(SO.spell("ABCD" * 40))[1:] == (160, 0)


@pytest.mark.parametrize("mode,order", [("word", 3), ("word", 1), ("char", 3), ("char", 6)])
def test_agrees_with_the_beam_contract(tmp_path, mode, order):
    """for an admissible labeling, alpha * (lm_sum - 1000 n_oov) + beta * n_tok is what the search adds (Fusion.labeling)"""
    lm, ref = make_lm(tmp_path, mode, order)
    alpha, beta = 0.7, -0.3
    fusion = LO.Fusion(ref, SO.LABELS, SO.BLANK, SO.SPACE, alpha, beta)
    n = 0
    for name, labels in SO.sequences(mode, order):
        want = fusion.labeling(tuple(labels))
        if want == -math.inf or len(labels) > 130:
            continue
        res = SO.score_sequence(ref, SO.LABELS, SO.BLANK, SO.SPACE, labels)
        _, got, nt, no = host_score(lm, labels)
        total = alpha * (float(got) + LO.OOV * no) + beta * nt
        assert abs(total - want) <= alpha * SO.bound(ref, res) + 1e-9 * max(1.0, abs(want)), (name, total, want)
        n += 1
    assert n >= 8


def test_refusals(tmp_path):
    from asr_amd import _lib
    lm, _ = make_lm(tmp_path, "word", 3)
    refused = lambda r: r[0] == 0 and math.isnan(r[1]) and r[2:] == (-1, -1)   # noqa: E731
    good = SO.spell("AB CAB")
    assert host_score(lm, good)[2] == 2
    assert refused(host_score(lm, good[:2] + [SO.BLANK] + good[2:]))          # the blank inside
    assert refused(host_score(lm, good + [7])) and refused(host_score(lm, [-1] + good))   # a label outside [0, C)
    assert refused(host_score(lm, good, max_len=len(good) - 1))               # len > max_len
    assert host_score(lm, good, max_len=len(good))[2] == 2
    # the header: magic, sizes, classes
    for field, value in ((0, 0x12345678), (2, 12345), (3, 0), (4, 0), (1, 9), (7, 5)):
        bad = lm.packed.copy()
        bad.view(np.int32)[field] = value
        rc = host_score(lm, good, packed=bad)[0]
        msg = _lib.load().ds2_last_error().decode()
        assert rc != 0 and msg.startswith("ds2_lm_score_seq_host: "), (field, rc, msg)
    assert host_score(lm, good, packed=lm.packed[:32].copy())[0] != 0        # cut short
    assert host_score(lm, good, packed=lm.packed[:lm.packed.nbytes - 4].copy())[0] != 0
    assert host_score(lm, good, C=lm.C + 1)[0] != 0 and "classes" in _lib.load().ds2_last_error().decode()
    assert host_score(lm, good, space=SO.BLANK)[0] != 0 and host_score(lm, good, space=-1)[0] != 0   # word mode needs its space
    assert host_score(lm, good, blank=lm.C)[0] != 0


def test_abi():
    import re

    from asr_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ds2hip.h")).read()
    for name in ("ds2_lm_score_seqs", "ds2_lm_score_seq_host", "ds2_nbest_sweep"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_lm_score_seqs"][1]) == 18 and len(_lib.SIGNATURES["ds2_nbest_sweep"][1]) == 16
    # what ds2_nbest_sweep refuses before any HIP call
    one = ctypes.c_void_p(8)
    ok = dict(ac=one, lm=one, nt=one, no=one, err=one, N=4, K=3, R=2, oov=-1000.0, al=one, Ga=2, be=one, Gb=2, pick=None, total=one, st=None)
    for v in (dict(K=0), dict(R=0), dict(R=65), dict(Ga=0), dict(Gb=0), dict(N=-1), dict(oov=math.nan), dict(al=None), dict(total=None),
              dict(err=None)):
        rc = lib.ds2_nbest_sweep(*dict(ok, **v).values())
        assert rc != 0 and lib.ds2_last_error().decode().startswith("ds2_nbest_sweep: "), v


def test_ops_refuse_host_tensors(tmp_path):
    import torch

    from asr_amd import ops
    lm, _ = make_lm(tmp_path, "word", 2)
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="lm_score: labels must be a GPU tensor"):
        ops.lm_score(z, z.long(), z, lm, 4)
    f = torch.zeros((2, 2))
    with pytest.raises(ValueError, match="nbest_sweep: ac must be a GPU tensor"):
        ops.nbest_sweep(f, f, f.int(), f.int(), torch.zeros((2, 2, 2), dtype=torch.int32), [0.0], [0.0])


def test_rescorer_arguments(tmp_path):
    from asr_amd.decoders import BeamCTCDecoder, GreedyDecoder, NBestRescorer
    labels = {c: i for i, c in enumerate(SO.LABELS)}
    lm, _ = make_lm(tmp_path, "word", 2)
    plain = BeamCTCDecoder(labels, beam_width=4)
    with pytest.raises(ValueError, match="no language model"):
        NBestRescorer(plain)
    with pytest.raises(ValueError, match="BeamCTCDecoder"):
        NBestRescorer(GreedyDecoder(labels), lm=lm)
    with pytest.raises(ValueError, match="acoustic"):
        NBestRescorer(plain, lm=lm, acoustic="fast")
    fused = BeamCTCDecoder(labels, lm_path=lm.path, alpha=0.5, beta=0.1, beam_width=4)
    with pytest.raises(ValueError, match="acoustic='beam'"):
        NBestRescorer(fused, acoustic="beam")
    with pytest.raises(ValueError, match="acoustic='beam'"):
        NBestRescorer(BeamCTCDecoder(labels, beam_width=4, hotwords=["CAB"]), lm=lm, acoustic="beam")
    assert NBestRescorer(fused).lm is fused.lm and NBestRescorer(plain, lm=lm.path).lm.order == 2
    assert NBestRescorer(plain, lm=lm, acoustic="beam").acoustic == "beam"
    with pytest.raises(ValueError, match="oov_score"):
        NBestRescorer(plain, lm=lm, oov_score=math.nan)


def test_tune_summary_bookkeeping():
    from asr_amd.decoders import _reference_strings, tune_summary
    alphas, betas = [0.0, 0.5, 1.0], [-1.0, 0.0]
    total = np.array([[[5, 9], [4, 9]], [[2, 8], [2, 7]], [[2, 6], [3, 5]]], np.int64)
    out = tune_summary(total, 20, 50, alphas, betas, "wer", first_pass=(5, 10), oracle=(1, 2))
    assert (out["alpha"], out["beta"]) == (0.5, -1.0)            # three cells tie at 2 word errors: the first in row-major order
    assert out["wer"] == 10.0 and out["cer"] == 16.0
    assert out["grid_wer"].shape == (3, 2) and out["grid_wer"][0, 1] == 20.0 and out["grid_cer"][2, 1] == 10.0
    assert out["first_pass"] == (25.0, 20.0) and out["oracle"] == (5.0, 4.0)
    out = tune_summary(total, 20, 50, alphas, betas, "cer")
    assert (out["alpha"], out["beta"], out["cer"]) == (1.0, 0.0, 10.0)
    assert tune_summary(total * 0, 0, 0, alphas, betas)["wer"] == 0.0     # no reference token: divides as 1
    for bad in (dict(metric="ser"), dict(alphas=[]), dict(betas=[math.nan])):
        with pytest.raises(ValueError):
            tune_summary(**dict(dict(total=total, ref_words=20, ref_chars=50, alphas=alphas, betas=betas), **bad))
    with pytest.raises(ValueError, match="grid"):
        tune_summary(total[:2], 20, 50, alphas, betas)
    # references: plain strings, or evaluate()'s output_data form
    assert _reference_strings(["AB CAB", "DE"]) == _reference_strings([["AB CAB"], ["DE"]]) == ["AB CAB", "DE"]
    with pytest.raises(ValueError):
        _reference_strings([["AB", "CAB"]])
