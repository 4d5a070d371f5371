"""BeamCTCDecoder with an n-gram language model, without a GPU: ARPA parsing and its errors, mode detection, the KenLM binary
refusal, the library's packed tables and host scorer against the naive restatement tests/ctc_beam_lm_oracle.py, the dictionary,
and that restatement against brute-force enumeration."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_lm_oracle as LO   # noqa: E402
import ctc_beam_oracle as O   # noqa: E402
from lm_fixtures import random_arpa, write_arpa   # noqa: E402

LABELS = "_ABCDE "   # index 0 is the blank, 6 the space
WORDS = ["A", "AB", "BAD", "CAB", "DE", "EDA", "Z"]   # "Z" has no label: not in the dictionary


def _word_lm(tmp_path, seed=0, order=3, name="w.arpa"):
    return random_arpa(str(tmp_path / name), WORDS, order, 40, seed)


def _char_lm(tmp_path, seed=0, order=3, name="c.arpa", chars="ABCDE"):
    return random_arpa(str(tmp_path / name), list(chars), order, 40, seed)


def test_arpa_edge_cases(tmp_path):
    from asr_amd.decoders.lm import ArpaError, read_arpa
    secs = [[(("<s>",), -99, -0.5), (("</s>",), -1.0, None), (("A",), -0.7, None), (("B",), -0.9, -0.2)],
            [(("<s>", "A"), -0.3, None), (("A", "B"), -0.4, None)]]
    order, ng = read_arpa(write_arpa(str(tmp_path / "a.arpa"), secs))
    assert order == 2 and [len(s) for s in ng] == [4, 2]
    assert ng[0][0] == (("<s>",), -99.0, -0.5) and ng[0][2] == (("A",), -0.7, 0.0)   # missing backoff column -> 0
    order_gz, ng_gz = read_arpa(write_arpa(str(tmp_path / "a.arpa.gz"), secs, gz=True))
    assert (order_gz, ng_gz) == (order, ng)
    with pytest.raises(ArpaError, match="declares"):
        read_arpa(write_arpa(str(tmp_path / "bad.arpa"), secs, counts=[4, 3]))
    with pytest.raises(ArpaError, match="order 7"):
        read_arpa(write_arpa(str(tmp_path / "o7.arpa"), [secs[0]] + [[]] * 6))
    p = tmp_path / "noend.arpa"
    p.write_text(open(write_arpa(str(tmp_path / "x.arpa"), secs)).read().replace("\\end\\", ""))
    with pytest.raises(ArpaError, match="end"):
        read_arpa(str(p))
    p = tmp_path / "junk.arpa"
    p.write_text("\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0 A B C D\n\\end\\\n")
    with pytest.raises(ArpaError):
        read_arpa(str(p))
    p.write_text("hello\n")
    with pytest.raises(ValueError):
        read_arpa(str(p))


def test_mode_detection(tmp_path):
    from asr_amd.decoders.lm import MODE_CHAR, MODE_WORD, NgramLM, detect_mode
    assert detect_mode({"<s>", "</s>", "<unk>", "a", "b"}) == MODE_CHAR
    assert detect_mode({"<s>", "a", "ab"}) == MODE_WORD
    kana = [chr(0x3041 + i) for i in range(20)]
    assert detect_mode(set(kana) | {"<s>", "</s>"}) == MODE_CHAR
    labels = {chr(0x3041 + i) if i else "_": i for i in range(21)}
    from asr_amd.decoders import BeamCTCDecoder
    d = BeamCTCDecoder(labels, lm_path=_char_lm(tmp_path, chars=kana, name="kana.arpa"), alpha=0.8, beta=1)
    assert d.lm.mode == MODE_CHAR and d.lm.label_tok[1] == d.lm.vocab[chr(0x3042)]
    w = NgramLM(_word_lm(tmp_path), dict(enumerate(LABELS)), 0, 6)
    assert w.mode == MODE_WORD
    with pytest.raises(ValueError, match="space"):   # word mode needs a space label
        BeamCTCDecoder(labels, lm_path=_word_lm(tmp_path, name="w2.arpa"))


def test_kenlm_binary_is_refused(tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    for name in ("missing.binary", "missing.klm"):   # refused before the file is looked for
        with pytest.raises(NotImplementedError):
            BeamCTCDecoder(LABELS, lm_path=str(tmp_path / name))
    p = tmp_path / "model.arpa"
    p.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0")
    with pytest.raises(NotImplementedError):
        BeamCTCDecoder(LABELS, lm_path=str(p))


@pytest.mark.parametrize("mode,order", [("word", 3), ("word", 1), ("char", 4), ("char", 6)])
def test_host_score_matches_naive_backoff(tmp_path, mode, order):
    from asr_amd.decoders.lm import NgramLM
    path = _word_lm(tmp_path, seed=order, order=order) if mode == "word" else _char_lm(tmp_path, seed=order, order=order)
    lm = NgramLM(path, dict(enumerate(LABELS)), 0, 6)
    ref = LO.NaiveLM(path)
    assert lm.order == ref.order == order
    queries = [(list(k[:-1]), k[-1]) for k in ref.table]
    rng = np.random.default_rng(order)
    toks = sorted(ref.vocab - {"</s>"}) + ["OOV1"]
    for _ in range(1000):
        h = [toks[i] for i in rng.integers(0, len(toks), size=int(rng.integers(0, order)))]
        queries.append((h, toks[int(rng.integers(0, len(toks)))]))
    n_oov = 0
    for h, w in queries:
        want = ref.score(h, w)
        n_oov += want == LO.OOV
        assert abs(lm.score(h, w) - want) <= 1e-6 * max(1.0, abs(want)), (h, w)
    assert n_oov > 0


def test_dictionary_membership(tmp_path):
    from asr_amd.decoders.lm import NgramLM
    lm = NgramLM(_word_lm(tmp_path), dict(enumerate(LABELS)), 0, 6)
    assert all(lm.in_dictionary(w) for w in WORDS if w != "Z")
    assert not lm.in_dictionary("Z") and not lm.in_dictionary("<s>") and not lm.in_dictionary("ABC")
    f = LO.Fusion(LO.NaiveLM(_word_lm(tmp_path)), LABELS, 0, 6, 1.0, 0.5)
    assert f.dictionary == lm.dictionary
    assert f.bonus((), 6) == -math.inf and f.bonus((1,), 2) == 0.0 and f.bonus((1, 2), 3) == -math.inf
    assert f.bonus((1, 6), 6) == -math.inf and f.bonus((2,), 6) == -math.inf and f.bonus((1, 2), 6) > -math.inf
    assert f.end((2, 1)) == LO.OOV + 0.5 and f.end((1, 2, 6)) == 0.0


def _fusion(tmp_path, mode, seed, alpha, beta, chars=LABELS):
    path = _word_lm(tmp_path, seed=seed, name=f"w{seed}.arpa") if mode == "word" else _char_lm(tmp_path, seed=seed, name=f"c{seed}.arpa")
    space = chars.index(" ") if " " in chars else None
    return LO.Fusion(LO.NaiveLM(path), chars, 0, space, alpha, beta)


@pytest.mark.parametrize("mode", ["word", "char"])
@pytest.mark.parametrize("T,C,seed", [(3, 3, 0), (4, 4, 1), (5, 5, 2), (6, 3, 3), (6, 4, 4)])
def test_oracle_matches_brute_force(tmp_path, mode, T, C, seed):
    """with an unbounded beam and no cutoff the search's best beam is the best admissible labeling"""
    chars = "_AB " if C == 4 and mode == "word" else ("_A " if C == 3 and mode == "word" else LABELS[:C - 1] + " ")
    rng = np.random.default_rng(seed)
    probs = rng.dirichlet(np.ones(C) * 0.7, size=T)
    for alpha, beta in ((0.8, 1.0), (2.0, -0.5)):
        f = _fusion(tmp_path, mode, seed, alpha, beta, chars)
        want = LO.brute_force_best(probs, f, 0)
        res = LO.beam_search(probs, f, None, 0, 10 ** 6, C, 1.0)
        assert want is not None and res["beams"], (mode, T, C)
        pr, _, s = res["beams"][0]
        assert pr == want[0] and abs(s - want[1]) < 1e-9, (pr, s, want)
        # every surviving beam's total is its labeling's probability plus its terms
        truth = O.brute_force_label_logprobs(probs, 0)
        for pr, _, s in res["beams"]:
            assert abs(s - truth[pr] - f.labeling(pr)) < 1e-9


@pytest.mark.parametrize("K,top_n,cut,blank", [(1, 40, 1.0, 0), (4, 3, 1.0, 0), (16, 40, 0.9, 0), (100, 40, 1.0, 2)])
def test_oracle_without_lm_weight_is_plain_beam_search(tmp_path, K, top_n, cut, blank):
    f = _fusion(tmp_path, "char", 7, 0.0, 0.0)
    rng = np.random.default_rng(K)
    probs = rng.dirichlet(np.ones(7) * 0.5, size=12)
    a = LO.beam_search(probs, f, None, blank, K, top_n, cut)["beams"]
    b = O.beam_search(probs, None, blank, K, top_n, cut)["beams"]
    assert [x[0] for x in a] == [x[0] for x in b] and [x[1] for x in a] == [x[1] for x in b]
    assert all(abs(x[2] - y[2]) < 1e-12 for x, y in zip(a, b))


def test_packed_size_query_and_grid_limit():
    from asr_amd import _lib
    lib = _lib.load()
    assert lib.ds2_ctc_beam_lm_max_candidates() == 4096
    assert lib.ds2_ctc_lm_packed_bytes(3, 10, 4, 5, 29) > 0
    assert lib.ds2_ctc_lm_packed_bytes(7, 10, 4, 5, 29) == 0
    assert 100 * (min(40, 28) + 2) <= lib.ds2_ctc_beam_lm_max_candidates()   # K = 100 at C = 29 fits


def test_decoder_keeps_lm_arguments(tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    d = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, lm_path=_word_lm(tmp_path), alpha=0.8, beta=1, beam_width=10)
    assert (d.alpha, d.beta, d.beam_width) == (0.8, 1, 10) and d.lm.mode_name == "word" and d.lm.space == 6
    assert d.lm.packed.nbytes > 0 and list(itertools.islice(d.lm.vocab, 2)) == ["<s>", "</s>"]
