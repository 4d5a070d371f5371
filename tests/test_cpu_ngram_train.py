"""The n-gram estimator without a GPU: the fp64 restatement (tests/ngram_train_oracle.py) against itself and a brute-force Counter, the
library's host twin (ds2_ngram_estimate_host, ops.ngram_estimate_host) against the restatement, and the written ARPA file read back
through NgramLM.  tests/test_gpu_ngram_train.py holds the kernels to the host twin with `compare` below."""
import gzip
import math
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ngram_train_oracle as O   # noqa: E402
from lm_fixtures import random_arpa   # noqa: E402

REL = 1e-12              # p and gamma: both sides evaluate the same fp64 formulas from equal integers, about 50 ulp at the worst
LN10 = math.log(10.0)

CORPORA = {"tiny": (lambda: O.TINY, 3), "zipf": (lambda: O.zipf_corpus(1), 3), "char": (lambda: O.char_corpus(1), 5)}
_models = {}


def corpus(name):
    """(sentences, order, the restatement's model), computed once"""
    if name not in _models:
        make, N = CORPORA[name]
        sents = make()
        _models[name] = (sents, N, O.estimate(sents, N))
    return _models[name]


def keys_to_grams(raw, vocab, n):
    keys, b = raw["orders"][n - 1][0], raw["bits"]
    mask = np.uint64((1 << b) - 1)
    cols = [((keys >> np.uint64(b * (n - 1 - j))) & mask).astype(np.int64) for j in range(n)]
    return [tuple(vocab[int(c[r])] for c in cols) for r in range(len(keys))]


def compare(raw, m, vocab):
    """an ops.ngram_estimate / ngram_estimate_host dictionary against the restatement's model: every n-gram in file order, every count,
    adjusted count and count-of-counts to the integer, every p, backoff and discount within relative REL"""
    assert raw["order"] == m.N and raw["fallback_orders"] == m.fallback_orders
    assert raw["count_of_counts"].tolist() == [m.t[n] for n in range(1, m.N + 1)]
    for n in range(1, m.N + 1):
        for k in (1, 2, 3):
            assert abs(raw["discounts"][n - 1][k - 1] - m.D[n][k]) <= REL * max(1.0, abs(m.D[n][k])), (n, k)
    assert abs(raw["unk_log10"] - math.log10(m.unk_p)) * LN10 <= REL
    want = O.listing(m)
    for n in range(1, m.N + 1):
        sec = want[n - 1][1:] if n == 1 else want[n - 1]
        _, count, adjusted, lp, lb = raw["orders"][n - 1]
        grams = keys_to_grams(raw, vocab, n)
        assert grams == [g for g, _, _ in sec], n
        assert count.tolist() == [m.c[n][g] for g in grams], n
        assert adjusted.tolist() == [m.a[n][g] for g in grams], n
        for r, (g, p, b) in enumerate(sec):
            assert abs(lp[r] - p) * LN10 <= REL, (g, lp[r], p)                       # (relative error of p = ln 10 * error of log10 p)
            assert (b is None and math.isnan(lb[r])) or (b is not None and abs(lb[r] - b) * LN10 <= REL), (g, lb[r], b)


def host(sentences, N, **kw):
    from asr_amd import ops
    vocab, flat, off = O.to_ids(sentences)
    return ops.ngram_estimate_host(flat, off, len(vocab), N, **kw), vocab


# ---- the restatement -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CORPORA))
def test_oracle_distributions_sum_to_one(name):
    _, _, m = corpus(name)
    sums = O.distribution_sums(m)
    assert len(sums) == len(O.contexts(m))
    assert max(abs(v - 1.0) for v in sums.values()) <= 1e-12
    rng = np.random.default_rng(0)                                    # and word by word, on the empty context and a sample of the others
    hs = [()] + [list(sums)[i] for i in rng.choice(len(sums), size=min(12, len(sums)), replace=False)]
    for h in hs:
        assert abs(O.distribution_sum(m, h) - 1.0) <= 1e-12, h


def test_oracle_fallbacks():
    assert corpus("zipf")[2].fallback_orders == []                    # the closed form is exercised in all three orders
    assert corpus("char")[2].fallback_orders != []                    # 26 tokens: the unigram count-of-counts has zeros
    assert all(0.0 < d <= k for n in (1, 2, 3) for k, d in enumerate(corpus("zipf")[2].D[n][1:], 1))


@pytest.mark.parametrize("sents,N", [(O.TINY, 3), (O.zipf_corpus(2, n_words=30, n_sent=60, max_len=6), 4)])
def test_oracle_counts_match_brute_force(sents, N):
    m = O.estimate(sents, N)
    text = [["<s>"] + list(s) + ["</s>"] for s in sents if s]
    for n in range(1, N + 1):
        c = Counter(tuple(t[i:i + n]) for t in text for i in range(len(t) - n + 1))
        assert c == m.c[n]
        bigger = Counter(tuple(t[i:i + n + 1]) for t in text for i in range(len(t) - n))
        for g in c:
            if n == N or (n >= 2 and g[0] == "<s>"):
                want = c[g]
            elif g == ("<s>",):
                want = 0
            else:
                want = len({x[0] for x in bigger if x[1:] == g})
            assert m.a[n][g] == want, g


# ---- the host twin ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CORPORA))
def test_host_twin_matches_oracle(name):
    sents, N, m = corpus(name)
    raw, vocab = host(sents, N)
    compare(raw, m, vocab)


@pytest.mark.parametrize("N", [1, 2, 6])
def test_host_twin_orders_and_short_sentences(N):
    sents = [[], ["a"], ["b", "a"], [], ["a", "b", "c"], ["c"], ["a", "b", "a", "b", "c", "a", "b"], []]     # empty, and shorter than N - 1
    m = O.estimate(sents, N)
    raw, vocab = host(sents, N)
    compare(raw, m, vocab)
    assert m.n_empty == 3 and m.a[1][("<s>",)] == 0 and m.c[1][("<s>",)] == 5
    assert raw["orders"][0][2][0] == 0                                    # a_1(<s>) = 0, at N = 1 as well
    assert abs(max(abs(v - 1.0) for v in O.distribution_sums(m).values())) <= 1e-12


def test_sentence_boundaries_and_bos_counts():
    raw, vocab = host([["a", "b"], ["c", "d"]], 3)
    bigrams = keys_to_grams(raw, vocab, 2)
    assert ("b", "c") not in bigrams and ("b", "</s>") in bigrams and ("<s>", "c") in bigrams
    assert all(("</s>" not in g[:-1]) and ("<s>" not in g[1:]) for n in (2, 3) for g in keys_to_grams(raw, vocab, n))
    # <s>-initial n-grams below the top order keep their raw counts: "<s> a" occurs three times but has one left extension at most
    sents = [["a", "b"], ["a", "b"], ["a", "c"], ["b", "a"]]
    raw, vocab = host(sents, 3)
    grams = keys_to_grams(raw, vocab, 2)
    _, count, adjusted, _, _ = raw["orders"][1]
    i, j = grams.index(("<s>", "a")), grams.index(("a", "b"))
    assert (count[i], adjusted[i]) == (3, 3) and (count[j], adjusted[j]) == (2, 1)


def test_discount_fallback_is_taken():
    raw, vocab = host(O.TINY, 3, discount_fallback=(0.25, 0.5, 0.75))
    m = O.estimate(O.TINY, 3, fallback=(0.25, 0.5, 0.75))
    assert raw["fallback_orders"] == [1, 2, 3] and raw["discounts"].tolist() == [[0.25, 0.5, 0.75]] * 3
    compare(raw, m, vocab)


def test_refusals():
    from asr_amd import ops
    from asr_amd.decoders import lm_train
    flat, off = np.array([3, 4, 3], np.int32), np.array([0, 3], np.int64)
    for bad in (0, 7, 2.5, True):
        with pytest.raises(ValueError, match="order"):
            ops.ngram_estimate_host(flat, off, 5, bad)
        with pytest.raises(ValueError, match="order"):
            lm_train.estimate_ngram(["a b"], order=bad, device="cpu")
    # 70 000 ids need 17 bits a token: order 3 fits the 64-bit key, order 4 does not, and the refusal says so
    assert lm_train.max_order(70000) == 3 and lm_train.max_order(65536) == 4 and lm_train.max_order(29) == 6 and lm_train.max_order(2049) == 5
    with pytest.raises(ValueError, match="admits order 3 at most"):
        ops.ngram_estimate_host(flat, off, 70000, 4)
    with pytest.raises(ValueError, match="U\\+2581"):
        lm_train.estimate_ngram(["AB"], mode="char", labels="_AB▁", device="cpu")
    with pytest.raises(ValueError, match="offsets"):
        ops.ngram_estimate_host(flat, np.array([0, 2], np.int64), 5, 2)
    with pytest.raises(Exception, match="outside"):
        ops.ngram_estimate_host(np.array([3, 9], np.int32), np.array([0, 2], np.int64), 5, 2)
    with pytest.raises(ValueError, match="no token"):
        lm_train.estimate_ngram(["", "  "], device="cpu")
    with pytest.raises(ValueError, match="outside the labels"):
        lm_train.estimate_ngram(["ABC"], mode="char", labels="_AB ", unknown="error", device="cpu")
    with pytest.raises(ValueError, match="reserved"):
        lm_train.estimate_ngram(["a <s> b"], device="cpu")


# ---- tokenisation, the file, the loader --------------------------------------------------------------------------------

def test_tokenize():
    from asr_amd.decoders.lm_train import tokenize
    vocab, flat, off, n_empty = tokenize(["b a", "", "  a\tc ", " "], "word")
    assert vocab == ["<unk>", "<s>", "</s>", "a", "b", "c"] and flat.tolist() == [4, 3, 3, 5] and off.tolist() == [0, 2, 2, 4, 4]
    assert n_empty == 2
    vocab, flat, off, n_empty = tokenize(["A B", "xA"], "char", labels="_AB ")
    assert vocab == ["<unk>", "<s>", "</s>", "A", "B", "▁"] and flat.tolist() == [3, 5, 4, 3] and off.tolist() == [0, 3, 4]
    vocab, flat, _, _ = tokenize(["A B"], "char", labels="_AB")        # no space label: the space is dropped like any other character
    assert vocab[3:] == ["A", "B"] and flat.tolist() == [3, 4]


def lm_of(path, labels):
    from asr_amd.decoders.lm import NgramLM
    space = labels.index(" ") if " " in labels else None
    return NgramLM(str(path), dict(enumerate(labels)), 0, space)


@pytest.mark.parametrize("name,gz", [("tiny", False), ("zipf", True), ("char", False)])
def test_written_file_scores_as_the_oracle(tmp_path, name, gz):
    from asr_amd.decoders.lm_train import estimate_ngram
    sents, N, m = corpus(name)
    est = estimate_ngram([" ".join(s) for s in sents], order=N, mode="word", device="cpu")
    assert (est.order, est.mode, est.vocab, est.fallback_orders) == (N, "word", m.vocab, m.fallback_orders)
    assert (est.n_sentences, est.n_empty, est.n_tokens) == (len(sents), m.n_empty, sum(len(s) for s in sents))
    assert [len(sec[0]) for sec in est.ngrams] == [len(m.c[n]) for n in range(1, N + 1)]
    path = est.write_arpa(tmp_path / ("m.arpa.gz" if gz else "m.arpa"))
    if gz:
        with gzip.open(path, "rt", encoding="utf-8") as f:
            assert f.readline() == "\n" and f.readline() == "\\data\\\n"
    lm = lm_of(path, "_ ")                                               # (a word-level model needs a space label and nothing else here)
    assert lm.order == N and list(lm.vocab) == m.vocab
    rng = np.random.default_rng(1)
    want = O.listing(m)
    # listed n-grams of full-length or <s>-initial contexts: the file's number, rounded once to fp32 (|log10 p| < 8: half an ulp is
    # 2^-22; the 8 decimals of the text add 5e-9)
    for n in range(1, N + 1):
        if n == 1 and N > 1:
            continue                                                     # (a 1-gram is reached through backoffs only: the sums cover it)
        sec = [(g, p) for g, p, _ in want[n - 1] if g != ("<s>",) and (n == N or g[0] == "<s>")]   # score() pads a context with <s>
        for i in rng.choice(len(sec), size=min(200, len(sec)), replace=False):
            g, p = sec[int(i)]
            assert abs(p) < 8 and abs(lm.score(g[:-1], g[-1]) - p) <= 2.0 ** -22 + 1e-8, g
    # the distributions the file holds: every looked-up value carries at most N + 1 fp32 roundings at magnitudes below 8
    bound = 2 * (N + 1) * 2.0 ** -21 * LN10
    ctx = [h for h in O.contexts(m) if len(h) == N - 1 or (h and h[0] == "<s>")]   # (score() pads a shorter context with <s>)
    words = [w for w in m.vocab if w != "<s>"]
    per_ctx = max(1, 40000 // len(words))
    for i in rng.choice(len(ctx), size=min(per_ctx, len(ctx)), replace=False):
        h = ctx[int(i)]
        total = math.fsum(10.0 ** lm.score(h, w) for w in words)
        assert abs(total - 1.0) <= bound, (h, total)


def test_space_token_mapping(tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    d = BeamCTCDecoder("_AB ")
    est = d.fit_lm(["AB A", "B A", "A B AB"], order=2, mode="char", path=str(tmp_path / "c.arpa"), device="cpu")
    assert est.mode == "char" and "▁" in est.vocab and d.lm.mode_name == "char" and d.lm_path == str(tmp_path / "c.arpa")
    assert d.lm.label_tok.tolist() == [-1, d.lm.vocab["A"], d.lm.vocab["B"], d.lm.vocab["▁"]]
    m = O.estimate([list(s.replace(" ", "▁")) for s in ("AB A", "B A", "A B AB")], 2)
    assert abs(d.lm.score(("A",), "▁") - math.log10(m.p[2][("A", "▁")])) <= 2.0 ** -22 + 1e-8            # a token, not OOV (-1000)
    # defaults: word mode with a space label, character mode without one; a temporary file leaves no path behind
    assert d.fit_lm(["AB A", "B A"], device="cpu").mode == "word" and d.lm.mode_name == "word" and d.lm_path is None
    assert d.lm.in_dictionary("AB") and not d.lm.in_dictionary("BA")
    e = BeamCTCDecoder("_AB")
    assert e.fit_lm(["AB A", "B A"], order=2, alpha=0.5, beta=1.5, device="cpu").mode == "char" and (e.alpha, e.beta) == (0.5, 1.5)
    assert "▁" not in e.lm.vocab


def test_models_without_the_space_token_load_as_before(tmp_path):
    path = random_arpa(str(tmp_path / "c.arpa"), "ABCDE", 3, 40, seed=3)
    lm = lm_of(path, "_ABCDE ")
    assert lm.mode_name == "char"
    assert lm.label_tok.tolist() == [-1] + [lm.vocab[c] for c in "ABCDE"] + [-1]     # the space label stays out of the vocabulary


def test_model_fit_lm_reads_the_manifest(tmp_path):
    import pandas as pd
    from asr_amd.decoders import BeamCTCDecoder, GreedyDecoder
    from asr_amd.modules.deepspeech import DeepSpeech
    pd.DataFrame({"audio_filepath": ["a.wav", "b.wav", "c.wav"], "text": ["AB A", "B A", None]}).to_csv(tmp_path / "m.csv", index=False)
    model = DeepSpeech.__new__(DeepSpeech)                               # fit_lm touches the decoder only
    object.__setattr__(model, "decoder", BeamCTCDecoder("_AB "))
    est = DeepSpeech.fit_lm(model, str(tmp_path / "m.csv"), order=2, device="cpu")
    assert (est.n_sentences, est.n_empty, est.mode) == (3, 1, "word") and model.decoder.lm.in_dictionary("AB")
    object.__setattr__(model, "decoder", GreedyDecoder("_AB "))
    with pytest.raises(ValueError, match="BeamCTCDecoder"):
        DeepSpeech.fit_lm(model, str(tmp_path / "m.csv"))
