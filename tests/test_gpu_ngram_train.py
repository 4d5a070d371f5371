"""-m gpu: the n-gram estimation kernels (ds2_ngram_count / _adjust / _probs, ops.ngram_estimate) against their host twin, which
tests/test_cpu_ngram_train.py holds to the fp64 restatement: every key, count, adjusted count and count-of-counts to the integer, every
log10 p, backoff and discount within the same relative 1e-12; and BeamCTCDecoder.fit_lm through the search.  MI355X figures are in
profiles/ngram_train_timing.txt."""
import math

import numpy as np
import pytest
import torch

import ngram_train_oracle as O
from test_cpu_ngram_train import LN10, REL, compare, corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def on_device(dev, flat, off, n_vocab, N, **kw):
    from asr_amd import ops
    return ops.ngram_estimate(torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev), n_vocab, N, **kw)


def same(got, want):
    """two estimator dictionaries: integers equal, fp64 values within relative REL (of p and gamma: ln 10 times the error of a log10)"""
    assert (got["order"], got["bits"], got["fallback_orders"]) == (want["order"], want["bits"], want["fallback_orders"])
    assert got["count_of_counts"].tolist() == want["count_of_counts"].tolist()
    assert np.all(np.abs(got["discounts"] - want["discounts"]) <= REL * np.maximum(1.0, np.abs(want["discounts"])))
    assert abs(got["unk_log10"] - want["unk_log10"]) * LN10 <= REL
    for n, (g, w) in enumerate(zip(got["orders"], want["orders"]), 1):
        for j in range(3):
            assert g[j].dtype == w[j].dtype and np.array_equal(g[j], w[j]), (n, j)
        assert np.all(np.abs(g[3] - w[3]) * LN10 <= REL), n
        assert np.array_equal(np.isnan(g[4]), np.isnan(w[4])) and np.all(np.abs(np.nan_to_num(g[4]) - np.nan_to_num(w[4])) * LN10 <= REL), n


def random_sentences(seed, ids, n_tokens, max_len):
    """flat ids drawn from `ids` with Zipf weights, cut into sentences of 0..max_len tokens (empty ones included)"""
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids, dtype=np.int32)
    w = 1.0 / (np.arange(len(ids)) + 1.0)
    flat = ids[rng.choice(len(ids), size=n_tokens, p=w / w.sum())]
    cuts = [0]
    while cuts[-1] < n_tokens:
        cuts.append(min(n_tokens, cuts[-1] + int(rng.integers(0, max_len + 1))))
    return np.ascontiguousarray(flat), np.array(cuts, dtype=np.int64)


def shape(name):
    """(flat ids, offsets, n_vocab, order) of the further shapes"""
    if name == "blocks":            # 131 072 tokens of V = 29 at order 6: every block and grid boundary of the launches
        return (*random_sentences(5, range(3, 29), 131072, 60), 29, 6)
    if name == "repeated":          # one sentence 10 000 times: every lane of the machine on a handful of keys
        sent = np.array([3, 4, 5, 3, 4], np.int32)
        return np.tile(sent, 10000), np.arange(10001, dtype=np.int64) * 5, 6, 3
    if name == "strided":           # ids that are all multiples of 256 (run with every table at its minimum of slots)
        return (*random_sentences(6, range(256, 65536, 256), 3000, 9), 65536, 3)
    if name == "full key":          # n_vocab = 65 536 at order 4: 16 bits a token, the key uses all 64, its top bit included
        return (*random_sentences(7, [65535, 3, 40000, 32768, 17, 65534], 2000, 7), 65536, 4)
    if name == "one token":
        return np.array([3], np.int32), np.array([0, 1], np.int64), 4, 3
    raise KeyError(name)


@pytest.mark.parametrize("name", ["tiny", "zipf", "char"])
def test_kernels_match_host_twin_and_oracle(dev, name):
    from asr_amd import ops
    sents, N, m = corpus(name)
    vocab, flat, off = O.to_ids(sents)
    got = on_device(dev, flat, off, len(vocab), N)
    same(got, ops.ngram_estimate_host(flat, off, len(vocab), N))
    compare(got, m, vocab)


@pytest.mark.parametrize("name", ["blocks", "repeated", "strided", "full key", "one token"])
def test_kernels_match_host_twin_on_shapes(dev, name):
    from asr_amd import ops
    flat, off, n_vocab, N = shape(name)
    want = ops.ngram_estimate_host(flat, off, n_vocab, N)
    slots = None
    if name == "strided":           # the smallest power of two that holds each order's distinct n-grams: the longest probe chains
        slots = [max(2, 1 << (len(sec[0]) - 1).bit_length()) for sec in want["orders"]]
        assert all(2 * len(sec[0]) > s for sec, s in zip(want["orders"], slots))
    if name == "full key":
        assert int(want["orders"][3][0].max()) >> 63 == 1 and want["bits"] * N == 64
    same(on_device(dev, flat, off, n_vocab, N, slots=slots), want)


def test_flags_raise(dev):
    from asr_amd import _lib
    flat, off, n_vocab, N = shape("strided")
    with pytest.raises(_lib.DS2LibraryError, match="overflowed"):          # a full table ends its probes and reports; it is no retry path
        on_device(dev, flat, off, n_vocab, N, slots=[4, 4, 4])
    with pytest.raises(_lib.DS2LibraryError, match="token id outside"):
        on_device(dev, np.array([3, 9, 4], np.int32), np.array([0, 3], np.int64), 5, 2)


def test_two_runs_write_the_same_bytes(dev, tmp_path):
    from asr_amd.decoders.lm_train import estimate_ngram
    text = ["".join(s) for s in corpus("char")[0]]
    files = []
    for i in range(2):
        est = estimate_ngram(text, order=5, mode="char", device=dev)
        files.append(open(est.write_arpa(tmp_path / f"run{i}.arpa"), "rb").read())
    assert files[0] == files[1] and len(files[0]) > 100000
    assert est.fallback_orders == corpus("char")[2].fallback_orders


def test_fit_lm_decodes_as_the_written_file(dev, tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    labels = "_ABC "
    sentences = ["AB CA", "CA AB B", "B AB", "CAB AB", "AB"]
    fitted = BeamCTCDecoder(labels, beam_width=20)
    est = fitted.fit_lm(sentences, order=3, path=str(tmp_path / "w.arpa"), alpha=1.5, beta=0.5, device=dev)
    assert est.mode == "word" and fitted.lm is not None and (fitted.alpha, fitted.beta) == (1.5, 0.5)
    loaded = BeamCTCDecoder(labels, lm_path=str(tmp_path / "w.arpa"), alpha=1.5, beta=0.5, beam_width=20)
    probs = torch.softmax(2.0 * torch.randn(3, 14, len(labels), generator=torch.Generator().manual_seed(4)), dim=-1).to(dev)
    a, _ = fitted.decode(probs)
    b, _ = loaded.decode(probs)
    assert a == b and fitted.last_scores.numpy().tobytes() == loaded.last_scores.numpy().tobytes()
    assert any(s for s in a[0])


def test_fitted_model_prefers_the_spelling_of_the_corpus(dev):
    from asr_amd.decoders import BeamCTCDecoder
    labels = "_AB"                                                        # no space label: fit_lm takes character mode
    # the first label is surely A; the second is A at 0.55 against B at 0.43, with a blank frame between them
    probs = torch.tensor([[[0.01, 0.98, 0.01], [0.98, 0.01, 0.01], [0.02, 0.55, 0.43]]], device=dev)
    plain = BeamCTCDecoder(labels, beam_width=10)
    assert plain.decode(probs)[0][0][0] == "AA"
    fitted = BeamCTCDecoder(labels, beam_width=10, alpha=2.0)
    est = fitted.fit_lm(["AB"] * 20 + ["AA"] * 2 + ["BA", "BB"], order=2, device=dev)
    assert est.mode == "char"
    # alpha * (log10 p(B | A) - log10 p(A | A)) outweighs the acoustic ln(0.55 / 0.43) = 0.25
    assert 2.0 * (fitted.lm.score(("A",), "B") - fitted.lm.score(("A",), "A")) > math.log(0.55 / 0.43) + 0.5
    assert fitted.decode(probs)[0][0][0] == "AB"
