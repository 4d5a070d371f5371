"""-m gpu: the evaluation and pruning kernels (ds2_ngram_eval, ds2_ngram_prune_*; ops.ngram_eval, ops.ngram_prune) against their host
twins, which tests/test_cpu_ngram_prune.py holds to the fp64 restatement: marks and kept sets exactly, kept log10 p bit for bit,
backoffs within the bound derived there; and BeamCTCDecoder.fit_lm(prune=) through the search.  Both sides start from the SAME arrays
(the host estimate), so that only the pruning is compared.  MI355X figures are in profiles/ngram_prune_timing.txt."""
import numpy as np
import pytest
import torch

import ngram_prune_oracle as P
import ngram_train_oracle as O
from test_cpu_ngram_prune import (CASES, FULL_KEY_THETA, GAP, check_against_restatement, full, full_key, got, held_out, listed, once,
                                  same_model, want)
from test_cpu_ngram_train import LN10, REL, corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def on_device(dev, name, theta=None, min_count=None):
    """the host estimate of a corpus, pruned by the kernels"""
    return once(("kernels", name, theta, min_count), lambda: full(name).prune(theta, min_count, device=dev))


@pytest.mark.parametrize("name,theta", CASES)
def test_kernels_match_twin(dev, name, theta):
    assert min(abs(v - theta) / theta for v in listed(name)[1].values()) >= GAP          # the condition of an exact comparison
    if name == "zipf":                                                   # <s> and w0: their children span waves and blocks
        ids = full("zipf").ngrams[1][0]
        kids = np.bincount(ids[:, 0])
        assert kids[1] > 256 and kids[3] > 64 and np.flatnonzero(ids[:, 0] == 1)[0] % 64 + kids[1] > 256
    same_model(on_device(dev, name, theta), got(name, theta), want(name, theta))
    check_against_restatement(on_device(dev, name, theta), want(name, theta), full(name))


def test_count_cut_and_both_modes(dev):
    for theta in (None, 1e-6):
        same_model(on_device(dev, "zipf", theta, (1, 1, 2)), got("zipf", theta, (1, 1, 2)), want("zipf", theta, (1, 1, 2)))
        check_against_restatement(on_device(dev, "zipf", theta, (1, 1, 2)), want("zipf", theta, (1, 1, 2)), full("zipf"))
    assert full("zipf").prune(1e-12, device=dev) is full("zipf")         # nothing is marked: the same arrays


@pytest.mark.parametrize("name", ["zipf", "char"])
def test_values_and_marks_match_twin(dev, name):
    from asr_amd import ops
    est = full(name)
    val, mark = ops.ngram_prune_values(est.model(dev), 1e-6)
    val_h, mark_h = ops.ngram_prune_values(est.model("cpu"), 1e-6)
    for n in range(2, est.order + 1):
        a, b = val[n - 1].cpu().numpy(), val_h[n - 1].numpy()
        # the bracket of dH cancels by about 1e3 and the two sides' logarithms and sums differ by a few ulp: 1e-9 of the value, far inside GAP
        assert np.all(np.abs(a - b) <= 1e-9 * np.abs(b)), n
        assert torch.equal(mark[n - 1].cpu(), mark_h[n - 1]), n


def test_full_key(dev):
    """n_vocab = 65 536 at order 4, the key's 64 bits all in use: the kernels on the arrays the twin was held to the restatement with"""
    from asr_amd import ops
    est, L, vals, sents = full_key()
    assert min(abs(v - FULL_KEY_THETA) / FULL_KEY_THETA for v in vals.values()) >= GAP
    M = once("full key want", lambda: P.prune(L, FULL_KEY_THETA))
    pruned = est.prune(FULL_KEY_THETA, device=dev)
    same_model(pruned, once("full key got", lambda: est.prune(FULL_KEY_THETA, device="cpu")), M)
    check_against_restatement(pruned, M, est)
    for one in (est, pruned):
        flat, off = one.tokens(sents[:200] + [[], ["never-seen"]])
        lp, order = ops.ngram_eval(one.model(dev), torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev))
        lp_h, order_h = ops.ngram_eval(one.model("cpu"), torch.from_numpy(flat), torch.from_numpy(off))
        assert torch.equal(order.cpu(), order_h) and bool((torch.abs(lp.cpu() - lp_h) * LN10 <= REL).all())


def wide(n_children=5000):
    """one context with 5 000 children, in three count classes: its rows fill 79 waves, so the second launch strides over the partials"""
    return [["x", f"w{i:04d}"] for i in range(n_children) for _ in range(1 + i % 3)]


def test_one_context_across_79_waves(dev):
    from asr_amd import ops
    sents = wide()
    vocab, flat, off = O.to_ids(sents)
    raw = ops.ngram_estimate_host(flat, off, len(vocab), 2)
    L = P.from_estimate(O.estimate(sents, 2))
    vals = sorted(set(P.values(L)[0].values()))
    theta = next((a * b) ** 0.5 for a, b in zip(vals, vals[1:]) if b / a > 1.5)      # between two count classes
    assert min(abs(v - theta) / theta for v in vals) >= GAP
    M = P.prune(L, theta)
    assert 0 < sum(1 for g in M.p[2] if g[0] == "x") < 5000 and (len(M.p[2]) + 63) // 64 > 64
    out = [ops.ngram_model_download(ops.ngram_prune(ops.ngram_model(raw, d), theta)) for d in (dev, "cpu")]
    for (k, c, _, lp, lb), (k2, c2, _, lp2, lb2) in zip(out[0]["orders"], out[1]["orders"]):
        assert np.array_equal(k, k2) and np.array_equal(c, c2) and lp.tobytes() == lp2.tobytes()
        assert np.array_equal(np.isnan(lb), np.isnan(lb2))
    keys, _, _, _, lb = out[0]["orders"][0]
    lb2 = out[1]["orders"][0][4]
    for tok in ("x", "<s>"):
        r = int(np.flatnonzero(keys == np.uint64(vocab.index(tok)))[0])
        num, den = M.nd[(tok,)]
        bound = REL * (1.0 + 1.0 / num + 1.0 / den)
        assert abs(10.0 ** lb[r] / M.bow[1][(tok,)] - 1.0) <= bound and abs(10.0 ** (lb[r] - lb2[r]) - 1.0) <= bound, tok


@pytest.mark.parametrize("name,theta", [("tiny", None), ("zipf", None), ("zipf", 1e-6), ("char", 1e-4)])
def test_evaluation_matches_twin(dev, name, theta):
    from asr_amd import ops
    est = got(name, theta)
    sents = held_out(name) + corpus(name)[0][:300]
    flat, off = est.tokens(sents)
    lp, order = ops.ngram_eval(est.model(dev), torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev))
    lp_h, order_h = ops.ngram_eval(est.model("cpu"), torch.from_numpy(flat), torch.from_numpy(off))
    assert lp.numel() == flat.size + len(sents) and torch.equal(order.cpu(), order_h)
    assert bool((torch.abs(lp.cpu() - lp_h) * LN10 <= REL).all())
    a, b = est.perplexity(sents, device=dev), est.perplexity(sents, device="cpu")
    assert {k: a[k] for k in ("n_tokens", "n_sentences", "n_oov", "hits")} == {k: b[k] for k in ("n_tokens", "n_sentences", "n_oov", "hits")}
    assert abs(a["log10_prob"] - b["log10_prob"]) <= 1e-12 * abs(b["log10_prob"])


def test_two_runs_write_the_same_bytes(dev, tmp_path):
    from asr_amd.decoders.lm_train import estimate_ngram
    text = [" ".join(s) for s in corpus("zipf")[0]]
    files = []
    for i in range(2):
        est = estimate_ngram(text, order=3, device=dev, prune=1e-6)
        files.append(open(est.write_arpa(tmp_path / f"run{i}.arpa"), "rb").read())
    assert files[0] == files[1]
    assert est.model() is est.model("cuda") is est.model(dev) and len(est._models) == 1      # the pruned arrays, kept where they were made
    assert [len(s[0]) for s in est.ngrams] == [len(s[0]) for s in got("zipf", 1e-6).ngrams]


def test_fit_lm_pruned_decodes_as_the_written_file(dev, tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    labels = "_w0123456789 "
    sentences = [" ".join(s) for s in corpus("zipf")[0]]
    fitted = BeamCTCDecoder(labels, beam_width=20)
    est = fitted.fit_lm(sentences, order=3, path=str(tmp_path / "w.arpa"), alpha=1.5, beta=0.5, device=dev, prune=1e-6)
    assert est.mode == "word" and len(est.ngrams[2][0]) == len(got("zipf", 1e-6).ngrams[2][0]) < len(full("zipf").ngrams[2][0])
    assert fitted.lm.n_ngrams == sum(len(s[0]) for s in est.ngrams) + 1
    loaded = BeamCTCDecoder(labels, lm_path=str(tmp_path / "w.arpa"), alpha=1.5, beta=0.5, beam_width=20)
    probs = torch.softmax(2.0 * torch.randn(3, 14, len(labels), generator=torch.Generator().manual_seed(4)), dim=-1).to(dev)
    a, _ = fitted.decode(probs)
    b, _ = loaded.decode(probs)
    assert a == b and fitted.last_scores.numpy().tobytes() == loaded.last_scores.numpy().tobytes()
    assert any(s for s in a[0])
