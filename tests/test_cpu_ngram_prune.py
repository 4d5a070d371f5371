"""N-gram pruning and evaluation without a GPU: the library's host twins (ds2_ngram_eval_host, ds2_ngram_prune_*_host, through
NgramEstimate.prune / .perplexity with device="cpu") against the fp64 restatement (tests/ngram_prune_oracle.py), the invariants of a
pruned model, the written file read back through NgramLM, prune_arpa, and the refusals.  tests/test_gpu_ngram_prune.py holds the kernels
to the host twins with `same_model` below."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ngram_prune_oracle as P   # noqa: E402
import ngram_train_oracle as O   # noqa: E402
from test_cpu_ngram_train import LN10, REL, corpus, lm_of   # noqa: E402

THETAS = {"tiny": (5e-3,), "zipf": (1e-7, 1e-6, 1e-5, 1e-4), "char": (1e-7, 1e-6, 1e-5, 1e-4)}
GAP = 1e-6               # no restated value may lie this close (relatively) to a threshold: device, host and Python logarithms differ in
#                          their last bits and the bracket of dH cancels by about 1e3, so a decision is safe well beyond 1e-6
CASES = [(name, th) for name, ths in THETAS.items() for th in ths]
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def listed(name):
    """the restatement's listed model of a corpus and its entropy values"""
    return once(("listed", name), lambda: (lambda L: (L, P.values(L)[0]))(P.from_estimate(corpus(name)[2])))


def want(name, theta=None, min_count=None):
    return once(("want", name, theta, min_count), lambda: P.prune(listed(name)[0], theta, min_count, corpus(name)[2].c))


def full(name, device="cpu"):
    from asr_amd.decoders.lm_train import estimate_ngram
    sents, N, _ = corpus(name)
    return once(("full", name, str(device)), lambda: estimate_ngram([" ".join(s) for s in sents], order=N, mode="word", device=device))


def got(name, theta=None, min_count=None, device="cpu"):
    return once(("got", name, theta, min_count, str(device)), lambda: full(name, device).prune(theta, min_count, device=device))


def table(est):
    """an NgramEstimate as {n: {n-gram of token strings: (log10 p, log10 backoff)}}, <unk> included"""
    out = {}
    for n, (ids, _, _, lp, lb) in enumerate(est.ngrams, 1):
        out[n] = {tuple(est.vocab[i] for i in row): (p, b) for row, p, b in zip(ids.tolist(), lp.tolist(), lb.tolist())}
    if est.unk_log10 is not None:
        out[1][("<unk>",)] = (est.unk_log10, math.nan)
    return out


def as_listed(est):
    """an NgramEstimate as the restatement's Listed model, to run the restatement's sums on the library's numbers"""
    L, t = P.Listed(), table(est)
    L.N, L.vocab = est.order, list(est.vocab)
    L.p = [None] + [{g: 10.0 ** p for g, (p, _) in t[n].items()} for n in range(1, L.N + 1)]
    L.bow = [None] + [{g: 10.0 ** b for g, (_, b) in t[n].items() if b == b} for n in range(1, L.N + 1)]
    return L


def check_against_restatement(est, M, before):
    """a pruned NgramEstimate against the restatement's pruned model M: the kept sets exactly, kept log10 p bit for bit those of
    `before`, backoffs within relative 1e-12 (1 + 1/num + 1/den) of alpha: a sum of up to 1e3 terms carries about 1e-13 of absolute
    error, which the division by num and by den amplifies"""
    t, t0 = table(est), table(before)
    assert est.order == M.N
    for n in range(1, M.N + 1):
        assert set(t[n]) == set(M.p[n]), n
        for g, (p, b) in t[n].items():
            assert p == t0[n][g][0], g
            if g in M.bow[n]:
                num, den = M.nd[g]
                bound = math.inf if min(num, den) <= 0 else REL * (1.0 + 1.0 / num + 1.0 / den)
                assert abs(10.0 ** b / M.bow[n][g] - 1.0) <= bound, (g, b, M.bow[n][g], num, den)
            else:
                assert b != b, g


def same_model(a, b, bound_from):
    """two NgramEstimates (the kernels' and the twin's): keys, counts and log10 p equal, backoffs within the bound above"""
    assert (a.order, a.vocab, a.unk_log10) == (b.order, b.vocab, b.unk_log10)
    for n, (x, y) in enumerate(zip(a.ngrams, b.ngrams), 1):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), n
        assert x[3].tobytes() == y[3].tobytes(), n
        assert np.array_equal(np.isnan(x[4]), np.isnan(y[4])), n
        for row, p, q in zip(x[0].tolist(), x[4].tolist(), y[4].tolist()):
            if p == p:
                num, den = bound_from.nd[tuple(a.vocab[i] for i in row)]
                bound = math.inf if min(num, den) <= 0 else REL * (1.0 + 1.0 / num + 1.0 / den)
                assert abs(10.0 ** (p - q) - 1.0) <= bound, (row, p, q)


# ---- the restatement -------------------------------------------------------------------------------------------------

def test_restatement_keeps_what_the_prototype_kept():
    """the figures the rule was prototyped with: a changed rule shows here before it shows anywhere else"""
    assert [len(want("zipf", th).p[3]) for th in THETAS["zipf"]] == [13515, 4251, 370, 38]
    assert [len(want("char", th).p[5]) if want("char", th).N == 5 else 0 for th in THETAS["char"]] == [2629, 234, 36, 0]
    assert abs(min(listed("tiny")[1].values()) - 2.1e-3) < 1e-4
    M = want("zipf", None, (1, 1, 2))
    assert (len(M.p[2]), len(M.p[3])) == (12333, 616)


@pytest.mark.parametrize("name,theta", CASES)
def test_no_value_lies_at_a_threshold(name, theta):
    assert min(abs(v - theta) / theta for v in listed(name)[1].values()) >= GAP


def test_restatement_sums_to_one_for_any_removal_set():
    L = listed("tiny")[0]
    grams = [g for n in (2, 3) for g in L.p[n]]
    rng = np.random.default_rng(0)
    for _ in range(20):
        M = P.cut(L, {grams[i] for i in np.flatnonzero(rng.random(len(grams)) < 0.5)})
        for h in [()] + [g for n in range(1, M.N) for g in M.p[n] if g[-1] != "</s>" and g != ("<unk>",)]:
            assert abs(P.distribution_sum(M, h) - 1.0) <= 1e-12, h


# ---- the host twin ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,theta", CASES)
def test_twin_matches_restatement(name, theta):
    assert min(abs(v - theta) / theta for v in listed(name)[1].values()) >= GAP          # the condition of an exact comparison
    check_against_restatement(got(name, theta), want(name, theta), full(name))


def test_twin_values_match_restatement():
    from asr_amd import ops
    est = full("zipf")
    val, mark = ops.ngram_prune_values(est.model("cpu"), 1e-6)
    vals = listed("zipf")[1]
    assert val[0] is None and mark[0] is None
    for n in (2, 3):
        grams = [tuple(est.vocab[i] for i in row) for row in est.ngrams[n - 1][0].tolist()]
        v = val[n - 1].numpy()
        # the bracket of dH cancels by about 1e3 and the logarithms carry a few ulp: 1e-9 of the value is generous and far inside GAP
        assert all(abs(a - vals[g]) <= 1e-9 * abs(vals[g]) for a, g in zip(v.tolist(), grams)), n
        assert mark[n - 1].numpy().tolist() == [vals[g] < 1e-6 for g in grams]


def test_count_cut_and_both_modes():
    before = full("zipf")
    check_against_restatement(got("zipf", None, (1, 1, 2)), want("zipf", None, (1, 1, 2)), before)
    assert [len(s[0]) for s in got("zipf", None, (1, 1, 2)).ngrams] == [1757, 12333, 616]
    assert all((s[1] >= c).all() for s, c in zip(got("zipf", None, (1, 1, 2)).ngrams[1:], (1, 2)))       # the kept raw counts
    both = want("zipf", 1e-6, (1, 1, 2))
    vals = P.values(want("zipf", None, (1, 1, 2)))[0]                  # the entropy cut judges the model AFTER the count cut
    assert min(abs(v - 1e-6) / 1e-6 for v in vals.values()) >= GAP
    check_against_restatement(got("zipf", 1e-6, (1, 1, 2)), both, before)
    assert len(both.p[3]) < 616


@pytest.mark.parametrize("name", ["tiny", "zipf", "char"])
def test_invariants(name):
    rng = np.random.default_rng(2)
    kept = []
    for theta in THETAS[name]:
        est = got(name, theta)
        t = table(est)
        kept.append({g for n in t for g in t[n]})
        assert all(g[:-1] in t[n - 1] for n in range(2, est.order + 1) for g in t[n])       # every kept n-gram's prefix is kept
        L = as_listed(est)
        ctx = [g for n in range(1, est.order) for g, (_, b) in t[n].items() if b == b]
        pick = ctx if len(ctx) <= 30 else [ctx[int(i)] for i in rng.choice(len(ctx), size=12, replace=False)]
        for h in [()] + pick:
            assert abs(P.distribution_sum(L, h) - 1.0) <= 1e-12, (theta, h)
    assert all(b <= a for a, b in zip(kept, kept[1:]))                                       # nested in theta


def test_edges(tmp_path):
    from asr_amd.decoders.lm_train import estimate_ngram
    est = full("char")
    assert est.prune() is est and est.prune(None, None) is est
    assert est.prune(1e-12, device="cpu") is est                       # nothing is marked: the same arrays
    # theta = 1e-4 leaves no 5-gram: the order is dropped, from the model and from the file
    small = got("char", 1e-4)
    assert (small.order, len(small.ngrams)) == (4, 4) and all(len(s[0]) for s in small.ngrams)
    lm = lm_of(small.write_arpa(tmp_path / "c4.arpa"), "_ ")
    assert lm.order == 4 and lm.n_ngrams == sum(len(s[0]) for s in small.ngrams) + 1
    # a context that lost all its children lists no backoff; one that kept a child lists one
    t, t0 = table(small), table(est)
    lost = [g for n in (1, 2, 3) for g in t[n] if t0[n][g][1] == t0[n][g][1] and not any(k[:-1] == g for k in t[n + 1])]
    assert lost and all(t[len(g)][g][1] != t[len(g)][g][1] for g in lost)
    assert all((b == b) == any(k[:-1] == g for k in t[n + 1]) for n in (1, 2, 3) for g, (_, b) in t[n].items())
    # <s>-initial contexts are judged and kept like any other
    assert any(g[0] == "<s>" for g in t[3]) and any(g[0] == "<s>" for g in t0[5] if g[:4] not in t[4])
    # a corpus of one token
    one = estimate_ngram(["a"], order=3, device="cpu")
    L = P.from_estimate(O.estimate([["a"]], 3))
    vals = P.values(L)[0]
    theta = 2.0 * sorted(vals.values())[len(vals) // 2]
    assert min(abs(v - theta) / theta for v in vals.values()) >= GAP
    check_against_restatement(one.prune(theta, device="cpu"), P.prune(L, theta), one)


FULL_KEY_THETA = 1e-4


def full_key():
    """n_vocab = 65 536 at order 4: the key uses all 64 bits, its top bit included -> (the host estimate as an NgramEstimate whose
    vocabulary names all 65 536 ids, the restatement's listed model and its values, the sentences as token strings)"""
    def make():
        from asr_amd import ops
        from asr_amd.decoders.lm_train import NgramEstimate
        from test_gpu_ngram_train import shape
        flat, off, n_vocab, N = shape("full key")
        raw = ops.ngram_estimate_host(flat, off, n_vocab, N)
        assert raw["bits"] * N == 64 and int(raw["orders"][3][0].max()) >> 63 == 1
        vocab = ["<unk>", "<s>", "</s>"] + [f"t{i:05d}" for i in range(3, n_vocab)]
        sents = [[vocab[int(i)] for i in flat[a:b]] for a, b in zip(off[:-1], off[1:])]
        L = P.from_estimate(O.estimate(sents, N))
        return NgramEstimate(raw, "word", vocab, int(flat.size), len(off) - 1, 0), L, P.values(L)[0], sents
    return once("full key", make)


def test_full_key():
    """the shifts of pr_low and pr_log_history where the key is full: kept sets, kept log10 p, new backoffs and the evaluation"""
    import torch
    from asr_amd import ops
    est, L, vals, sents = full_key()
    assert min(abs(v - FULL_KEY_THETA) / FULL_KEY_THETA for v in vals.values()) >= GAP
    M = once("full key want", lambda: P.prune(L, FULL_KEY_THETA))
    assert 0 < len(M.p[4]) < len(L.p[4])
    pruned = once("full key got", lambda: est.prune(FULL_KEY_THETA, device="cpu"))
    check_against_restatement(pruned, M, est)
    for one, ref in ((est, L), (pruned, M)):
        flat, off = one.tokens(sents[:200] + [[], ["never-seen"]])
        lp, order = ops.ngram_eval(one.model("cpu"), torch.from_numpy(flat), torch.from_numpy(off))
        want_scores = P.score(ref, sents[:200] + [[], ["never-seen"]])
        assert order.tolist() == [n for _, n in want_scores]
        assert all(abs(a - math.log10(p)) * LN10 <= REL for a, (p, _) in zip(lp.tolist(), want_scores))


# ---- evaluation ------------------------------------------------------------------------------------------------------

def held_out(name):
    sents = corpus(name)[0]
    rng = np.random.default_rng(3)
    out = [list(sents[int(i)]) for i in rng.choice(len(sents), size=min(40, len(sents)), replace=False)]
    out[3] = out[3] + ["never-seen"] + out[4]                            # OOV in the middle, at the start and alone
    out[5] = ["never-seen", "nor-this"] + out[5]
    return out + [[], ["never-seen"], list(reversed(sents[0]))]


@pytest.mark.parametrize("name,theta", [("tiny", None), ("zipf", None), ("char", None), ("zipf", 1e-6), ("char", 1e-4)])
def test_evaluation_matches_restatement(name, theta):
    import torch
    from asr_amd import ops
    est = got(name, theta)
    m = corpus(name)[2]
    L = listed(name)[0] if theta is None else want(name, theta)
    sents = held_out(name)
    flat, off = est.tokens(sents)
    assert (flat == 0).sum() == 4 and len(off) == len(sents) + 1
    lp, order = ops.ngram_eval(est.model("cpu"), torch.from_numpy(flat), torch.from_numpy(off))
    ref = P.score(L, sents)
    assert len(ref) == len(lp) == sum(len(s) + 1 for s in sents)
    assert order.tolist() == [n for _, n in ref]
    assert all(abs(a - math.log10(p)) * LN10 <= REL for a, (p, _) in zip(lp.tolist(), ref))
    if theta is None:                                                    # and the estimator's own reader of the file
        framed = [["<s>"] + [w if w in m.vocab else "<unk>" for w in s] + ["</s>"] for s in sents]
        flat_ref = [O.arpa_prob(m, f[:i], f[i]) for f in framed for i in range(1, len(f))]
        assert all(abs(a - math.log10(p)) * LN10 <= REL for a, p in zip(lp.tolist(), flat_ref))
    r = est.perplexity(sents, device="cpu")
    total = math.fsum(math.log10(p) for p, _ in ref)
    assert abs(r["log10_prob"] - total) <= 1e-12 * abs(total)
    assert (r["n_tokens"], r["n_sentences"], r["n_oov"]) == (sum(len(s) for s in sents), len(sents), 4)
    assert r["hits"] == [sum(1 for _, n in ref if n == k) for k in range(1, est.order + 1)] and sum(r["hits"]) == len(ref)
    assert abs(r["perplexity"] / 10.0 ** (-total / len(ref)) - 1.0) <= 1e-12


@pytest.mark.parametrize("name", ["tiny", "zipf", "char"])
def test_pruning_does_not_lower_training_perplexity(name):
    sents = corpus(name)[0]
    ppl = [full(name).perplexity(sents, device="cpu")["perplexity"]] + [got(name, th).perplexity(sents, device="cpu")["perplexity"]
                                                                         for th in THETAS[name]]
    assert all(p >= ppl[0] for p in ppl[1:]) and ppl[-1] > ppl[0]


def test_model_without_unk_leaves_oov_out(tmp_path):
    from asr_amd.decoders.lm_train import prune_arpa
    src = tmp_path / "nounk.arpa"
    src.write_text("\n\\data\\\nngram 1=4\nngram 2=3\n\n\\1-grams:\n-99\t<s>\t-0.2\n-0.5\t</s>\n-0.4\ta\t-0.3\n-0.6\tb\n\n"
                   "\\2-grams:\n-0.2\t<s> a\n-0.3\ta b\n-0.25\ta </s>\n\n\\end\\\n")
    est = prune_arpa(str(src), str(tmp_path / "out.arpa"), 1e-9)
    assert est.unk_log10 is None and est.order == 2 and "<unk>" not in open(tmp_path / "out.arpa").read()
    r = est.perplexity([["a", "zzz", "b"]], device="cpu")
    assert (r["n_oov"], r["hits"], r["n_tokens"]) == (1, [2, 1], 3)
    # a (after <s>), b after the OOV (the context ends there: the 1-gram) and </s> after b
    assert abs(r["log10_prob"] - (-0.2 - 0.6 - 0.5)) <= 1e-12 and abs(r["perplexity"] - 10.0 ** (1.3 / 3)) <= 1e-12


# ---- the file and the public layer -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,theta", [("zipf", 1e-6), ("char", 1e-5)])
def test_written_file_scores_as_the_restatement(tmp_path, name, theta):
    est, M = got(name, theta), want(name, theta)
    N = M.N
    lm = lm_of(est.write_arpa(tmp_path / "p.arpa"), "_ ")
    assert lm.order == N and list(lm.vocab) == est.vocab
    rng = np.random.default_rng(4)
    text = [["<s>"] * (N - 1) + list(s) + ["</s>"] for s in corpus(name)[0] if s]          # (score() pads a short context with <s>)
    n_backed = 0
    for i in rng.choice(len(text), size=60, replace=False):
        f = text[int(i)]
        j = int(rng.integers(N - 1, len(f)))
        h, w = tuple(f[j - (N - 1):j]), f[j]
        while len(h) > 1 and h[0] == "<s>" and h[1] == "<s>":          # the restatement knows one <s>
            h = h[1:]
        p, n = P.prob(M, h, w)
        n_backed += n < N
        # at most N backoffs and one probability, each below 8 in magnitude and read as fp32, added in fp32
        assert abs(lm.score(f[j - (N - 1):j], w) - math.log10(p)) <= 2 * (N + 1) * 2.0 ** -21, (h, w)
    assert n_backed > 10


def test_prune_arpa_matches_prune(tmp_path):
    """the file holds 8 decimals: each p and q moves by up to 1.2e-8 relatively, which the bracket of dH amplifies to about 1e-5 of a
    value, so the decisions are the same where no value lies within 1e-4 of the threshold"""
    from asr_amd.decoders.lm_train import prune_arpa
    for name, theta in (("tiny", 5e-3), ("char", 5e-6)):
        assert min(abs(v - theta) / theta for v in listed(name)[1].values()) >= 1e-4
        src = full(name).write_arpa(tmp_path / f"{name}.arpa")
        est = prune_arpa(str(src), str(tmp_path / f"{name}.pruned.arpa"), theta, device="cpu")
        ref, M = got(name, theta), want(name, theta)
        assert (est.order, est.vocab, est.mode) == (ref.order, ref.vocab, "char")          # (every token is one character)
        assert est.ngrams[0][1] is None and est.discounts is None
        a, b = table(est), table(ref)
        for n in range(1, ref.order + 1):
            assert set(a[n]) == set(b[n]), n
            for g, (p, bo) in a[n].items():
                assert abs(p - b[n][g][0]) <= 5.1e-9 and (bo == bo) == (b[n][g][1] == b[n][g][1]), g
                if bo == bo:
                    num, den = M.nd[g]
                    assert min(num, den) <= 0 or abs(bo - b[n][g][1]) * LN10 <= 1.2e-8 * (1.0 + 1.0 / num + 1.0 / den), g
        assert lm_of(tmp_path / f"{name}.pruned.arpa", "_ ").n_ngrams == sum(len(s[0]) for s in ref.ngrams) + 1


def test_public_layer(tmp_path):
    from asr_amd.decoders import BeamCTCDecoder
    from asr_amd.decoders.lm_train import estimate_ngram
    text = [" ".join(s) for s in corpus("zipf")[0]]
    ref = got("zipf", 1e-6, (1, 1, 2))
    est = estimate_ngram(text, order=3, device="cpu", prune=1e-6, min_count=(1, 1, 2))
    a, b = est.write_arpa(tmp_path / "a.arpa"), ref.write_arpa(tmp_path / "b.arpa")
    assert open(a, "rb").read() == open(b, "rb").read() and est.n_tokens == ref.n_tokens
    # without the new arguments: the bytes of the plain estimate, through every layer
    sentences = ["AB CA", "CA AB B", "B AB", "CAB AB", "AB", "AB CA B"]
    d = BeamCTCDecoder("_ABC ")
    d.fit_lm(sentences, order=3, path=str(tmp_path / "plain.arpa"), device="cpu")
    plain = estimate_ngram(sentences, order=3, device="cpu")
    assert open(tmp_path / "plain.arpa", "rb").read() == open(plain.write_arpa(tmp_path / "plain2.arpa"), "rb").read()
    vals = P.values(P.from_estimate(O.estimate([s.split() for s in sentences], 3)))[0]
    theta = 2.0 * sorted(vals.values())[len(vals) // 2]
    assert min(abs(v - theta) / theta for v in vals.values()) >= GAP
    est = d.fit_lm(sentences, order=3, path=str(tmp_path / "pruned.arpa"), device="cpu", prune=theta)
    assert sum(len(s[0]) for s in est.ngrams) < sum(len(s[0]) for s in plain.ngrams) and d.lm.n_ngrams == sum(len(s[0]) for s in est.ngrams) + 1
    assert open(tmp_path / "pruned.arpa", "rb").read() == open(plain.prune(theta, device="cpu").write_arpa(tmp_path / "p2.arpa"), "rb").read()


def test_model_fit_lm_passes_pruning_through(tmp_path):
    import pandas as pd
    from asr_amd.decoders import BeamCTCDecoder
    from asr_amd.modules.deepspeech import DeepSpeech
    rows = ["AB A", "B A", "AB A", "A B AB", "B AB A"]
    pd.DataFrame({"audio_filepath": [f"{i}.wav" for i in range(len(rows))], "text": rows}).to_csv(tmp_path / "m.csv", index=False)
    model = DeepSpeech.__new__(DeepSpeech)                               # fit_lm touches the decoder only
    object.__setattr__(model, "decoder", BeamCTCDecoder("_AB "))
    whole = DeepSpeech.fit_lm(model, str(tmp_path / "m.csv"), order=2, device="cpu")
    cut = DeepSpeech.fit_lm(model, str(tmp_path / "m.csv"), order=2, device="cpu", min_count=(1, 2))
    assert len(cut.ngrams[1][0]) < len(whole.ngrams[1][0]) and (cut.ngrams[1][1] >= 2).all()


def test_refusals(tmp_path):
    from asr_amd.decoders.lm_train import prune_arpa
    est = full("tiny")
    for bad in (0, 0.0, -1e-6, math.inf, math.nan, "1e-6", True, np.float32(0.0), [1e-3]):
        with pytest.raises(ValueError, match="threshold"):
            est.prune(bad, device="cpu")
    import torch
    for good in (np.float32(5e-3), np.float64(5e-3), torch.tensor(5e-3)):          # any real number is taken
        assert [len(s[0]) for s in est.prune(good, device="cpu").ngrams] == [len(s[0]) for s in got("tiny", 5e-3).ngrams]
    for bad in ((1, 2, 1), (1, 1), (1, 1, 1, 1), (1, 0, 1), (1, 1.5, 2), 2, "112"):
        with pytest.raises(ValueError, match="min_count"):
            est.prune(min_count=bad, device="cpu")
    assert est.prune(min_count=(7, 1, 1), device="cpu") is est         # the first entry is ignored; nothing is below 1
    src = est.write_arpa(tmp_path / "t.arpa")
    from_file = prune_arpa(str(src), str(tmp_path / "t2.arpa"), 5e-3, device="cpu")
    with pytest.raises(ValueError, match="counts"):
        from_file.prune(min_count=(1, 2, 2), device="cpu")
    with pytest.raises(ValueError, match="threshold"):
        prune_arpa(str(src), str(tmp_path / "t3.arpa"), None)
    # 70 000 words need 17 bits a token: order 4 does not fit the key
    big = tmp_path / "big.arpa"
    words = [f"w{i}" for i in range(70000)]
    big.write_text("\n\\data\\\nngram 1=70000\nngram 2=0\nngram 3=0\nngram 4=1\n\n\\1-grams:\n" + "".join(f"-5\t{w}\n" for w in words) +
                   "\n\\2-grams:\n\n\\3-grams:\n\n\\4-grams:\n-1\tw0 w1 w2 w3\n\n\\end\\\n")
    with pytest.raises(ValueError, match="64-bit"):
        prune_arpa(str(big), str(tmp_path / "big2.arpa"), 1e-6)
    bad = tmp_path / "ctx.arpa"
    bad.write_text("\n\\data\\\nngram 1=2\nngram 2=1\nngram 3=1\n\n\\1-grams:\n-1\ta\n-1\tb\n\n\\2-grams:\n-0.5\ta b\n\n"
                   "\\3-grams:\n-0.2\tb a b\n\n\\end\\\n")
    with pytest.raises(ValueError, match="context"):
        prune_arpa(str(bad), str(tmp_path / "ctx2.arpa"), 1e-6)
