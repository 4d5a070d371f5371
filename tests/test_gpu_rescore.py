"""-m gpu: NBestRescorer and tune_lm_weights (asr_amd/decoders) end to end on tiny problems: the exact acoustic term against brute-force
enumeration (the suite's nll bar: atol 1e-4, rtol 1e-5), the rescored order and totals against the plain-Python restatement
tests/lm_score_oracle.py, chunked against unchunked likelihoods to the bit, and the grid of a planted dev set against NumPy."""
import math
import pathlib
import tempfile

import numpy as np
import pytest
import torch

import ctc_beam_lm_oracle as LO
import lm_score_oracle as SO
from ctc_beam_oracle import brute_force_label_logprobs
from lm_fixtures import random_arpa, write_arpa
from test_gpu_lm_score import sweep_reference

pytestmark = pytest.mark.gpu
CHARS = "_AB "                # blank 0, space 3
LABELS = {c: i for i, c in enumerate(CHARS)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lm_dir():
    with tempfile.TemporaryDirectory() as d:
        yield pathlib.Path(d)


def random_lm(lm_dir):
    return random_arpa(str(lm_dir / "random.arpa"), ["A", "AB", "BA", "B", "ABB"], 3, 30, seed=5)


def planted_lm(lm_dir):
    """two words, AB and BA; every other spelling is out of the vocabulary"""
    uni = [(("<s>",), -99.0, -0.3), (("</s>",), -1.0, None), (("AB",), -1.0, -0.3), (("BA",), -1.0, -0.3)]
    bi = [(("<s>", "AB"), -0.4, None), (("AB", "BA"), -0.5, None), (("BA", "AB"), -0.6, None)]
    return write_arpa(str(lm_dir / "planted.arpa"), [uni, bi])


def decoder(K, lm_path=None, alpha=0.0, beta=0.0):
    from asr_amd.decoders import BeamCTCDecoder
    return BeamCTCDecoder(LABELS, lm_path=lm_path, alpha=alpha, beta=beta, beam_width=K)


def dirichlet(B, T, seed):
    return np.random.default_rng(seed).dirichlet(np.ones(len(CHARS)) * 0.6, size=(B, T)).astype(np.float32)


def slots(f):
    """features -> per utterance [(labels tuple, valid)] from the device tensors"""
    lab, lens, ac = f["labels"].cpu().numpy(), f["lens"].cpu().numpy(), f["ac"].cpu().numpy()
    sc = f["scores"].cpu().numpy()
    return [[(tuple(int(x) for x in lab[b, k, :lens[b, k]]), sc[b, k] > -math.inf, float(ac[b, k])) for k in range(lab.shape[1])]
            for b in range(lab.shape[0])]


@pytest.mark.parametrize("fused", [False, True])
def test_exact_acoustic_term_is_the_ctc_likelihood(dev, lm_dir, fused):
    """with or without an LM in the first pass, ac is log p_ctc(labeling | x): none of the terms that chose the list"""
    from asr_amd.decoders import NBestRescorer
    probs, sizes = dirichlet(3, 6, seed=1), [6, 2, 5]            # (2 frames: 10 labelings, so slots stay empty)
    dec = decoder(40, random_lm(lm_dir), 0.8, 0.3) if fused else decoder(40)
    f = NBestRescorer(dec, lm=None if fused else random_lm(lm_dir)).features(torch.from_numpy(probs), torch.tensor(sizes))
    seen = empty = 0
    for b, row in enumerate(slots(f)):
        truth = brute_force_label_logprobs(probs[b, :sizes[b]].astype(np.float64), 0)
        for lab, valid, ac in row:
            if not valid:
                assert ac == -math.inf and lab == ()
                empty += 1
                continue
            err = abs(ac - truth[lab])
            print(f"utterance {b} {lab}: ac {ac:.6f} brute force {truth[lab]:.6f} err {err:.2e}")
            assert err <= 1e-4 + 1e-5 * abs(truth[lab]), (b, lab, ac, truth[lab])
            seen += 1
    assert seen > 20 and (fused or empty > 0)


def oracle_totals(ref, probs, size, row, alpha, beta, oov_score=LO.OOV):
    """per valid slot of one utterance: (fp64 total, tolerance of an fp32 restatement of it)"""
    truth = brute_force_label_logprobs(probs[:size].astype(np.float64), 0)
    out = {}
    for lab, valid, _ in row:
        if valid:
            r = SO.score_sequence(ref, CHARS, 0, 3, lab)
            lm = r["lm_sum"] + oov_score * r["n_oov"]
            total = truth[lab] + alpha * lm + beta * r["n_tok"]
            # the likelihood's bar, the LM sum's derived bound, and five fp32 roundings of the terms
            tol = 1e-4 + 1e-5 * abs(truth[lab]) + abs(alpha) * SO.bound(ref, r) \
                + 5 * 2.0 ** -24 * (abs(truth[lab]) + (1 + abs(alpha)) * abs(lm) + abs(beta) * r["n_tok"])
            out[lab] = (total, tol)
    return out


def test_rescoring_swaps_the_planted_pair_and_follows_the_oracle(dev, lm_dir):
    from asr_amd.decoders import NBestRescorer
    sharp = lambda c: [0.985 if i == c else 0.005 for i in range(4)]   # noqa: E731
    amb = lambda hi, lo: [0.55 if i == hi else 0.43 if i == lo else 0.01 for i in range(4)]   # noqa: E731
    probs = np.array([[sharp(1), amb(1, 2), sharp(0), sharp(0)],           # "A" (no word) ahead of "AB"
                      [sharp(2), amb(2, 1), sharp(3), sharp(1)]], np.float32)   # "B A" ahead of "BA A": both out of the vocabulary
    probs[1, 3] = amb(1, 0)
    sizes = [2, 4]
    dec, path = decoder(24), planted_lm(lm_dir)
    ref = LO.NaiveLM(path)
    first, _ = dec.decode(torch.from_numpy(probs), torch.tensor(sizes))
    assert first[0][:2] == ["A", "AB"]
    resc = NBestRescorer(dec, lm=path)
    f = resc.features(torch.from_numpy(probs), torch.tensor(sizes))
    for alpha, beta in ((0.5, 0.2), (2.0, -0.5), (0.0, 0.0)):
        strings, offsets = resc.rescore(torch.from_numpy(probs), torch.tensor(sizes), alpha, beta)
        assert (strings[0][0] == "AB") == (alpha > 0)
        got = resc.last_scores.numpy()
        for b, row in enumerate(slots(f)):
            want = oracle_totals(ref, probs[b], sizes[b], row, alpha, beta)
            live = [lab for lab, valid, _ in row if valid]
            assert sorted(strings[b][:len(live)]) == sorted("".join(CHARS[x] for x in lab) for lab in live)
            assert all(s == "" for s in strings[b][len(live):]) and (got[b, len(live):] == -math.inf).all()
            assert all(len(o) == len(s) for o, s in zip(offsets[b], strings[b]))
            prev = math.inf
            for k in range(len(live)):
                total, tol = want[tuple(CHARS.index(ch) for ch in strings[b][k])]
                print(f"alpha {alpha} beta {beta} utterance {b} rank {k} {strings[b][k]!r}: {got[b, k]:.6f} oracle {total:.6f} tol {tol:.1e}")
                assert abs(got[b, k] - total) <= tol, (b, k, strings[b][k], got[b, k], total)
                assert total <= prev + 1e-3, (b, k)              # the oracle's order wherever its gaps exceed 1e-3
                prev = total


def test_chunked_likelihoods_are_the_unchunked_bits(dev, lm_dir):
    from asr_amd.decoders import NBestRescorer
    B, T, K = 5, 6, 16
    probs, sizes = torch.from_numpy(dirichlet(B, T, seed=3)), torch.tensor([6, 5, 6, 3, 4])
    dec, path = decoder(K), random_lm(lm_dir)
    whole = NBestRescorer(dec, lm=path)
    small = NBestRescorer(dec, lm=whole.lm, workspace_bytes=1)       # below any utterance's need: one utterance per chunk
    fw, fs = whole.features(probs, sizes), small.features(probs, sizes)
    assert len(whole._chunks(fw["lens_host"], T, K)) == 1 and len(small._chunks(fs["lens_host"], T, K)) == B
    for key in ("labels", "lens", "ac", "lm_sum", "n_tok", "n_oov"):
        assert torch.equal(fw[key], fs[key]), key
    assert torch.isfinite(fw["ac"]).any()


def test_beam_scores_as_the_acoustic_term(dev, lm_dir):
    from asr_amd.decoders import NBestRescorer
    path = random_lm(lm_dir)
    with pytest.raises(ValueError, match="acoustic='beam'"):
        NBestRescorer(decoder(8, path, 0.5, 0.1), acoustic="beam")
    probs = torch.from_numpy(dirichlet(2, 3, seed=4))                # T = 3: at most 40 prefixes, so a beam of 64 prunes nothing
    f = NBestRescorer(decoder(64), lm=path, acoustic="beam").features(probs)
    assert torch.equal(f["ac"], f["scores"])
    exact = NBestRescorer(decoder(64), lm=path).features(probs)["ac"]
    # an unpruned search without an LM sums every alignment: its totals ARE the likelihoods (the beam suite's bar: 1e-4 relative)
    assert torch.allclose(f["ac"], exact, rtol=1e-4, atol=1e-4) and torch.isfinite(exact).sum() > 20


def test_tune_decoder_is_tune_lm_weights_on_the_eval_forward(dev, lm_dir):
    """DeepSpeech.tune_decoder: the grid of tune_lm_weights on evaluate()'s own output_data; confirm=True reports the evaluate() of the
    chosen weights and leaves the decoder's weights as they were"""
    import os

    from asr_amd.decoders import BeamCTCDecoder, NBestRescorer, tune_lm_weights
    from helpers import model_inputs
    from test_gpu_model import make_model
    cfg = dict(rnn="gru", hidden=40, layers=2, classes=29, t_ins=[140, 120, 90, 33])
    sd, x, targets, pct, tsz = model_inputs(cfg)
    model = make_model(cfg, sd)
    chars = "".join(model.decoder.int_to_char[i] for i in range(29))
    lm_path = random_arpa(str(lm_dir / "eval_char.arpa"), sorted({c for c in chars if c not in "_ "}), 3, 200, 5)
    dec = model.decoder = BeamCTCDecoder(model.labels, lm_path=lm_path, alpha=0.5, beta=0.5, beam_width=16)
    alphas, betas = [0.0, 0.4, 1.2], [-0.5, 0.5]
    loader = lambda: [(x, targets, pct.clone(), tsz), (x[:2], targets[:int(tsz[:2].sum())], pct[:2].clone(), tsz[:2])]   # noqa: E731
    got = model.tune_decoder(loader=loader(), alphas=alphas, betas=betas, confirm=True, device="cuda")
    assert (dec.alpha, dec.beta) == (0.5, 0.5) and model.decoder is dec
    _, _, output_data = model.evaluate(loader=loader(), device="cuda", output_file=os.path.join(str(lm_dir), "eval.txt"))
    want = tune_lm_weights(NBestRescorer(dec), output_data, alphas, betas)
    for key in ("alpha", "beta", "wer", "cer", "first_pass", "oracle"):
        assert got[key] == want[key], key
    assert np.array_equal(got["grid_wer"], want["grid_wer"]) and np.array_equal(got["grid_cer"], want["grid_cer"])
    assert got["oracle"][0] <= min(got["first_pass"][0], got["grid_wer"].min())
    dec.alpha, dec.beta = got["alpha"], got["beta"]
    wer, cer, _ = model.evaluate(loader=loader(), device="cuda")
    assert got["confirmed"] == (wer, cer)


def planted_dev_set():
    """8 utterances over the words AB and BA whose posteriors spell the reference sharply, except that the second letter of one word
    is a little less likely (0.43) than a repeat of the first (0.55): the first pass drops that letter, which leaves no word"""
    sharp = lambda c: [0.985 if i == c else 0.005 for i in range(4)]   # noqa: E731
    amb = lambda hi, lo: [0.55 if i == hi else 0.43 if i == lo else 0.01 for i in range(4)]   # noqa: E731
    refs = ["AB", "BA", "AB BA", "BA AB", "AB AB", "BA BA", "AB BA AB", "BA AB BA"]
    rows = []
    for i, r in enumerate(refs):
        words, fr = r.split(), []
        for wi, w in enumerate(words):
            if wi:
                fr.append(sharp(3))
            a, b = LABELS[w[0]], LABELS[w[1]]
            fr += [sharp(a), amb(a, b) if wi == i % len(words) else sharp(b)]
        rows.append(fr)
    T = max(len(fr) for fr in rows)
    probs = np.full((len(rows), T, 4), 0.25, np.float32)
    for i, fr in enumerate(rows):
        probs[i, :len(fr)] = fr
    return probs, np.array([len(fr) for fr in rows], np.int32), refs


def test_tune_lm_weights_on_a_planted_dev_set(dev, lm_dir):
    from asr_amd.decoders import NBestRescorer, tune_lm_weights
    probs, sizes, refs = planted_dev_set()
    resc = NBestRescorer(decoder(30), lm=planted_lm(lm_dir))
    # two batches, in the form of evaluate()'s output_data
    batches = [(probs[:4], sizes[:4], [[r] for r in refs[:4]]), (probs[4:], sizes[4:], [[r] for r in refs[4:]])]
    alphas, betas = [0.0, 0.5, 1.0, 2.0], [-0.5, 0.0, 0.5]
    out = tune_lm_weights(resc, batches, alphas, betas)
    feats, errs = [], []
    for p, s, r in batches:
        f = resc.features(p, s)
        errs.append(resc.errors(f, r).cpu().numpy())
        feats.append([f[k].cpu().numpy() for k in ("ac", "lm_sum", "n_tok", "n_oov")])
    ac, lm_sum, n_tok, n_oov = (np.concatenate([x[i] for x in feats]) for i in range(4))
    err = np.concatenate(errs)
    n_words, n_chars = sum(len(r.split()) for r in refs), sum(len(r.replace(" ", "")) for r in refs)
    _, total = sweep_reference(ac, lm_sum, n_tok, n_oov, err, -1000.0, alphas, betas)
    assert np.array_equal(out["grid_wer"], 100.0 * total[:, :, 0].astype(np.float64) / n_words)
    assert np.array_equal(out["grid_cer"], 100.0 * total[:, :, 1].astype(np.float64) / n_chars)
    # as planted: one word (one character) wrong per utterance without the LM, none with it, and the right answer is on every list
    assert out["first_pass"] == (100.0 * 8 / n_words, 100.0 * 8 / n_chars) and out["oracle"] == (0.0, 0.0)
    assert (out["grid_wer"][0] == out["first_pass"][0]).all() and (out["grid_wer"][1:] == 0.0).all()
    assert (out["alpha"], out["beta"], out["wer"], out["cer"]) == (0.5, -0.5, 0.0, 0.0)     # the first zero cell in row-major order
    assert tune_lm_weights(resc, batches, alphas, betas, metric="cer")["alpha"] == 0.5
