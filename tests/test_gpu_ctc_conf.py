"""-m gpu: the word / character confidences (ds2_ctc_conf_f32, ops.ctc_confidence, CTCConfidence, DeepSpeech.confidence) against
their fp64 restatement (tests/ctc_conf_oracle.py).  The bar is the suite's nll bar of tests/test_gpu_ctc_star.py and
tests/test_gpu_ctc_mwer.py (rtol 1e-5, atol 1e-4) applied to each of the three log-sums a result is made of:
|logconf - oracle| <= 3 * (1e-4 + 1e-5 * M), M the largest magnitude of the oracle's num, A and Bq; NaN and -inf patterns match
exactly.  MI355X figures are in profiles/ctc_conf_timing.txt."""
import numpy as np
import pytest
import torch

import ctc_conf_oracle as O

pytestmark = pytest.mark.gpu

_CACHE = {}


def _fixture(name):
    if name not in _CACHE:
        f = O.fixture_a() if name == "a" else O.fixture_b()
        f["logits"] = f["logits"].astype(np.float32)                # what the kernels see
        f["oracle"] = O.confidence(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], max_hyp_len=f["max_hyp_len"])
        for a in (f["logits"],) + f["oracle"]:
            a.setflags(write=False)
        _CACHE[name] = f
    return _CACHE[name]


def _run(logits, hyps, in_lens, units, w_max, max_hyp_len, lattice=0, n_units=None):
    """ops.ctc_confidence on host arrays -> (nll (B), logconf (B, W_max)) as fp32 numpy arrays"""
    from asr_amd import ops
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    dev = torch.device("cuda:0")
    B = len(hyps)
    flat = [7, 7, 7] + [i for h in hyps for i in h]                 # (offsets do not start at 0)
    lens = [len(h) for h in hyps]
    off = np.concatenate([[3], 3 + np.cumsum(lens)[:-1]]).astype(np.int64)
    grid = np.full((4, B, w_max), -7, np.int64)                     # (slots beyond n_units hold garbage)
    for b, us in enumerate(units):
        for w, u in enumerate(us):
            grid[:, b, w] = u
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)          # noqa: E731
    nu = [len(u) for u in units] if n_units is None else n_units
    nll, lc = ops.ctc_confidence(torch.from_numpy(np.ascontiguousarray(logits, np.float32).copy()).to(dev), t(flat, torch.int32), t(off, torch.int64),
                                 t(lens, torch.int32), t(in_lens, torch.int32), max_hyp_len, t(nu, torch.int32), t(grid[0], torch.int32),
                                 t(grid[1], torch.int32), t(grid[2], torch.int32), t(grid[3], torch.int32), lattice=lattice)
    torch.cuda.synchronize()
    return nll.cpu().numpy(), lc.cpu().numpy()


def _run_fixture(f, **kw):
    return _run(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], f["max_hyp_len"], **kw)


def _check(what, got, want):
    nll, lc = (a.astype(np.float64) for a in got)
    wn, wl, mag = want
    assert (np.isinf(nll) == np.isinf(wn)).all() and (nll[np.isinf(nll)] > 0).all(), (what, nll, wn)
    fin = np.isfinite(wn)
    assert (np.abs(nll[fin] - wn[fin]) <= 1e-4 + 1e-5 * np.abs(wn[fin])).all(), (what, nll, wn)
    assert (np.isnan(lc) == np.isnan(wl)).all(), (what, lc, wl)
    assert ((lc == -np.inf) == (wl == -np.inf)).all(), (what, lc, wl)
    ok = np.isfinite(wl)
    assert np.isfinite(lc[ok]).all() and (lc[ok] <= 0).all(), (what, lc)
    err, bar = np.abs(lc[ok] - wl[ok]), 3.0 * (1e-4 + 1e-5 * mag[ok])
    i = int(np.argmax(err / bar))
    print(f"{what}: {int(ok.sum())} finite units, logconf err max {err.max():.2e} (worst against its bar: {err[i]:.2e} of {bar[i]:.2e}, "
          f"M = {mag[ok][i]:.1f}); largest M {mag[ok].max():.1f}")
    assert (err <= bar).all(), what


@pytest.mark.parametrize("name", ["a", "b"])
def test_against_the_oracle(name):
    f = _fixture(name)
    got = _run_fixture(f)
    _check(f"fixture {name}", got, f["oracle"])
    if name == "a":
        assert np.isfinite(got[1][0, :12]).all() and got[1][0, 12] == -np.inf and np.isnan(got[1][0, 13:]).all()
        assert np.isnan(got[1][1, 0]) and got[1][1, 1] == -np.inf and np.isnan(got[1][2]).all() and got[0][1] == np.inf
    else:
        assert np.isfinite(got[1][0, :2]).all() and np.isnan(got[1][0, 2])     # 63 labels are scored, 64 are not


def test_both_lattice_kernels_and_a_rerun_give_the_same_bits():
    f = _fixture("a")
    a, b, c = _run_fixture(f), _run_fixture(f, lattice=1), _run_fixture(f)
    for x, y in ((a, b), (a, c)):
        assert np.array_equal(x[0].view(np.int32), y[0].view(np.int32)) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32))
    _check("fixture a, lattice = 1", b, f["oracle"])


def test_bits_do_not_depend_on_the_batch_or_the_slot():
    f = _fixture("a")
    base = _run_fixture(f)
    # utterance 0 alone, its units in reverse order; then as the last of B = 4 behind copies of utterance 1
    n = len(f["units"][0])
    alone = _run(f["logits"][:, :1], f["hyps"][:1], f["in_lens"][:1], [f["units"][0][::-1]], n, f["max_hyp_len"])
    assert alone[0].view(np.int32)[0] == base[0].view(np.int32)[0]
    assert np.array_equal(alone[1][0, ::-1].view(np.int32), base[1][0, :n].view(np.int32))
    order = [1, 1, 2, 0]
    moved = _run(f["logits"][:, order], [f["hyps"][i] for i in order], [f["in_lens"][i] for i in order], [f["units"][i] for i in order],
                 f["w_max"], f["max_hyp_len"])
    for k, i in enumerate(order):
        assert moved[0].view(np.int32)[k] == base[0].view(np.int32)[i]
        assert np.array_equal(moved[1][k].view(np.int32), base[1][i].view(np.int32))


def test_counts_outside_the_slots_and_bad_hypotheses_void_only_their_utterance():
    f = _fixture("a")
    base = _run_fixture(f)
    got = _run_fixture(f, n_units=[f["w_max"] + 1, -1, 1])
    assert np.isnan(got[1][:2]).all() and np.array_equal(got[0].view(np.int32), base[0].view(np.int32))
    hyps = [f["hyps"][0], [1, f["C"], 2], [1, 2, 3, 4, 1, 2]]           # a label outside [1, C-1]; a length above max_hyp_len
    units = [f["units"][0], [(0, 1, 0, 3)], [(0, 1, 0, 1)]]
    got = _run(f["logits"], hyps, f["in_lens"], units, f["w_max"], f["max_hyp_len"])
    assert np.array_equal(got[1][0].view(np.int32), base[1][0].view(np.int32)) and got[0][0] == base[0][0]
    assert np.isnan(got[1][1:]).all() and (got[0][1:] == np.inf).all()


def _log(conf):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(conf, np.float64))


def test_score_on_the_planted_posteriors_gives_1_and_a_quarter():
    from asr_amd import CTCConfidence
    p, y, units, want = O.planted()
    probs = torch.from_numpy(p.astype(np.float32))[None].cuda()
    recs = CTCConfidence("_ab ").score(probs, None, ["a a"])
    assert len(recs) == 1 and set(recs[0]) == {"nll", "units"}
    assert abs(recs[0]["nll"] + np.log(0.25)) <= 1e-4
    got = recs[0]["units"]
    assert [u[:3] for u in got] == [("a", 0, 2), ("a", 4, 6)]              # the aligner's spans are the planted windows
    for u, w in zip(got, want):                                              # M = log 4: num of both, and Bq of the first
        assert 0.0 < u[3] <= 1.0 and abs(_log(u[3]) - np.log(w)) <= 3.0 * (1e-4 + 1e-5 * np.log(4.0)), (u, w)
    chars = CTCConfidence("_ab ").score(probs.log(), torch.tensor([7]), ["a a"], is_log=True, unit="char", margin=1)[0]["units"]
    assert [u[:3] for u in chars] == [("a", 0, 3), (" ", 2, 5), ("a", 3, 7)]
    # a widened window takes frames from its neighbours: the last one holds the only frame of the space, so the frames before it
    # cannot spell "a " and the context is impossible on these one-hot posteriors (the oracle: 1, 0.5, NaN)
    bar = 3.0 * (1e-4 + 1e-5 * np.log(4.0))                                  # M = log 4 again: num = log 0.25 in both
    assert abs(_log(chars[0][3])) <= bar and abs(_log(chars[1][3]) - np.log(0.5)) <= bar and np.isnan(chars[2][3])
    # an infeasible text has no units
    assert CTCConfidence("_ab ").score(probs[:, :2], None, ["a a"])[0]["units"] == []


def _oracle_units(logp, sizes, texts, labels, unit, margin):
    """What CTCConfidence.score must return on log-posteriors logp (B,T,C) fp32 (GPU): the aligner's spans, the unit builder, the oracle"""
    from asr_amd.decoders import CTCAligner, confidence_units, encode_transcripts
    recs = CTCAligner(labels).align(logp, sizes, texts, is_log=True)
    hyps = encode_transcripts(texts, labels)
    units = [confidence_units(t, [(k[1], k[2]) for k in r["tokens"]], int(n), unit, margin) if r["tokens"] else []
             for t, r, n in zip(texts, recs, sizes.tolist())]
    print(f"aligned {texts!r} ({unit}, margin {margin}): scores {[r['score'] for r in recs]}, {[len(us) for us in units]} units")
    _, lc, mag = O.confidence(logp.transpose(0, 1).cpu().numpy(), hyps, sizes.tolist(), [[u[1:] for u in us] for us in units])
    return units, lc, mag


def test_model_confidence_equals_the_oracle_on_the_models_posteriors():
    from asr_amd import CTCConfidence
    from test_gpu_align_long import spectrogram, tiny_model
    model = tiny_model()
    x = torch.stack((spectrogram(100), spectrogram(100).flip(1)))[:, None].cuda()
    sizes = torch.tensor([100, 77], dtype=torch.int32)
    recs = model.confidence(x, sizes)
    assert len(recs) == 2 and all(set(r) == {"text", "words", "confidence"} for r in recs) and not model.training
    plain = model.transcribe(x, sizes)
    assert [(r["text"], r["words"]) for r in recs] == [(r["text"], r["words"]) for r in plain]
    assert all(len(r["confidence"]) == len(r["words"]) for r in recs)
    with torch.no_grad():
        probs, out_sizes = model.forward(x, sizes)
    logp = torch.log(probs.float())
    chars = "_'abcdefghijklmnopqrstuvwxy "                                  # the model's 28 classes with the last one read as the space
    assert probs.shape[2] == len(chars)
    cases = [([r["text"] for r in recs], "word", 0, [r["confidence"] for r in recs], model.labels),
             (["ab a 'it", "q  b"], "word", 0, None, chars), (["ab a 'it", "q  b"], "char", 2, None, chars)]   # (a random-init model may decode nothing)
    scored = 0
    for texts, unit, margin, conf, labels in cases:
        units, lc, mag = _oracle_units(logp, out_sizes, texts, labels, unit, margin)
        if conf is None:
            got = CTCConfidence(labels).score(probs, out_sizes, texts, unit=unit, margin=margin)
            assert [[u[:3] for u in g["units"]] for g in got] == [[(u[0], u[3], u[4]) for u in us] for us in units]
            conf = [[u[3] for u in g["units"]] for g in got]
        for b, us in enumerate(units):
            assert len(conf[b]) == len(us)
            for w in range(len(us)):
                if np.isnan(lc[b, w]):                                 # a margin that reaches frame 0 or T_b past labels still outside: no context
                    assert margin > 0 and np.isnan(conf[b][w]) and (us[w][3] == 0 or us[w][4] == int(out_sizes[b])), (texts[b], us[w])
                    continue
                assert np.isfinite(lc[b, w]) and 0.0 < conf[b][w] <= 1.0, (texts[b], us[w], lc[b, w], conf[b][w])
                err, bar = abs(_log(conf[b][w]) - lc[b, w]), 3.0 * (1e-4 + 1e-5 * mag[b, w])
                assert err <= bar, (texts[b], us[w], err, bar)
                scored += 1
    print(f"model posteriors: {scored} units within the bar")
    assert scored >= 8
    # one recording, three windows: every segment gains its confidences, the units' frames are the recording's
    spect = spectrogram(437)
    opts = dict(window=128, overlap=16, batch_size=3, decode_batch=4, threshold=0.05, min_gap=2, pad=1, max_len=30)
    rec, base = model.confidence_long(spect, **opts), model.transcribe_long(spect, **opts)
    assert rec["text"] == base["text"] and len(rec["segments"]) == len(base["segments"]) > 1
    for s, t in zip(rec["segments"], base["segments"]):
        assert {k: v for k, v in s.items() if k not in ("confidence", "units")} == t
        assert len(s["confidence"]) == len(s["words"])
        assert all(s["start"] <= u[1] < u[2] <= s["end"] for u in s["units"])
        assert [u[0] for u in s["units"]] == s["text"].split()
