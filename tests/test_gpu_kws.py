"""GPU (-m gpu): keyword search over CTC posteriors (csrc/ctc_kws.h, `ds2_ctc_kws_f32`) against tests/ctc_kws_oracle.py — all six outputs
bit for bit with log-probability input (scores after + 0.0f), hits equal and scores within a derived tolerance with probability input —
plus KeywordSpotter and DeepSpeech.spot / spot_long end to end.  Shapes are the smallest at which each path can still go wrong; the
oracle results are computed once per problem and shared."""
import functools
import math
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import det
import ctc_kws_oracle as K
import kws_problems as P

pytestmark = pytest.mark.gpu

NAMES = ("frame_score", "frame_start", "hit_start", "hit_end", "hit_score", "n_hits")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def log_softmax64(shape, seed, scale=4.0):
    z = det.uniform01(shape, seed).astype(np.float64) * scale
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def pack(kws):
    lens = np.array([len(k) for k in kws], np.int32)
    off = np.zeros(len(kws), np.int32)
    off[1:] = np.cumsum(lens)[:-1]
    return np.array([c for k in kws for c in k], np.int32), off, lens


def run(dev, x, kws, thr, in_lens, is_log, max_hits, x_dev=None, max_kw_len=None):
    from asr_amd import ops
    flat, off, lens = pack(kws)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev) if x_dev is None else x_dev
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.int32)).to(dev)
    out = ops.ctc_keyword_search(xd, t(flat), t(off), t(lens), int(lens.max(initial=0)) if max_kw_len is None else max_kw_len,
                                 torch.from_numpy(np.asarray(thr, np.float32)).to(dev), t(in_lens), is_log, max_hits)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def assert_same_bits(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = (g + np.float32(0)).view(np.int32), (w + np.float32(0)).view(np.int32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def cyc(n, C, start=0, doubled=()):
    """n labels cycling through 1..C-1 (no adjacent repeat), label i made equal to label i-1 for i in `doubled`"""
    lab = [1 + (start + i) % (C - 1) for i in range(n)]
    for i in doubled:
        lab[i] = lab[i - 1]
    return lab


def thresholds(want_frames, q=0.7):
    """One threshold per keyword, read off the oracle's own frame scores so that the pick has work to do: the q-quantile of the finite
    scores over the batch (a value that IS a score: the comparison is inclusive), -1 where no frame is finite."""
    K_ = want_frames.shape[1]
    thr = np.full(K_, -1.0, np.float32)
    for k in range(K_):
        f = np.sort(want_frames[:, k][np.isfinite(want_frames[:, k])])
        if f.size:
            thr[k] = f[int(q * (f.size - 1))]
    return thr


def problem(x, kws, in_lens, max_hits, q=0.7):
    B, T, _ = x.shape
    frames = np.stack([np.stack([K.kws_frames(x[b, :T if in_lens is None else max(min(in_lens[b], T), 0)], kw, T)[0] for kw in kws])
                       for b in range(B)])
    thr = thresholds(frames, q)
    return x, kws, in_lens, thr, max_hits, P.batch32(x, in_lens, kws, thr, max_hits)


# ---- bit-exact, log-probabilities ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_problem():
    """B = 4, T = 37 (no multiple of the load ring), C = 29, T_b = (37, 1, 0, 20); keywords: U = 1, U = 3 with a doubled label, U = 7,
    U = 20 (longer than T_b = 1, and than what 20 frames hold comfortably), U = 0, a label C; -inf entries in x."""
    T, C = 37, 29
    kws = [[5], [4, 4, 9], cyc(7, C, 2), cyc(20, C, 11, doubled=(6,)), [], [3, C]]
    x = log_softmax64((4, T, C), det.seed_of("kws.ragged")).astype(np.float32)
    x[0, 5, 0] = x[0, 20, 5] = x[0, 21, 4] = x[3, 0, 5] = x[3, 7, 9] = -np.inf
    return problem(x, kws, [37, 1, 0, 20], 4)


def test_ragged_problem_is_what_the_docstring_says():
    x, kws, in_lens, thr, max_hits, want = ragged_problem()
    fs, fst, hs, he, hv, nh = want
    assert np.isfinite(fs[0, :4]).any(axis=1).all() and not np.isfinite(fs[:, 4:]).any() and (nh[:, 4:] == 0).all()
    assert not np.isfinite(fs[2]).any() and (fst[2] == -1).all() and not np.isfinite(fs[1, :, 1:]).any()
    assert np.isfinite(fs[1, 0, 0]) and not np.isfinite(fs[1, 1:, 0]).any()          # one frame holds a keyword of one label only
    assert (nh == max_hits + 1).any() and ((nh > 0) & (nh <= max_hits)).any() and (hs[nh == 0] == -1).all()


def test_ragged_batch_bit_for_bit(dev):
    x, kws, in_lens, thr, max_hits, want = ragged_problem()
    assert_same_bits(run(dev, x, kws, thr, in_lens, True, max_hits), want)
    # a max_kw_len above the longest keyword changes nothing; one below it turns the longer keywords into keywords without a hit
    assert_same_bits(run(dev, x, kws, thr, in_lens, True, max_hits, max_kw_len=63), want)
    got = run(dev, x, kws, thr, in_lens, True, max_hits, max_kw_len=3)
    short = [k if len(k) <= 3 else [] for k in kws]
    assert_same_bits(got, P.batch32(x, in_lens, short, thr, max_hits), "max_kw_len = 3")


@functools.lru_cache(maxsize=None)
def last_lane_problem():
    """U = 63 fills the wavefront's pairs 0 .. 62; T = 140 crosses two blocks of 64 stored frames.  Utterance 0 has the keyword planted
    (each label the best class for two frames); utterance 1 has T_b = 9 next to a keyword of one label."""
    T, C = 140, 29
    long = cyc(63, C, 3, doubled=(10, 40))
    x64 = log_softmax64((2, T, C), det.seed_of("kws.lastlane"))
    t = 5
    for u, c in enumerate(long):
        if u and long[u - 1] == c:
            x64[0, t, 0] = 0.5
            t += 1
        x64[0, t:t + 2, c] = 0.5
        t += 2
    assert t < T
    x = (x64 - np.log(np.exp(x64).sum(-1, keepdims=True))).astype(np.float32)
    return problem(x, [long, [7]], [140, 9], 8, q=0.9)


def test_last_lane_bit_for_bit(dev):
    x, kws, in_lens, thr, max_hits, want = last_lane_problem()
    fs, fst, hs, he, hv, nh = want
    assert nh[0, 0] >= 1 and hv[0, 0, 0] == 0 and hs[0, 0, 0] == 5 and he[0, 0, 0] - hs[0, 0, 0] >= 2 * 63 + 1   # the plant, to its first best end
    assert not np.isfinite(fs[1, 0]).any() and np.isfinite(fs[1, 1, :9]).all() and not np.isfinite(fs[1, 1, 9:]).any()
    assert_same_bits(run(dev, x, kws, thr, in_lens, True, max_hits), want)


def test_tie_rules_on_the_device(dev):
    for tie in (P.TIE_ENTER, P.TIE_STAY_STEP, P.TIE_STEP_SKIP):
        x = P.tie_e(tie)[None]
        kws = [tie["labels"]]
        thr = np.array([-100.0], np.float32)
        want = P.batch32(x, None, kws, thr, 4)
        if "t" in tie:
            assert want[1][0, 0, tie["t"]] == tie["winner"]
        assert_same_bits(run(dev, x, kws, thr, None, True, 4), want, tie["labels"])


@functools.lru_cache(maxsize=None)
def grid_problem():
    """K = 130 keywords (more than a wavefront's lanes, more than 127), B = 3, T = 20: the (utterance, keyword) of every workgroup"""
    T, C = 20, 11
    kws = [cyc(1 + k % 4, C, k) for k in range(130)]
    x = log_softmax64((3, T, C), det.seed_of("kws.grid")).astype(np.float32)
    return problem(x, kws, [20, 13, 17], 2, q=0.5)


def test_grid_indexing_bit_for_bit(dev):
    x, kws, in_lens, thr, max_hits, want = grid_problem()
    assert_same_bits(run(dev, x, kws, thr, in_lens, True, max_hits), want)


@functools.lru_cache(maxsize=None)
def edge_problem(T):
    C = 9
    x = log_softmax64((1, T, C), det.seed_of(f"kws.edge.{T}"), scale=6.0).astype(np.float32)
    return problem(x, [[2, 5, 2], [8]], None, 16, q=0.995 if T > 100 else 0.0)


@pytest.mark.parametrize("T", [1, 5000])
def test_prefetch_edges_bit_for_bit(dev, T):
    """T = 1: the load ring is clamped to the only frame; T = 5000 = 78 * 64 + 8: whole blocks of stored frames, then one whole load group
    and no tail.  The ragged problem (37, 20) and the last-lane one (140, 9) have tails of 5, 4, 4 and 1 frames."""
    x, kws, in_lens, thr, max_hits, want = edge_problem(T)
    assert T != 5000 or want[5].max() >= 2
    assert_same_bits(run(dev, x, kws, thr, in_lens, True, max_hits), want)


def test_pick_fills_the_slots_and_a_threshold_excludes(dev):
    p, kws = P.planted_five()
    x = P.as_log32(p)
    for threshold, max_hits, n in ((0.02, 3, 4), (0.02, 8, 5), (0.5, 8, 3)):
        thr = P.thr_of(kws, threshold)
        want = P.batch32(x, None, kws, thr, max_hits)
        assert want[5].tolist() == [[n]]
        assert_same_bits(run(dev, x, kws, thr, None, True, max_hits), want, (threshold, max_hits))
    p, kws, thr = P.planted_three()
    want = P.batch32(P.as_log32(p), None, kws, thr, 8)
    assert want[5].tolist() == [[3, 0]]
    assert_same_bits(run(dev, P.as_log32(p), kws, thr, None, True, 8), want, "three plants")


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def test_strided_input_gives_identical_results(dev):
    x, kws, in_lens, thr, max_hits, want = ragged_problem()
    B, T, C = x.shape
    xt = torch.from_numpy(x).to(dev)
    tbc = xt.transpose(0, 1).contiguous()                                       # (T,B,C) storage, as the model's eval output
    padded = torch.full((B, T, C + 3), float("nan"), device=dev)
    padded[..., :C] = xt
    for name, view in (("(T,B,C)-backed", tbc.transpose(0, 1)), ("row pitch C + 3", padded[..., :C])):
        assert view.shape == (B, T, C) and view.stride(2) == 1 and not view.is_contiguous()
        assert_same_bits(run(dev, None, kws, thr, in_lens, True, max_hits, x_dev=view), want, name)


# ---- probabilities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["three", "five@0.5", "five@0.02"])
def test_probability_input_within_the_derived_bound(dev, which):
    """is_log = 0 on the planted problems (whose margins tests/test_cpu_kws.py asserts): the hits are the float64 oracle's on the logs of
    the same float32 probabilities, and every score is within tol = 2 n M (2^-22 + n 2^-24) of it, n the frames of its span."""
    if which == "three":
        p, kws, thr = P.planted_three()
        max_hits = 8
    else:
        p, kws = P.planted_five()
        thr, max_hits = P.thr_of(kws, float(which.split("@")[1])), 3 if which.endswith("0.02") else 8
    x = p.astype(np.float32)
    M = np.abs(np.log(x.astype(np.float64))).max()
    wfs, wfst, whs, whe, whv, wnh = K.kws_batch(x, None, kws, thr, max_hits, False, np.float64)
    fs, fst, hs, he, hv, nh = run(dev, x, kws, thr, None, False, max_hits)
    assert np.array_equal(nh, wnh) and np.array_equal(hs, whs) and np.array_equal(he, whe)
    used = whs >= 0
    n = (whe - whs)[used]
    err = np.abs(hv[used].astype(np.float64) - whv[used])
    print("hit score errors", err.tolist(), "bounds", P.prob_tol(n, M).tolist())
    assert (err <= P.prob_tol(n, M)).all() and (hv[~used] == -np.inf).all()
    finite = np.isfinite(wfs)
    assert np.array_equal(np.isfinite(fs), finite)
    nf = (np.arange(x.shape[1])[None, None, :] + 1 - wfst)[finite]
    ferr = np.abs(fs[finite].astype(np.float64) - wfs[finite])
    print("largest frame score error / bound", float((ferr / P.prob_tol(nf, M)).max()))
    assert (ferr <= P.prob_tol(nf, M)).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:KeywordSpotter.search")        # (flat posteriors overflow max_hits = 4; the warning has its own check below)
def test_spotter_and_model_end_to_end(dev):
    import pandas as pd
    from asr_amd import DeepSpeech, KeywordSpotter
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                           spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    torch.manual_seed(3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": chars}).to_csv(path, index=False)
        model = DeepSpeech(audio_conf=conf, decoder=None, label_path=path, rnn_type="gru", rnn_hidden_size=32, rnn_hidden_layers=2,
                           bidirectional=True)
    model.to(dev).eval()
    sizes = torch.tensor([80, 66, 51], dtype=torch.int32)
    x = torch.from_numpy(det.unitvar((3, 1, 161, 80), det.seed_of("kws.e2e")))
    for b, n in enumerate(sizes.tolist()):
        x[b, :, :, n:] = 0
    x = x.to(dev)
    keywords, fsec = ["ab", "it's", "q"], 2 * conf.window_stride
    with torch.no_grad():
        probs, out_sizes = model.forward(x, sizes)
    # an untrained model's posteriors are nearly flat: a low threshold makes every keyword fire, a high one none
    spotter = KeywordSpotter(model.labels, keywords, threshold=0.5, max_hits=4)
    recs = spotter.search(probs, out_sizes, frame_seconds=fsec)
    assert len(recs) == 3 and sum(len(r) for r in recs) > 0
    for b, utt in enumerate(recs):
        assert utt == sorted(utt, key=lambda r: r["start"])
        for r in utt:
            assert r["keyword"] in keywords and 0 <= r["start"] < r["end"] <= int(out_sizes[b]) and r["score"] <= 0
            assert r["end"] - r["start"] >= len(r["keyword"]) and 0 < r["confidence"] <= 1
            assert r["confidence"] == math.exp(r["score"] / len(r["keyword"])) and r["score"] >= len(r["keyword"]) * np.log(0.5) - 1e-6
            assert r["start_s"] == r["start"] * fsec and r["end_s"] == r["end"] * fsec
        for kw in keywords:                                                     # detections of one keyword do not overlap
            spans = [(r["start"], r["end"]) for r in utt if r["keyword"] == kw]
            assert all(a[1] <= b_[0] for a, b_ in zip(spans, spans[1:]))
    # on the logs of the same posteriors the records are the float32 oracle's, bit for bit
    logp = probs.clamp_min(1e-30).log()
    lrecs = spotter.search(logp, out_sizes, is_log=True)
    want = P.batch32(logp.cpu().numpy(), out_sizes.tolist(), spotter.kw_ids, spotter.thr, 4)
    for b, utt in enumerate(lrecs):
        for k, kw in enumerate(keywords):
            got = sorted((r["start"], r["end"], r["score"]) for r in utt if r["keyword"] == kw)
            n = min(int(want[5][b, k]), 4)
            assert got == sorted(zip(want[2][b, k, :n].tolist(), want[3][b, k, :n].tolist(), want[4][b, k, :n].tolist())), (b, kw)
    assert model.spot(x, sizes, keywords, threshold=0.5, max_hits=4) == recs
    assert all(r == [] for r in KeywordSpotter(model.labels, ["abcdefgh"], threshold=0.999).search(probs, out_sizes))
    with pytest.warns(RuntimeWarning, match="max_hits=1"):
        KeywordSpotter(model.labels, ["q"], threshold=0.01, max_hits=1).search(probs, out_sizes)
    # one recording three windows long: spot_long is search on posteriors_long's output
    spect = x[0, 0, :, :80]
    long_probs = model.posteriors_long(spect, window=40, overlap=8, batch_size=2)
    from asr_amd.functional import long_windows
    assert len(long_windows(80, 40, 8)) == 3 and long_probs.shape[0] == 40
    want_long = spotter.search(long_probs[None], None, frame_seconds=fsec)[0]
    assert model.spot_long(spect, keywords, window=40, overlap=8, batch_size=2, threshold=0.5, max_hits=4) == want_long
    assert len(want_long) > 0


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    from asr_amd import KeywordSpotter, ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    x = torch.zeros((1, 4, 5), device=dev)
    thr = torch.zeros(1, device=dev)
    with pytest.raises(ValueError, match="GPU"):
        ops.ctc_keyword_search(x.cpu(), i32(1), i32(0), i32(1), 1, thr)
    with pytest.raises(ValueError, match="kw_lens"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1).cpu(), 1, thr)
    with pytest.raises(ValueError, match="thr"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, thr.double())
    with pytest.raises(ValueError, match="in_lens"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, thr, in_lens=torch.tensor([4]))
    with pytest.raises(ValueError, match="max_kw_len"):
        ops.ctc_keyword_search(x, i32(*([1] * 64)), i32(0), i32(64), 64, thr)
    with pytest.raises(ValueError, match="max_hits"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, thr, max_hits=1025)
    with pytest.raises(ValueError, match="thresholds"):
        ops.ctc_keyword_search(x, i32(1), i32(0), i32(1), 1, torch.zeros(2, device=dev))
    with pytest.raises(ValueError, match="contiguous class"):
        ops.ctc_keyword_search(x.transpose(1, 2), i32(1), i32(0), i32(1), 1, thr)
    with pytest.raises(ValueError, match="threshold"):
        KeywordSpotter("_ab ", ["ab"], threshold=1.01)
    with pytest.raises(ValueError, match="63"):
        KeywordSpotter("_ab ", ["ab" * 32])
    # a kw_lens entry above max_kw_len is a keyword without a hit, not an error and not an overrun
    fs, fst, hs, he, hv, nh = ops.ctc_keyword_search(x, i32(1, 2, 1), i32(0), i32(3), 2, thr, is_log=True)
    assert not torch.isfinite(fs).any() and (fst == -1).all() and int(nh) == 0
