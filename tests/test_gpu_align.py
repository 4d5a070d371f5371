"""GPU (-m gpu): the CTC forced-alignment kernels (csrc/ctc_align.h, `ds2_ctc_align_f32`) against tests/ctc_align_oracle.py — bit for
bit with log-probability input, within a derived tolerance with probability input — plus CTCAligner and DeepSpeech.align end to end.
Shapes are the smallest at which each path can still go wrong; the oracle results are computed once per problem and shared."""
import functools
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import det
import ctc_align_oracle as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def log_softmax64(shape, seed, scale=4.0):
    z = det.uniform01(shape, seed).astype(np.float64) * scale
    z -= z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def pack(targets):
    lens = np.array([len(t) for t in targets], np.int32)
    off = np.zeros(len(targets), np.int32)
    off[1:] = np.cumsum(lens)[:-1]
    flat = np.array([c for t in targets for c in t], np.int32)
    return flat, off, lens


def run(dev, x, targets, in_lens, is_log, variant, x_dev=None):
    """One ops.ctc_forced_align call -> dict of numpy arrays.  x: (B,T,C) numpy, or x_dev a prepared device tensor / view."""
    from asr_amd import ops
    flat, off, lens = pack(targets)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev) if x_dev is None else x_dev
    t = lambda a: torch.from_numpy(a).to(dev)
    out = ops.ctc_forced_align(xd, t(flat), t(off), None if in_lens is None else t(np.asarray(in_lens, np.int32)), t(lens),
                               int(lens.max(initial=0)), is_log, variant)
    torch.cuda.synchronize()
    return dict(zip(("score", "states", "tok_start", "tok_end", "tok_logp"), (o.cpu().numpy() for o in out)))


def assert_same_bits(got, want, what=""):
    for k in ("score", "tok_logp"):
        assert np.array_equal(np.asarray(got[k], np.float32).view(np.int32), np.asarray(want[k], np.float32).view(np.int32)), (what, k, got[k], want[k])
    for k in ("states", "tok_start", "tok_end"):
        assert np.array_equal(got[k], want[k]), (what, k)


def cyc(n, C, start=0, doubled=()):
    """n labels cycling through 1..C-1 (no adjacent repeat), then label i made equal to label i-1 for i in `doubled`."""
    lab = [1 + (start + i) % (C - 1) for i in range(n)]
    for i in doubled:
        lab[i] = lab[i - 1]
    return lab


# ---- bit-exact, log-probabilities ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_problem():
    """B = 6, T = 37 (no multiple of the load ring), C = 29; T_b includes 37, 1 and 0; U: 7 with a doubled label, 1, 0, 18 at exactly the
    minimal T_b (two doubled labels: 20 frames), 20 one frame short, 63 at T_b = 37 (infeasible by length)."""
    T, C = 37, 29
    targets = [cyc(7, C, 3, doubled=(4,)), [5], [], cyc(18, C, 1, doubled=(3, 11)), cyc(20, C, 7), cyc(63, C, 2)]
    in_lens = [37, 1, 0, 20, 19, 37]
    x = log_softmax64((6, T, C), det.seed_of("align.ragged")).astype(np.float32)
    # -inf entries that leave the feasible cases feasible: utterance 0 has slack (a blank frame, a frame of its first label and of its
    # doubled label); utterance 3's path is forced, so only classes it never takes
    x[0, 5, 0] = x[0, 0, targets[0][0]] = x[0, 20, targets[0][4]] = x[0, 36, 0] = -np.inf
    unused = [c for c in range(1, C) if c not in targets[3]]
    x[3, :, unused[0]] = -np.inf
    x[1, 0, 0] = -np.inf
    want = A.align_batch(x, *pack(targets)[:2], in_lens, pack(targets)[2])
    return x, targets, in_lens, want


def test_ragged_problem_is_what_the_docstring_says():
    x, targets, in_lens, want = ragged_problem()
    assert np.isfinite(want["score"][[0, 1, 3]]).all() and want["score"][2] == 0 and np.isneginf(want["score"][[4, 5]]).all()
    assert (want["states"][4] == -1).all() and (want["states"][2] == -1).all() and want["states"][1, 0] == 1
    assert want["states"][3, 19] == 35 and want["states"][3, 0] == 1            # the forced path: first label at frame 0, last at T_b - 1


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_log_input_is_bit_exact_on_the_ragged_batch(dev, variant):
    x, targets, in_lens, want = ragged_problem()
    assert_same_bits(run(dev, x, targets, in_lens, True, variant), want, f"variant {variant}")


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_log_input_is_bit_exact_at_the_last_lane(dev, variant):
    """T = 140, U = 63 feasible (S = 127: the last lane's two states), next to U = 0 over 9 frames."""
    C = 29
    targets = [cyc(63, C, 5, doubled=(10, 40, 62)), []]
    in_lens = [140, 9]
    x = log_softmax64((2, 140, C), det.seed_of("align.lastlane")).astype(np.float32)
    want = A.align_batch(x, *pack(targets)[:2], in_lens, pack(targets)[2])
    assert np.isfinite(want["score"]).all() and want["states"][0].max() >= 125
    assert_same_bits(run(dev, x, targets, in_lens, True, variant), want)


@pytest.mark.parametrize("variant", [1, 2])
def test_tie_rule_on_the_device(dev, variant):
    """Emissions that are multiples of 0.25 (every sum exact, ties everywhere): T = 12, U = 4 with a repeat, B = 8."""
    B, T, C = 8, 12, 4
    q = det.randint((B, T, C), det.seed_of("align.ties"), 0, 3)
    x = (-0.25 * q).astype(np.float32)
    targets = [[1 + (b + i) % 3 for i in range(4)] for b in range(B)]
    for b in range(B):
        targets[b][1 + b % 3] = targets[b][b % 3]                               # a doubled label at a different place per utterance
    want = A.align_batch(x, *pack(targets)[:2], None, pack(targets)[2])
    assert np.isfinite(want["score"]).all()
    assert_same_bits(run(dev, x, targets, [T] * B, True, variant), want)


# ---- beyond one wavefront --------------------------------------------------------------------------------------------------------
def test_one_state_past_the_wavefront(dev):
    """U = 64 (S = 129): variant 1 is refused before any launch, variants 0 and 2 equal the oracle."""
    from asr_amd import _lib
    C = 29
    targets = [cyc(64, C, 0, doubled=(33,)), cyc(5, C, 9)]
    in_lens = [140, 77]
    x = log_softmax64((2, 140, C), det.seed_of("align.s129")).astype(np.float32)
    want = A.align_batch(x, *pack(targets)[:2], in_lens, pack(targets)[2])
    assert np.isfinite(want["score"]).all()
    with pytest.raises(_lib.DS2LibraryError, match="128"):
        run(dev, x, targets, in_lens, True, 1)
    for variant in (0, 2):
        assert_same_bits(run(dev, x, targets, in_lens, True, variant), want, f"variant {variant}")


def test_long_target_loops_over_states_per_thread(dev):
    """U = 1100 (1101 state pairs for 1024 threads), T = 1200, B = 2, C = 5."""
    C, T = 5, 1200
    targets = [cyc(1100, C, 0, doubled=(7, 500, 1099)), cyc(1000, C, 2, doubled=tuple(range(50, 1000, 100)))]
    in_lens = [1200, 1150]
    x = log_softmax64((2, T, C), det.seed_of("align.long"), scale=2.0).astype(np.float32)
    want = A.align_batch(x, *pack(targets)[:2], in_lens, pack(targets)[2])
    assert np.isfinite(want["score"]).all()
    assert_same_bits(run(dev, x, targets, in_lens, True, 2), want)
    assert_same_bits(run(dev, x, targets, in_lens, True, 0), want)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def test_layouts_give_identical_results(dev):
    x, targets, in_lens, want = ragged_problem()
    B, T, C = x.shape
    xt = torch.from_numpy(x).to(dev)
    tbc = xt.transpose(0, 1).contiguous()                                       # (T,B,C) storage, as the model's eval output
    padded = torch.full((B, T, C + 3), float("nan"), device=dev)
    padded[..., :C] = xt
    for name, view in (("(T,B,C)-backed", tbc.transpose(0, 1)), ("contiguous", xt), ("row pitch C + 3", padded[..., :C])):
        assert view.shape == (B, T, C) and view.stride(2) == 1
        assert_same_bits(run(dev, None, targets, in_lens, True, 0, x_dev=view), want, name)
    full = run(dev, x, targets, [T] * B, True, 0)
    assert_same_bits(run(dev, x, targets, None, True, 0), full, "in_lens = NULL")
    assert_same_bits(full, A.align_batch(x, *pack(targets)[:2], None, pack(targets)[2]), "all T")


# ---- probabilities ---------------------------------------------------------------------------------------------------------------
def planted(B, T, C, seed):
    rng = np.random.default_rng(seed)
    targets, paths = [], []
    for b in range(B):
        U = int(rng.integers(0, 13))
        lab = [int(v) for v in rng.integers(1, C, U)]
        if U >= 4:
            lab[2] = lab[1]
        S = 2 * U + 1
        visit = [s for s in range(S) if (s & 1) or rng.random() < 0.5
                 or (0 < s < S - 1 and lab[s // 2 - 1] == lab[s // 2])] or [0]
        cuts = np.sort(rng.choice(np.arange(1, T), len(visit) - 1, replace=False))
        runs = np.diff(np.concatenate(([0], cuts, [T])))
        path = np.repeat(visit, runs).astype(np.int32)
        assert A.check_path(path, lab) and len(path) == T
        targets.append(lab)
        paths.append(path)
    return targets, np.stack(paths)


@pytest.mark.parametrize("variant", [1, 2])
def test_probability_input_recovers_planted_alignments(dev, variant):
    """The planted path's class has p = 0.9 in every frame, the rest is spread evenly: any other alignment takes a class with p <= 0.1
    in at least one frame and scores at least log 9 lower, so the optimum is the planted path by construction."""
    B, T, C = 8, 40, 29
    targets, paths = planted(B, T, C, 20)
    p = np.full((B, T, C), 0.1 / (C - 1), np.float32)
    for b in range(B):
        cls = [A.state_class(int(s), targets[b]) for s in paths[b]]
        p[b, np.arange(T), cls] = 0.9
    got = run(dev, p, targets, None, False, variant)
    assert np.array_equal(got["states"], paths)
    assert np.allclose(got["score"], T * np.log(0.9), rtol=1e-5)


@functools.lru_cache(maxsize=None)
def soft_problem():
    B, T, C = 8, 40, 29
    targets, _ = planted(B, T, C, 21)
    p = np.exp(log_softmax64((B, T, C), det.seed_of("align.soft"), scale=6.0)).astype(np.float32)
    in_lens = [40, 40, 39, 33, 40, 31, 40, 40]
    e64 = np.log(p.astype(np.float64))
    best = [A.align(e64[b, :in_lens[b]], targets[b], np.float64) for b in range(B)]
    return p, targets, in_lens, e64, best


def soft_check(e64, targets, in_lens, best, score, states):
    """The issue's bound: the path is legal, its fp64 score is within 2 tol of the fp64 optimum, and the reported score within tol of the
    path's fp64 score; tol = T_b M (2^-22 + T_b 2^-24), M the largest finite |log p| of the utterance (2^-22: the hardware log2 and the
    ln 2 multiply; T_b 2^-24: T_b fp32 additions of partial sums bounded by T_b M)."""
    for b, tgt in enumerate(targets):
        Tb = in_lens[b]
        M = np.abs(e64[b, :Tb][np.isfinite(e64[b, :Tb])]).max()
        tol = Tb * M * (2.0 ** -22 + Tb * 2.0 ** -24)
        path = states[b, :Tb]
        assert A.check_path(path, tgt) and (states[b, Tb:] == -1).all(), b
        ps = float(A.path_score(e64[b], path, tgt, np.float64))
        print(f"soft b={b} Tb={Tb} tol={tol:.3e} optimum-path={float(best[b]['score']) - ps:.3e} score-path={float(score[b]) - ps:.3e}")
        assert ps >= float(best[b]["score"]) - 2 * tol, b
        assert abs(float(score[b]) - ps) <= tol, b


def test_soft_bound_holds_for_the_fp64_oracle_with_zero_slack():
    p, targets, in_lens, e64, best = soft_problem()
    states = np.full((len(targets), p.shape[1]), -1, np.int32)
    for b, r in enumerate(best):
        assert r["feasible"]
        states[b, :in_lens[b]] = r["states"]
        assert float(A.path_score(e64[b], r["states"], targets[b])) == float(r["score"])
    soft_check(e64, targets, in_lens, best, np.array([r["score"] for r in best]), states)


@pytest.mark.parametrize("variant", [1, 2])
def test_probability_input_on_soft_frames(dev, variant):
    p, targets, in_lens, e64, best = soft_problem()
    got = run(dev, p, targets, in_lens, False, variant)
    soft_check(e64, targets, in_lens, best, got["score"], got["states"])
    # the spans and their sums describe the returned path
    flat, off, lens = pack(targets)
    for b, tgt in enumerate(targets):
        sp = A.spans(e64[b], got["states"][b, :in_lens[b]], tgt, np.float64)
        sl = slice(off[b], off[b] + lens[b])
        assert np.array_equal(got["tok_start"][sl], sp["tok_start"]) and np.array_equal(got["tok_end"][sl], sp["tok_end"])
        assert np.allclose(got["tok_logp"][sl], sp["tok_logp"], rtol=1e-5, atol=1e-5)


def test_variants_write_the_same_bits_for_probability_input(dev):
    p, targets, in_lens, _, _ = soft_problem()
    assert_same_bits(run(dev, p, targets, in_lens, False, 2), run(dev, p, targets, in_lens, False, 1))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_model_align_end_to_end(dev):
    import pandas as pd
    from asr_amd import DeepSpeech
    from asr_amd.decoders import CTCAligner, GreedyDecoder
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
    sizes = torch.tensor([80, 66, 51, 40], dtype=torch.int32)
    x = torch.from_numpy(det.unitvar((4, 1, 161, 80), det.seed_of("align.e2e")))
    for b, n in enumerate(sizes.tolist()):
        x[b, :, :, n:] = 0
    x = x.to(dev)
    with torch.no_grad():
        probs, out_sizes = model.forward(x, sizes)
    strings, _ = GreedyDecoder(model.labels).decode(probs, out_sizes)
    transcripts = [s[0] for s in strings]
    if any(len(t) == 0 for t in transcripts):                                    # a random-init model may decode nothing
        transcripts = [("ab a " * 8)[:max(1, int(n) // 3)] for n in out_sizes.tolist()]
    records = model.align(x, sizes, transcripts)
    plain = CTCAligner(model.labels).align(probs, out_sizes, transcripts)
    assert len(records) == 4
    for b, r in enumerate(records):
        Tb = int(out_sizes[b])
        assert np.isfinite(r["score"]) and r["states"].numel() == Tb and torch.equal(r["states"], plain[b]["states"])
        assert r["score"] == plain[b]["score"]
        assert "".join(t[0] for t in r["tokens"]) == transcripts[b]
        prev_end = 0
        for ch, s, e, lp, s_s, e_s in r["tokens"]:
            assert prev_end <= s < e <= Tb and np.isfinite(lp)
            assert s_s == s * 2 * conf.window_stride and e_s == e * 2 * conf.window_stride
            prev_end = e
        assert [w[0] for w in r["words"]] == transcripts[b].split()
        toks = [t for t in r["tokens"] if t[0] != " "]
        for w in r["words"]:
            mine, toks = toks[:len(w[0])], toks[len(w[0]):]
            assert w[1] == mine[0][1] and w[2] == mine[-1][2] and w[3] == float(sum(np.float64(t[3]) for t in mine))
            assert w[4] == w[1] * 2 * conf.window_stride and w[5] == w[2] * 2 * conf.window_stride


def test_errors(dev):
    from asr_amd.decoders import CTCAligner
    al = CTCAligner({c: i for i, c in enumerate("_ab ")})
    probs = torch.full((2, 5, 4), 0.25)                                          # a host tensor: uploaded first
    with pytest.raises(ValueError, match="1 transcripts for a batch of 2"):
        al.align(probs, None, ["ab"])
    recs = al.align(probs, [5, 2], ["ab", "a b"])                               # the second one cannot fit: 3 labels in 2 frames
    assert np.isfinite(recs[0]["score"]) and recs[1] == {"score": float("-inf"), "states": recs[1]["states"], "tokens": [], "words": []}
    want = A.align(np.full((5, 4), np.log(0.25)), [1, 2])                       # every alignment ties: the tie rule decides
    assert recs[0]["states"].tolist() == want["states"].tolist() == [1, 3, 4, 4, 4]
    assert [t[:3] for t in recs[0]["tokens"]] == [("a", 0, 1), ("b", 1, 2)]
