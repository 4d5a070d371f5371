"""CPU (-m "not gpu"): the wildcard / free-ends oracle (tests/ctc_align_star_oracle.py) against brute force and against the plain oracle,
the planted problem, the host half of CTCAligner's new options, and the argument checks of the new entries (include/ds2hip.h,
ds2_ctc_align_star_f32)."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import det  # noqa: E402

import align_star_problems as P  # noqa: E402
import ctc_align_oracle as A  # noqa: E402
import ctc_align_star_oracle as S  # noqa: E402


def quarter_emissions(T, C, seed, levels=5, neg_inf=False):
    q = det.randint((T, C), seed, 0, levels)
    e = (-0.25 * q).astype(np.float32)
    if neg_inf:
        e[q == levels - 1] = -np.inf
    return e


def test_oracle_equals_brute_force_on_every_tiny_problem():
    """T <= 5, U <= 2 over the labels {1, 2, 3 = wildcard} of C = 3, all four flag combinations, fp32 and fp64, emissions and penalty
    on a quarter grid (every sum exact, ties frequent; every third problem has -inf entries): the recurrence finds the brute-force
    optimum and, among the optimal paths, the one that is lexicographically greatest read from the last frame backwards."""
    C = 3
    targets = [list(t) for U in range(3) for t in itertools.product((1, 2, 3), repeat=U)]
    n_feasible = n_skipped = n_star = 0
    for T in range(1, 6):
        for ti, target in enumerate(targets):
            for flags in range(4):
                kind = (T + ti + flags) % 3
                e = quarter_emissions(T, C, det.seed_of(f"alignstar.tiny.{T}.{ti}.{flags}"), neg_inf=kind == 2)
                penalty = -0.25 * (1 + (T + ti) % 2)
                ee = S.extend(e, penalty, np.float64)
                want_score, want_path = S.brute_force(ee, target, flags)
                for dtype in (np.float32, np.float64):
                    got = S.align(e, target, C, penalty, flags, dtype)
                    if want_path is None:
                        assert not got["feasible"] and got["score"] == -np.inf and (got["states"] == -1).all(), (T, target, flags)
                        assert (got["tok_start"] == -1).all() and (got["tok_end"] == -1).all() and np.isneginf(got["tok_logp"]).all()
                        continue
                    assert got["feasible"] and float(got["score"]) == float(want_score), (T, target, flags)
                    assert np.array_equal(got["states"], want_path), (T, target, flags, got["states"], want_path)
                    assert S.check_path(got["states"], target, flags)
                    for u, c in enumerate(target):
                        idx = np.nonzero(got["states"] == 2 * u + 1)[0]
                        if len(idx) == 0:                       # only an optional end token may be left out
                            assert (u == 0 and flags & 1) or (u == len(target) - 1 and flags & 2), (T, target, flags)
                            assert (got["tok_start"][u], got["tok_end"][u], got["tok_logp"][u]) == (-1, -1, 0)
                            n_skipped += dtype is np.float32
                        else:
                            assert (got["tok_start"][u], got["tok_end"][u]) == (idx[0], idx[-1] + 1)
                            assert float(got["tok_logp"][u]) == float(ee[idx, c].sum())
                if want_path is not None:
                    n_feasible += 1
                    n_star += any(target[s >> 1] == C for s in want_path if s & 1)
    assert n_feasible > 200 and n_skipped > 50 and n_star > 50, (n_feasible, n_skipped, n_star)   # of 260 problems


def test_plain_input_reproduces_the_plain_oracle():
    for T in range(1, 7):
        for ti, target in enumerate(([], [1], [2], [1, 1], [1, 2], [2, 1], [2, 2], [1, 3], [0], [1, 2, 1])):
            for dtype in (np.float32, np.float64):
                e = quarter_emissions(T, 3, det.seed_of(f"alignstar.plain.{T}.{ti}"), neg_inf=(T + ti) % 3 == 0)
                want, got = A.align(e, target, dtype), S.align(e, target, 3, -0.5, 0, dtype)
                if 3 in target:                                 # the plain oracle calls the value C a bad label
                    assert not want["feasible"]
                    continue
                assert want.keys() == got.keys() and want["feasible"] == got["feasible"]
                for k in want:
                    assert np.array_equal(np.asarray(want[k]), np.asarray(got[k])), (T, target, k)
    e = quarter_emissions(0, 3, 1)
    assert S.align(e, [], 3)["score"] == 0 and not S.align(e, [3], 3, flags=3)["feasible"]
    x = np.stack([quarter_emissions(9, 4, det.seed_of(f"alignstar.batch.{b}")) for b in range(3)])
    tg, off, lens = np.array([1, 2, 2, 3], np.int32), np.array([0, 3, 4], np.int32), np.array([3, 1, 0], np.int32)
    want, got = A.align_batch(x, tg, off, [9, 4, 0], lens), S.align_batch(x, tg, off, [9, 4, 0], lens, -0.25, None)
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def test_wildcard_row_and_path_rules():
    e = np.array([[-1.0, -0.25, -3.0], [-np.inf, -np.inf, -np.inf], [-0.5, -2.0, -0.75]], np.float32)
    g = S.star_row(e, -0.25)
    assert g.dtype == np.float32 and g.tolist() == [-0.5, -np.inf, -0.75]
    assert S.extend(e, -0.25).shape == (3, 4)
    # one fp32 add after the max: the rounding of the sum, not of anything wider
    e1 = np.array([[np.float32(-1e-8), -5.0]], np.float32)
    assert S.star_row(e1, math.log(0.5))[0] == np.float32(np.float32(-1e-8) + np.float32(math.log(0.5)))
    assert S.start_states(7, 0) == [0, 1] and S.start_states(7, 1) == [0, 1, 2, 3] and S.start_states(3, 1) == [0, 1, 2]
    assert S.start_states(1, 1) == [0]
    assert S.end_states(7, 0) == [6, 5] and S.end_states(7, 2) == [6, 5, 4, 3] and S.end_states(3, 2) == [2, 1, 0] and S.end_states(1, 2) == [0]
    assert S.check_path([2, 3], [3, 1], 1) and not S.check_path([2, 3], [3, 1], 0) and S.check_path([1, 1], [3, 1], 2)
    assert not S.check_path([1, 1], [3, 1], 1) and S.check_path([0, 0], [1], 2) and S.check_path([1, 3], [3, 1]) \
        and not S.check_path([1, 3], [3, 3])                    # two adjacent wildcards behave like a repeated label
    # the wildcard must take a frame: [*] over one frame is the wildcard (states 0 and 2 are no legal end / start of a single frame) ...
    r = S.align(np.array([[-0.25, -1.0]], np.float32), [2], 2, -0.25, 0)
    assert r["states"].tolist() == [1] and float(r["score"]) == -0.5 and float(r["tok_logp"][0]) == -0.5
    # ... unless it is optional: then the blank's -0.25 wins and the token is left out
    r = S.align(np.array([[-0.25, -1.0]], np.float32), [2], 2, -0.25, S.FREE_END)
    assert r["states"].tolist() == [0] and float(r["score"]) == -0.25 and (r["tok_start"][0], r["tok_end"][0], r["tok_logp"][0]) == (-1, -1, 0)


@pytest.mark.parametrize("without_ends", [False, True])
def test_planted_problem_is_recovered_by_the_oracle(without_ends):
    p, ts, te, states = P.planted(without_ends)
    assert p.shape == ((20 if without_ends else 33), 6) and np.allclose(p.sum(1), 1.0)
    assert S.check_path(states, P.TRANSCRIPT, P.FLAGS) and (without_ends or not S.check_path(states[7:], P.TRANSCRIPT, 0))
    for dtype in (np.float32, np.float64):
        r = S.align(np.log(p.astype(np.float64)), P.TRANSCRIPT, P.C, P.PENALTY, P.FLAGS, dtype)
        assert r["feasible"] and np.array_equal(r["states"], states)
        assert np.array_equal(r["tok_start"], ts) and np.array_equal(r["tok_end"], te)
        if without_ends:
            assert (ts[0], te[0], ts[-1], te[-1]) == (-1, -1, -1, -1) and r["tok_logp"][0] == 0 and r["tok_logp"][-1] == 0
            assert states[0] == 3 and states[-1] == 13          # starts in state 3, ends in state S - 4
        else:
            assert (ts[0], te[0], ts[4], te[4], ts[-1], te[-1]) == (0, 7, 15, 20, 27, 33)
        assert np.isclose(float(r["tok_logp"][4]), 5 * math.log(0.45), rtol=1e-6)
    # without the flags the same transcript has to give its end wildcards a frame each
    r0 = S.align(np.log(p.astype(np.float64)), P.TRANSCRIPT, P.C, P.PENALTY, 0)
    assert r0["feasible"] and r0["tok_start"][0] == 0 and r0["tok_end"][-1] == len(states) and (not without_ends or r0["score"] < r["score"])


# ---- host logic ----------------------------------------------------------------------------------------------------------------
def test_star_and_unknown_mapping():
    from asr_amd.decoders import encode_transcripts
    labels = {c: i for i, c in enumerate("_'abc ")}
    n = len(labels)
    assert encode_transcripts(["ab c", "", "'"], labels) == [[2, 3, 5, 4], [], [1]]                      # as before
    assert encode_transcripts(["a*b", "*", "**a***"], labels, star="*") == [[2, n, 3], [n], [n, 2, n]]
    assert encode_transcripts(["a1b", "12 3", "a*"], labels, unknown="star") == [[2, n, 3], [n, 5, n], [2, n]]
    assert encode_transcripts(["a#1b"], labels, star="#", unknown="star") == [[2, n, 3]]                # a run of both kinds collapses
    assert encode_transcripts([[2, n, n, 3], torch.tensor([n, n])], labels, unknown="star") == [[2, n, 3], [n]]
    assert encode_transcripts([[2, n, n, 3]], labels) == [[2, n, n, 3]]                                 # no option: ids pass as they are
    with pytest.raises(ValueError, match="'1'"):
        encode_transcripts(["a1"], labels, star="*")
    with pytest.raises(ValueError, match="is a label"):
        encode_transcripts(["ab"], labels, star="a")
    with pytest.raises(ValueError, match="single character"):
        encode_transcripts(["ab"], labels, star="**")
    with pytest.raises(ValueError, match="unknown"):
        encode_transcripts(["ab"], labels, unknown="drop")


def test_group_words_and_unaligned_records():
    from asr_amd.decoders import add_seconds, assemble_alignments, group_words
    toks = [("*", 0, 4, -3.0), ("a", 4, 5, -0.5), ("b", 5, 6, -0.25), ("*", 6, 9, -2.0), ("c", 9, 10, -1.0), (" ", 10, 11, -1.0),
            ("a", 11, 12, -0.125)]
    assert group_words(toks, star="*") == [("ab", 4, 6, -0.75), ("c", 9, 10, -1.0), ("a", 11, 12, -0.125)]
    assert group_words(toks) == [("*ab*c", 0, 10, -6.75), ("a", 11, 12, -0.125)]                        # without the option "*" is a character
    assert group_words([("*", 0, 3, -1.0)], star="*") == []
    int_to_char = dict(enumerate("_ab "))
    n = 4
    targets = [[n, 1, n, 2, n], [n, 1], [2]]
    ninf = float("-inf")
    score = np.array([-1.5, ninf, -0.25], np.float32)
    states = np.array([[2, 3, 5, 5, 6, 7], [-1] * 6, [0, 1, -1, -1, -1, -1]], np.int32)
    ts, te = [-1, 1, 2, 5, -1, -1, -1, 1], [-1, 2, 4, 6, -1, -1, -1, 2]
    lp = np.array([0, -0.5, -1.0, -0.75, 0, ninf, ninf, -0.25], np.float32)
    recs = assemble_alignments(score, states, ts, te, lp, targets, [6, 4, 2], int_to_char, 3, star_id=n, star_char="#")
    assert recs[0]["tokens"] == [("a", 1, 2, -0.5), ("#", 2, 4, -1.0), ("b", 5, 6, -0.75)]              # the skipped wildcards are absent
    assert recs[0]["words"] == [("a", 1, 2, -0.5), ("b", 5, 6, -0.75)] and recs[0]["unaligned"] == [(2, 4)]
    assert recs[0]["states"].tolist() == [2, 3, 5, 5, 6, 7]
    assert recs[1] == {"score": ninf, "states": recs[1]["states"], "tokens": [], "words": [], "unaligned": []}
    assert recs[2]["tokens"] == [("b", 1, 2, -0.25)] and recs[2]["unaligned"] == []
    add_seconds(recs, 0.02)
    assert recs[0]["unaligned"] == [(2, 4, 2 * 0.02, 4 * 0.02)] and recs[0]["tokens"][1] == ("#", 2, 4, -1.0, 2 * 0.02, 4 * 0.02)
    assert recs[1]["unaligned"] == [] and recs[0]["words"][1] == ("b", 5, 6, -0.75, 5 * 0.02, 6 * 0.02)
    # no wildcard option: the records of before, key for key
    plain = assemble_alignments(score[[2]], states[[2]], [1], [2], lp[[7]], [[2]], [2], int_to_char, 3)
    assert plain == [{"score": -0.25, "states": plain[0]["states"], "tokens": [("b", 1, 2, -0.25)], "words": [("b", 1, 2, -0.25)]}]
    assert add_seconds(plain, 0.02)[0].keys() == {"score", "states", "tokens", "words"}


class _Recorder:
    """Stands in for asr_amd.ops: records what CTCAligner.align hands to the wildcard entry and returns nothing aligned."""

    def __init__(self):
        self.calls = []

    def rnn_poison_seen(self, dev):
        return False

    def _out(self, x, targets):
        B, T = x.shape[0], x.shape[1]
        n = targets.numel()
        return (torch.full((B,), float("-inf")), torch.full((B, T), -1, dtype=torch.int32), torch.full((n,), -1, dtype=torch.int32),
                torch.full((n,), -1, dtype=torch.int32), torch.full((n,), float("-inf")))

    def ctc_forced_align_star(self, x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log, variant=0, star_penalty=None, flags=None):
        self.calls.append(("star", targets.tolist(), tgt_off.tolist(), tgt_lens.tolist(), max_u, variant, star_penalty, flags.tolist()))
        return self._out(x, targets)

    def ctc_forced_align_star_tiled(self, x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log, tile_frames=0, tile_pairs=0,
                                    star_penalty=None, flags=None):
        self.calls.append(("tiled", targets.tolist(), tgt_off.tolist(), tgt_lens.tolist(), max_u, 3, star_penalty, flags.tolist()))
        return self._out(x, targets)

    def ctc_forced_align(self, *a, **k):
        raise AssertionError("the plain entry must not be used with a wildcard option")

    ctc_forced_align_tiled = ctc_forced_align


def test_aligner_packs_wildcards_and_flags(monkeypatch):
    """The host half of CTCAligner.align with the GPU entry replaced by a recorder (pinned memory and the device are not needed for
    what is checked: the targets, the flags and the entry that is chosen)."""
    import asr_amd
    from asr_amd import decoders
    from asr_amd.decoders import CTCAligner
    rec = _Recorder()
    monkeypatch.setattr(asr_amd, "ops", rec, raising=False)
    monkeypatch.setattr(decoders, "_device", lambda *a: torch.device("cpu"))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **{kk: v for kk, v in k.items() if kk != "pin_memory"}))
    al = CTCAligner({c: i for i, c in enumerate("_ab ")})
    n = 4
    probs = torch.full((3, 9, 4), 0.25)
    al.align(probs, None, ["a*b", "*a", "b1"], star="*", unknown="star", free_start=True)
    kind, tg, off, lens, max_u, variant, pen, flags = rec.calls[-1]
    assert kind == "star" and tg == [n, 1, n, 2] + [n, 1] + [n, 2, n] and off == [0, 4, 6] and lens == [4, 2, 3] and max_u == 4
    assert flags == [1, 1, 1] and pen == math.log(0.5) and variant == 0      # "*a" already begins with a wildcard: none is added
    al.align(probs, None, ["ab", "", "a*"], star="*", free_end=True, free_start=True, variant=3, star_penalty=-2.0)
    kind, tg, off, lens, max_u, variant, pen, flags = rec.calls[-1]
    assert kind == "tiled" and tg == [n, 1, 2, n] + [n] + [n, 1, n] and lens == [4, 1, 3] and flags == [3, 3, 3] and pen == -2.0
    recs = al.align(probs, None, [[1, n, n, 2], [n], []], unknown="star")
    assert rec.calls[-1][1] == [1, n, 2, n] and rec.calls[-1][7] == [0, 0, 0]
    assert all(r["unaligned"] == [] and r["tokens"] == [] for r in recs)
    for bad in (dict(star_penalty=0.5), dict(star_penalty=float("nan")), dict(star_penalty=float("-inf")), dict(star="a"),
                dict(unknown="drop"), dict(variant=4)):
        with pytest.raises(ValueError):
            al.align(probs, None, ["a", "b", "ab"], **dict(dict(free_end=True), **bad))
    with pytest.raises(ValueError, match="classes"):
        al.align(torch.full((1, 9, 5), 0.2), None, ["a"], free_end=True)


def test_model_methods_take_the_new_options():
    import inspect
    from asr_amd import DeepSpeech
    from asr_amd.decoders import CTCAligner
    want = dict(star=None, star_penalty=math.log(0.5), unknown="error", free_start=False, free_end=False)
    for fn in (CTCAligner.align, DeepSpeech.align, DeepSpeech.align_long):
        sig = inspect.signature(fn).parameters
        assert {k: sig[k].default for k in want} == want, fn
    assert list(inspect.signature(CTCAligner.align).parameters)[:6] == ["self", "probs", "sizes", "transcripts", "is_log", "variant"]


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_workspace_sizes_of_the_new_entries():
    from asr_amd import _lib
    lib = _lib.load()
    for B, T, U in ((6, 37, 63), (2, 1200, 1100), (1, 1, 0)):
        assert lib.ds2_ctc_align_star_workspace_bytes(B, T, U) == lib.ds2_ctc_align_workspace_bytes(B, T, U) + 4 * B * T
        for tf, tp in ((8, 64), (0, 0), (64, 128)):
            assert lib.ds2_ctc_align_star_tiled_workspace_bytes(B, T, U, tf, tp) == \
                lib.ds2_ctc_align_tiled_workspace_bytes(B, T, U, tf, tp) + 8 * B + 4 * B * T
    assert lib.ds2_ctc_align_star_workspace_bytes(6, 37, 63) == 4 * 6 * 5 * 64 + 4 * 6 * 37
    assert lib.ds2_ctc_align_star_workspace_bytes(0, 5, 1) == 0 and lib.ds2_ctc_align_star_tiled_workspace_bytes(2, 5, 1, 12, 64) == 0
    assert lib.ds2_ctc_align_star_tiled_workspace_bytes(2, 5, 1, 8, 32) == 0


def test_new_entries_reject_bad_arguments_before_any_launch():
    from asr_amd import _lib
    lib = _lib.load()
    p = 4096                                                           # any non-null address: every call below returns before a launch
    ok = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, targets=p, off=p, in_lens=None, lens=p, max_u=3, variant=0, penalty=-0.5,
              flags=None, score=p, states=p, ts=p, te=p, lp=p, ws=p, wsb=1 << 20, stream=None)
    small = 4 * 2 * 2 * 4 + 4 * 2 * 10 - 1
    for bad in (dict(x=None), dict(B=0), dict(T=0), dict(C=0), dict(max_u=-1), dict(is_log=2), dict(variant=3), dict(variant=-1),
                dict(variant=1, max_u=64), dict(wsb=small), dict(ws=None), dict(score=None), dict(states=None), dict(ts=None),
                dict(targets=None), dict(lens=None), dict(penalty=0.25), dict(penalty=float("nan")), dict(penalty=float("-inf")),
                dict(penalty=float("inf"))):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_align_star_f32(*a.values()) != 0, bad
        assert b"ds2_ctc_align_star_f32" in lib.ds2_last_error()
    okt = dict(ok)
    del okt["variant"]
    okt = dict(list(okt.items())[:12] + [("tf", 8), ("tp", 64)] + list(okt.items())[12:])
    need = lib.ds2_ctc_align_star_tiled_workspace_bytes(2, 10, 3, 8, 64)
    assert need > 0
    for bad in (dict(x=None), dict(B=0), dict(is_log=2), dict(tf=12), dict(tf=-8), dict(tp=32), dict(tp=2048), dict(wsb=need - 1),
                dict(ws=None), dict(penalty=1e-3), dict(penalty=float("nan")), dict(penalty=float("-inf")), dict(targets=None)):
        a = dict(okt, **bad)
        assert lib.ds2_ctc_align_star_tiled_f32(*a.values()) != 0, bad
        assert b"ds2_ctc_align_star_tiled_f32" in lib.ds2_last_error()
    okr = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, in_lens=None, penalty=-0.5, g=p, stream=None)
    for bad in (dict(x=None), dict(g=None), dict(C=0), dict(is_log=-1), dict(penalty=0.5), dict(penalty=float("nan"))):
        assert lib.ds2_ctc_align_star_row_f32(*dict(okr, **bad).values()) != 0, bad
        assert b"ds2_ctc_align_star_row_f32" in lib.ds2_last_error()


def test_ops_wrappers_check_their_arguments():
    from asr_amd import ops
    x = torch.zeros((2, 5, 4))
    i = lambda *v: torch.tensor(v, dtype=torch.int32)
    for fn in (ops.ctc_forced_align_star, ops.ctc_forced_align_star_tiled):
        with pytest.raises(ValueError, match="star_penalty"):
            fn(x, i(1), i(0, 1), None, i(1, 0), 1, True, star_penalty=0.1)
        with pytest.raises(ValueError, match="star_penalty"):
            fn(x, i(1), i(0, 1), None, i(1, 0), 1, True, star_penalty=float("nan"))
        with pytest.raises(ValueError, match="flags"):
            fn(x, i(1), i(0, 1), None, i(1, 0), 1, True, flags=torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="batch"):
            fn(x, i(1), i(0, 1), None, i(1, 0), 1, True, flags=i(0, 0, 0))
        with pytest.raises(ValueError, match="contiguous class dim"):
            fn(x.transpose(1, 2), i(1), i(0, 1), None, i(1, 0), 1, True)
    for fn in (ops.ctc_forced_align, ops.ctc_forced_align_tiled, ops.ctc_forced_align_star, ops.ctc_forced_align_star_tiled):
        with pytest.raises(ValueError, match="batch"):
            fn(x, i(1), i(0, 1, 2), None, i(1, 0), 1, True)
        with pytest.raises(ValueError, match="contiguous class dim"):
            fn(x.transpose(1, 2), i(1), i(0, 1), None, i(1, 0), 1, True)
        with pytest.raises(ValueError, match="tgt_lens must be a contiguous int32"):
            fn(x, i(1), i(0, 1), None, torch.tensor([1, 0]), 1, True)
    with pytest.raises(ValueError, match="star_penalty"):
        ops.ctc_star_row(x, None, True, 1.0)
