"""CPU (-m "not gpu"): the forced-alignment oracle (tests/ctc_align_oracle.py) against brute force, the feasibility edges of the
contract (include/ds2hip.h, ds2_ctc_align_f32), and the host half of asr_amd.decoders.CTCAligner / DeepSpeech.align."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import det  # noqa: E402

import ctc_align_oracle as A  # noqa: E402

TARGETS = ([], [1], [2], [1, 1], [1, 2], [2, 1], [2, 2])


def quarter_emissions(T, C, seed, levels=5, neg_inf=False):
    """Multiples of -0.25 (exact in fp32 and fp64, sums too, so ties are frequent); optionally the lowest level becomes -inf."""
    q = det.randint((T, C), seed, 0, levels)
    e = (-0.25 * q).astype(np.float32)
    if neg_inf:
        e[q == levels - 1] = -np.inf
    return e


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_equals_brute_force_on_every_tiny_problem(dtype):
    """Every (T <= 6, U <= 2, C = 3) target, doubled labels included: the recurrence with its local tie rule finds the brute-force
    optimum and, among the optimal alignments, the one that is lexicographically greatest read from the last frame backwards."""
    n_ties = 0
    for T in range(1, 7):
        for ti, target in enumerate(TARGETS):
            for variant in range(3):
                e = quarter_emissions(T, 3, det.seed_of(f"align.tiny.{T}.{ti}.{variant}"), neg_inf=variant == 2)
                want_score, want_path = A.brute_force(e, target)
                got = A.align(e, target, dtype)
                if want_path is None:
                    assert not got["feasible"] and got["score"] == -np.inf and (got["states"] == -1).all(), (T, target)
                    assert (got["tok_start"] == -1).all() and (got["tok_end"] == -1).all() and np.isneginf(got["tok_logp"]).all()
                    continue
                assert got["feasible"] and float(got["score"]) == float(want_score), (T, target)
                assert np.array_equal(got["states"], want_path), (T, target, got["states"], want_path)
                assert A.check_path(got["states"], target)
                assert float(A.path_score(e, got["states"], target)) == float(want_score)
                # the spans partition the frames of each label state, and their emission sums add up to the labels' share of the score
                for u, c in enumerate(target):
                    idx = np.nonzero(got["states"] == 2 * u + 1)[0]
                    assert (got["tok_start"][u], got["tok_end"][u]) == (idx[0], idx[-1] + 1) and len(idx) == idx[-1] + 1 - idx[0]
                    assert float(got["tok_logp"][u]) == float(e[idx, c].astype(np.float64).sum())
                n_ties += 1
    assert n_ties > 80        # most of the 126 problems are feasible


def test_feasibility_edges():
    """T_b = U + repeats is feasible, one frame fewer is not; bad labels, empty inputs."""
    e = quarter_emissions(12, 4, det.seed_of("align.edges"))
    for target, need in (([1], 1), ([1, 1], 3), ([1, 2, 2, 3], 5), ([2, 2, 2], 5), ([1, 2, 3], 3)):
        r = A.align(e[:need], target)
        assert r["feasible"] and A.check_path(r["states"], target), target
        r = A.align(e[:need - 1], target)
        assert not r["feasible"] and r["score"] == -np.inf and (r["states"] == -1).all() and len(r["states"]) == need - 1, target
    assert not A.align(e, [1, 4])["feasible"] and not A.align(e, [0])["feasible"]          # outside [1, C)
    r = A.align(e[:0], [])
    assert r["feasible"] and r["score"] == 0 and len(r["states"]) == 0
    assert not A.align(e[:0], [1])["feasible"]
    r = A.align(e[:3], [])
    assert r["feasible"] and list(r["states"]) == [0, 0, 0] and float(r["score"]) == float(e[:3, 0].sum())
    assert A.check_path([0, 1, 1, 2], [1]) and A.check_path([1, 3], [1, 2]) and not A.check_path([1, 3], [1, 1])
    assert not A.check_path([2, 2], [1]) and not A.check_path([0, 2], [1]) and not A.check_path([1, 0], [1]) and not A.check_path([0, 0], [1])


def test_library_entry_rejects_bad_arguments_before_any_launch():
    """The C entry point returns nonzero (and sets the error text) for bad arguments; the workspace query is a pure host function."""
    from asr_amd import _lib
    lib = _lib.load()
    assert lib.ds2_ctc_align_workspace_bytes(6, 37, 63) == 4 * 6 * 5 * 64
    assert lib.ds2_ctc_align_workspace_bytes(2, 1200, 1100) == 4 * 2 * 150 * 1101
    p = 4096                                                           # any non-null address: every call below returns before a launch
    ok = dict(x=p, ld_b=100, ld_t=10, B=2, T=10, C=10, is_log=1, targets=p, off=p, in_lens=None, lens=p, max_u=3, variant=0, score=p,
              states=p, ts=p, te=p, lp=p, ws=p, wsb=1 << 20, stream=None)
    for bad in (dict(x=None), dict(B=0), dict(T=0), dict(C=0), dict(max_u=-1), dict(is_log=2), dict(variant=3), dict(variant=-1),
                dict(variant=1, max_u=64), dict(wsb=4 * 2 * 2 * 4 - 1), dict(ws=None), dict(score=None), dict(states=None), dict(ts=None),
                dict(targets=None), dict(lens=None)):
        a = dict(ok, **bad)
        assert lib.ds2_ctc_align_f32(*a.values()) != 0, bad
        assert b"ds2_ctc_align_f32" in lib.ds2_last_error()


def test_transcript_mapping_and_word_grouping():
    from asr_amd.decoders import CTCAligner, encode_transcripts, group_words
    labels = {c: i for i, c in enumerate("_'abc ")}
    assert encode_transcripts(["ab c", "", "'"], labels) == [[2, 3, 5, 4], [], [1]]
    assert encode_transcripts([[2, 3], torch.tensor([4]), np.array([5, 5])], labels) == [[2, 3], [4], [5, 5]]
    assert encode_transcripts(["ba"], "_ab") == [[2, 1]]
    with pytest.raises(ValueError, match="'z'"):
        encode_transcripts(["ab", "az"], labels)
    with pytest.raises(ValueError):
        CTCAligner(labels, blank_index=1)
    assert CTCAligner(labels).space_index == 5 and CTCAligner(list("_ab c")).space_index == 3
    toks = [(" ", 0, 1, -1.0), ("a", 1, 3, -0.5), ("b", 4, 5, -0.25), (" ", 5, 6, -1.0), (" ", 7, 8, -1.0), ("c", 9, 12, -2.0),
            (" ", 12, 13, -1.0)]
    assert group_words(toks) == [("ab", 1, 5, -0.75), ("c", 9, 12, -2.0)]
    assert group_words([]) == [] and group_words([(" ", 0, 1, 0.0)]) == []
    big = [("a", 0, 1, 1e8), ("b", 1, 2, 1.0), ("c", 2, 3, -1e8)]                         # summed in fp64
    assert group_words(big)[0][3] == 1.0


def test_record_assembly_and_seconds_from_raw_arrays():
    from asr_amd.decoders import add_seconds, assemble_alignments
    int_to_char = dict(enumerate("_ab "))
    targets = [[1, 3, 2], [2], []]
    ninf = float("-inf")
    score = np.array([-1.5, ninf, -0.25], np.float32)
    states = np.array([[0, 1, 1, 3, 4, 5], [-1] * 6, [0, 0, -1, -1, -1, -1]], np.int32)
    recs = assemble_alignments(score, states, [1, 3, 5, -1], [3, 4, 6, -1], np.array([-0.5, -0.25, -0.75, ninf], np.float32), targets,
                               [6, 4, 2], int_to_char, 3)
    assert recs[0]["score"] == -1.5 and recs[0]["states"].tolist() == [0, 1, 1, 3, 4, 5] and recs[0]["states"].dtype == torch.int32
    assert recs[0]["tokens"] == [("a", 1, 3, -0.5), (" ", 3, 4, -0.25), ("b", 5, 6, -0.75)]
    assert recs[0]["words"] == [("a", 1, 3, -0.5), ("b", 5, 6, -0.75)]
    assert recs[1] == {"score": ninf, "states": recs[1]["states"], "tokens": [], "words": []} and recs[1]["states"].numel() == 0
    assert recs[2]["score"] == -0.25 and recs[2]["states"].tolist() == [0, 0] and recs[2]["tokens"] == [] and recs[2]["words"] == []
    add_seconds(recs, 2 * 0.01)
    assert recs[0]["tokens"][0] == ("a", 1, 3, -0.5, 1 * 0.02, 3 * 0.02) and recs[0]["words"][1] == ("b", 5, 6, -0.75, 5 * 0.02, 6 * 0.02)
    assert recs[1]["tokens"] == [] and recs[2]["words"] == []


def test_aligner_checks_its_arguments_and_has_no_cpu_path():
    from asr_amd._lib import DS2LibraryError
    from asr_amd.decoders import CTCAligner
    al = CTCAligner({c: i for i, c in enumerate("_ab ")})
    probs = torch.full((2, 5, 4), 0.25)
    with pytest.raises(ValueError, match="1 transcripts for a batch of 2"):
        al.align(probs, None, ["ab"])
    with pytest.raises(ValueError, match="'x'"):
        al.align(probs, None, ["ab", "x"])
    if not torch.cuda.is_available():
        with pytest.raises(DS2LibraryError):                # align() itself is GPU-only: no CPU path
            al.align(probs, [5, 4], ["ab", "b"])


def test_model_align_is_part_of_the_api():
    from asr_amd import DeepSpeech
    assert callable(getattr(DeepSpeech, "align"))
