"""Host half of the GPU WER / CER scoring (no GPU needed): `pack_scoring` turns string pairs into int32 id sequences, and the edit
distance over those ids must be what Decoder.wer / Decoder.cer compute on the strings, with the reference word / char counts."""
import random

import numpy as np
import pytest

from asr_amd.decoders import Decoder, _edit_distance, pack_scoring

PAIRS = [
    ("", ""),
    ("", "a b"),
    ("a b", ""),
    ("   ", "  "),
    (" ", "abc"),
    (" leading", "leading "),
    ("trailing  ", "  trailing"),
    ("doubled  spaces  here", "doubled spaces here"),
    ("tab\tseparated words", "tab separated\twords"),
    ("ideographic　space", "ideographic space"),
    ("no break space", "no break space"),
    ("the the the cat", "the cat the the"),
    ("a a a a", "b b b"),
    ("こんにちは 世界", "こんばんは 世界"),
    ("emoji \U0001F600\U0001F601 x", "emoji \U0001F601 y"),
    ("lone \ud800 surrogate", "lone \udfff surrogate"),
    ("abc", "abd"),
    ("a b c", "a x c"),
]


def _check(pairs):
    d = Decoder(["_", "a"])
    seq, a_off, a_len, b_off, b_len, ref_w, ref_c = pack_scoring([h for h, _ in pairs], [r for _, r in pairs])
    B = len(pairs)
    assert seq.dtype == np.int32 and a_off.dtype == b_off.dtype == np.int64 and a_len.dtype == b_len.dtype == np.int32
    assert len(a_off) == len(a_len) == len(b_off) == len(b_len) == 2 * B
    assert int((a_off + a_len).max(initial=0)) <= len(seq) and int((b_off + b_len).max(initial=0)) <= len(seq)
    for b, (h, r) in enumerate(pairs):
        side = lambda off, ln, p: seq[off[p]:off[p] + ln[p]].tolist()
        assert _edit_distance(side(a_off, a_len, b), side(b_off, b_len, b)) == d.wer(h, r), (h, r)
        assert _edit_distance(side(a_off, a_len, B + b), side(b_off, b_len, B + b)) == d.cer(h, r), (h, r)
        assert ref_w[b] == len(r.split()) and ref_c[b] == len(r.replace(" ", ""))
        assert a_len[b] == len(h.split()) and a_len[B + b] == len(h.replace(" ", ""))


def test_pack_scoring_matches_wer_and_cer_on_edge_cases():
    _check(PAIRS)


def test_pack_scoring_one_pair_at_a_time():
    for pair in PAIRS:
        _check([pair])


def test_pack_scoring_random_words():
    rng = random.Random(3)
    vocab = ["a", "bb", "c c", "あ", "x\ty", "  ", "z"]
    pairs = [("".join(rng.choice(vocab) + rng.choice([" ", "", "  "]) for _ in range(rng.randrange(0, 12))),
              "".join(rng.choice(vocab) + rng.choice([" ", "", "  "]) for _ in range(rng.randrange(0, 12)))) for _ in range(60)]
    _check(pairs)


def test_pack_scoring_empty_batch_and_mismatch():
    seq, a_off, a_len, b_off, b_len, ref_w, ref_c = pack_scoring([], [])
    assert len(seq) == len(a_off) == len(ref_w) == 0
    with pytest.raises(ValueError):
        pack_scoring(["a"], [])
