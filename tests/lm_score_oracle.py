"""The LM term of a finished label sequence, `ds2_lm_score_seqs` (include/ds2hip.h), restated in plain Python from the contract: the
split at the space label, the word lookup BY STRING, the contexts, the three outputs.  Token scores come from NaiveLM (the dict-based
ARPA reader of tests/ctc_beam_lm_oracle.py) in fp64.  Also returned: the sum of |file value| over every value the scores used, for the
derived bound  |lm_sum - fp64| <= (order + n_tok) * 2^-23 * sum|values|  (each score sums at most `order` file values rounded to fp32,
and the sequence adds n_tok terms in fp32).  Test-only; shared by the CPU and the GPU tests, which also take their sequences here."""
from __future__ import annotations

import math

import numpy as np

from ctc_beam_lm_oracle import OOV, SPECIAL, NaiveLM   # noqa: F401

UNKNOWN = "\x00oov"   # stands for any token outside the vocabulary in a context


def tokens_of(lm, chars, blank, space, labels):
    """the tokens of a label sequence as vocabulary strings (UNKNOWN for an out-of-vocabulary one), in order"""
    if lm.char_mode:
        return [chars[x] if chars[x] in lm.vocab and x != blank else UNKNOWN for x in labels]
    ok = {c for i, c in enumerate(chars) if i not in (blank, space)}
    dictionary = {w for w in lm.vocab if w not in SPECIAL and all(ch in ok for ch in w)}
    runs, cur = [], ""
    for x in list(labels) + [space]:          # the last run is scored whether or not a space follows it
        if x == space:
            if cur:                           # empty runs (a leading, doubled or trailing space) score nothing
                runs.append(cur)
            cur = ""
        else:
            cur += chars[x]
    return [w if w in dictionary else UNKNOWN for w in runs]


def used_values(lm, h, w):
    """|file values| that the backoff rule reads for lm(w | h): the backoffs of the contexts it leaves and the listed probability"""
    tot = 0.0
    while (*h, w) not in lm.table:
        tot += abs(lm.table.get(h, (0.0, 0.0))[1])
        h = h[1:]
    return tot + abs(lm.table[(*h, w)][0])


def score_sequence(lm, chars, blank, space, labels, max_len=None):
    """-> dict(lm_sum fp64, n_tok, n_oov, abs_sum, tokens, scores) for one sequence; a refused one (longer than max_len, a label outside
    the classes, the blank inside) gives lm_sum NaN, n_tok = n_oov = -1"""
    labels = [int(x) for x in labels]
    if (max_len is not None and len(labels) > max_len) or any(x < 0 or x >= len(chars) or x == blank for x in labels):
        return dict(lm_sum=math.nan, n_tok=-1, n_oov=-1, abs_sum=0.0, tokens=[], scores=[])
    toks = tokens_of(lm, chars, blank, space, labels)
    m = lm.order - 1
    total, abs_sum, n_oov, scores = 0.0, 0.0, 0, []
    for i, w in enumerate(toks):
        s = lm.score(toks[:i], w)             # the previous order-1 tokens, <s>-padded; OOV when any of them or w is unknown
        scores.append(s)
        if s == OOV:
            n_oov += 1
        else:
            total += s
            h = tuple((["<s>"] * m + toks[:i])[len(toks[:i]):]) if m else ()
            abs_sum += used_values(lm, h, w)
    return dict(lm_sum=total, n_tok=len(toks), n_oov=n_oov, abs_sum=abs_sum, tokens=toks, scores=scores)


def bound(lm, res):
    return (lm.order + res["n_tok"]) * 2.0 ** -23 * res["abs_sum"]


# ---- the sequences both test files score ----

LABELS = "_ABCDE "            # index 0 is the blank, 6 the space
BLANK, SPACE = 0, 6
LONG_WORD = "ABCDE" * 14      # a dictionary word of 70 labels
WORDS = ["A", "AB", "BAD", "CAB", "DE", "EDA", "Z", LONG_WORD]   # "Z" has no label: in the vocabulary, not in the dictionary
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)


def spell(text):
    return [LABELS.index(ch) for ch in text]


def sequences(mode, order, seed=0):
    """[(name, labels)]: every length of LENGTHS, as random labels and (word mode) as dictionary words joined by single spaces and cut
    to the length; a leading, a doubled and a trailing space; an OOV word followed by `order` in-vocabulary words; the 70-label
    word; more than 64 words"""
    rng = np.random.default_rng(1000 * order + seed + (0 if mode == "word" else 7))
    dic = [w for w in WORDS if w != "Z"]
    out = []
    for n in LENGTHS:
        out.append((f"random{n}", [int(x) for x in rng.integers(1, 7, size=n)]))
        text = ""
        while len(text) < n:
            text += dic[int(rng.integers(0, len(dic) - 1))] + " "
        out.append((f"words{n}", spell(text[:n])))
        out.append((f"letters{n}", [int(x) for x in rng.integers(1, 6, size=n)]))   # no space at all
    out += [("leading", spell(" AB CAB")), ("doubled", spell("AB  CAB DE")), ("trailing", spell("AB CAB ")), ("plain", spell("AB CAB")),
            ("spaces", spell("   ")), ("one space", spell(" ")),
            ("oov then in-vocabulary", spell("AB EEE " + " ".join(dic[k % 6] for k in range(order)) + " DE AB")),
            ("not in the dictionary", spell("CAB DDD AB")),
            ("long word", spell("AB " + LONG_WORD + " DE")), ("long word alone", spell(LONG_WORD)),
            ("long word cut", spell(LONG_WORD[:69] + " A")),
            ("many words", spell(" ".join(dic[int(k)] for k in rng.integers(0, 6, size=150)))),
            ("many short words", spell(" ".join("A" for _ in range(70))))]
    return out
