"""BeamCTCDecoder's hotwords without a GPU: the restatement tests/ctc_beam_hot_oracle.py against its own naive scan and brute force,
the library's packed automaton and host stepping function (the device's code) against that restatement, node by node and label by
label, and the errors of decoders.hotwords.Hotwords."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_hot_oracle as HO   # noqa: E402
import ctc_beam_lm_oracle as LO   # noqa: E402
import ctc_beam_oracle as O   # noqa: E402

LABELS = "_ABCDE "   # index 0 is the blank, 6 the space
FIXED_SETS = [
    (["BAD", "DEAD", "ACE", "ABC", "BCD", "E A", "CC"], [1.0, 0.5, 2.0, 1.0, 1.5, 0.75, 1.25]),
    (["ABC", "ABD", "AC"], [0.3, 1.7, 0.9]),            # shared prefixes with different weights
    (["ABC", "BCD"], [1.0, 2.0]),                        # an overlapping pair
    (["ABCD", "BCD", "CE"], [0.7, 1.1, 0.4]),            # a phrase that is a suffix of another; a failure link into a phrase end
    (["ABCDE", "BCD", "C"], [1.0, 1.0, 3.0]),            # infixes
    (["A"], [0.0]),
]


def _ids(p):
    return tuple(LABELS.index(c) for c in p)


def _random_set(rng, C=6, n_max=12, len_max=7):
    """random prefix-free phrases over labels 1..C-1 with fp32-exact weights"""
    out = []
    for _ in range(int(rng.integers(1, n_max + 1))):
        p = tuple(int(x) for x in rng.integers(1, C, size=int(rng.integers(1, len_max + 1))))
        if all(p[:len(q)] != q and q[:len(p)] != p for q in out):
            out.append(p)
    return out, [float(rng.integers(0, 33)) / 8.0 for _ in out]


def test_invariant_labeling_equals_credit():
    """the terms of a complete labeling sum to the len * w of the phrases the naive scan credits"""
    rng = np.random.default_rng(0)
    n = 0
    sets = [([_ids(p) for p in ps], ws) for ps, ws in FIXED_SETS] + [_random_set(rng) for _ in range(30)]
    for phrases, weights in sets:
        f = HO.HotFusion(phrases, weights)
        for _ in range(40):
            lab = tuple(int(x) for x in rng.integers(1, 7, size=int(rng.integers(0, 25))))
            want = f.credit(lab)
            assert abs(f.labeling(lab) - want) <= 1e-6 * max(1.0, want), (phrases, lab)
            n += 1
    assert n >= 1200
    f = HO.HotFusion([_ids("CAT".replace("T", "B")), _ids("ABCD"), _ids("BC")], [1.0, 1.0, 1.0])   # "CAB", "ABCD", "BC"
    assert f.credit(_ids("CABA")) == 3.0          # no word boundary: the phrase inside a longer word is credited
    assert f.credit(_ids("ABCE")) == 0.0          # "BC" hidden inside the partial match "ABC" is not credited
    assert f.credit(_ids("CABC")) == 3.0          # after the credit of "CAB" matching restarts at the root: no "BC" from its B
    assert f.credit(_ids("BCBC")) == 4.0


def _node_ids(hot, fusion):
    """oracle node (a tuple of labels) -> the node id of the packed automaton, by walking its edges"""
    out = {}
    for node in fusion.phi:
        n = 0
        for c in node:
            n = hot.edges[(n, c)]
        out[node] = n
    return out


def _check_packed(phrases, weights, C=7):
    from asr_amd.decoders.hotwords import Hotwords
    hot = Hotwords([(list(p), w) for p, w in zip(phrases, weights)], LABELS[:C], 0)
    f = HO.HotFusion(phrases, weights)
    ids = _node_ids(hot, f)
    assert len(ids) == hot.n_nodes == len(set(ids.values()))
    n = 0
    for node, nid in ids.items():
        assert np.float32(hot.phi[nid]).view(np.int32) == np.float32(f.phi[node]).view(np.int32), node
        if node in f.ends:
            assert hot.terminal[nid] and f.phi[node] == float(np.float32(len(node) * f.ends[node]))
            continue   # a phrase end is never a state
        for c in range(1, C):
            new, reached, _ = f.step(node, c)
            nxt, term = hot.step(nid, c)
            want = np.float32(f.phi[reached]) - np.float32(f.phi[node])
            assert nxt == ids[new], (node, c, nxt, new)
            assert np.float32(term).view(np.int32) == np.float32(want).view(np.int32), (node, c, term, want)
            n += 1
    return n


def test_packed_automaton_steps_like_the_oracle():
    rng = np.random.default_rng(1)
    n = sum(_check_packed([_ids(p) for p in ps], ws) for ps, ws in FIXED_SETS)
    for _ in range(25):
        phrases, _ = _random_set(rng, C=6)
        n += _check_packed(phrases, [float(w) for w in rng.uniform(0, 3, size=len(phrases))])
    assert n > 2000


def test_thousand_phrases_of_sixty_four_labels_pack_and_walk():
    """the stated limits: 1000 phrases of 64 labels over 29 classes; a walk from the deepest nodes ends"""
    from asr_amd.decoders.hotwords import Hotwords
    rng = np.random.default_rng(2)
    phrases = {tuple(int(x) for x in rng.integers(1, 29, size=64)) for _ in range(1000)}
    hot = Hotwords([list(p) for p in phrases], [chr(65 + i) for i in range(29)], 0, 0.5)
    assert hot.n_nodes > 60000 and max(hot.depth) == 64
    f = HO.HotFusion([p for p in list(phrases)[:3]], [0.5] * 3)
    p = list(phrases)[0]
    node = 0
    for c in p[:-1]:
        node, term = hot.step(node, c)
        assert term == 0.5
    assert hot.step(node, p[-1]) == (0, 0.5)
    assert f.credit(p) == 32.0
    with pytest.raises(ValueError, match="64"):
        Hotwords([list(range(1, 29)) * 3], [chr(65 + i) for i in range(29)], 0)


def test_packer_refuses_a_walk_that_could_not_end():
    import ctypes
    from asr_amd import _lib
    lib = _lib.load()
    en, el, ec = (np.array(x, np.int32) for x in ([0, 1], [1, 2], [1, 2]))   # root -1-> 1 -2-> 2
    phi, term = np.array([0, 1, 2], np.float32), np.array([0, 0, 1], np.int32)
    nbytes = lib.ds2_ctc_hot_packed_bytes(3, 2)
    assert nbytes > 0 and lib.ds2_ctc_hot_packed_bytes(3, 3) == 0 and lib.ds2_ctc_hot_packed_bytes((1 << 20) + 1, 1 << 20) == 0
    buf = np.zeros(nbytes, np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def pack(fail, phi=phi):
        fail = np.array(fail, np.int32)
        return lib.ds2_ctc_hot_pack(3, 2, ptr(en), ptr(el), ptr(ec), ptr(fail), ptr(phi), ptr(term), 7, ptr(buf), nbytes)

    assert pack([0, 0, 0]) == 0
    nxt, t = ctypes.c_int(), ctypes.c_float()
    assert lib.ds2_ctc_hot_step(ptr(buf), 1, 2, ctypes.byref(nxt), ctypes.byref(t)) == 0 and (nxt.value, t.value) == (0, 1.0)
    assert lib.ds2_ctc_hot_step(ptr(buf), 3, 2, ctypes.byref(nxt), ctypes.byref(t)) != 0      # node out of range
    for bad in ([0, 1, 0], [0, 0, 2], [0, 2, 0], [1, 0, 0], [0, 0, 7]):   # self link, link to a deeper node, the root's link astray
        assert pack(bad) != 0, bad
        assert b"failure link" in lib.ds2_last_error()
        assert lib.ds2_ctc_hot_step(ptr(buf), 0, 1, ctypes.byref(nxt), ctypes.byref(t)) != 0   # a refused pack leaves no blob
    assert pack([0, 0, 0], np.array([0, -1, 2], np.float32)) != 0
    assert pack([0, 0, 0], np.array([0, np.inf, 2], np.float32)) != 0


def test_hotword_errors():
    from asr_amd.decoders.hotwords import Hotwords
    with pytest.raises(ValueError, match="equal after encoding"):
        Hotwords(["BAD", [2, 1, 4]], LABELS)
    with pytest.raises(ValueError, match=r"'BA'.*proper prefix.*'BAD'"):
        Hotwords(["BAD", "ACE", "BA"], LABELS)
    with pytest.raises(ValueError, match="'Z'"):
        Hotwords(["BAZ"], LABELS)
    with pytest.raises(ValueError, match="blank"):
        Hotwords(["B_D"], LABELS)
    with pytest.raises(ValueError, match="blank"):
        Hotwords([[2, 0]], LABELS)
    with pytest.raises(ValueError, match="blank"):
        Hotwords(["BAD "], " ABCDE_"[::-1], blank_index=6)     # labels "_EDCBA ": the space sits at the blank index 6
    for w in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="weight"):
            Hotwords([("BAD", w)], LABELS)
        with pytest.raises(ValueError, match="weight"):
            Hotwords(["BAD"], LABELS, weight=w)
    with pytest.raises(ValueError, match="empty"):
        Hotwords(["BAD", ""], LABELS)
    with pytest.raises(ValueError, match="empty"):
        Hotwords([[]], LABELS)
    with pytest.raises(ValueError, match="at least one"):
        Hotwords([], LABELS)
    with pytest.raises(ValueError, match="outside"):
        Hotwords([[1, 7]], LABELS)
    Hotwords(["ABCD", "BC", "CD"], LABELS)                       # an infix and a suffix of another phrase are fine


def test_encoding_weights_and_decoder_arguments():
    from asr_amd.decoders import BeamCTCDecoder
    from asr_amd.decoders.hotwords import Hotwords
    h = Hotwords(["E A", ("BAD", 2.0), [1, 3, 5]], LABELS, 0, 0.75)
    assert h.phrases == [(5, 6, 1), (2, 1, 4), (1, 3, 5)] and h.weights == [0.75, 2.0, 0.75]
    assert h.space == 6 and h.C == 7 and h.packed.nbytes > 0
    labels = {c: i for i, c in enumerate("_ABCDE|")}              # the space label spelt otherwise, as in the reference's label files
    assert Hotwords(["E A"], labels, 0, space_index=6).phrases == [(5, 6, 1)]
    with pytest.raises(ValueError, match="' '"):
        Hotwords(["E A"], labels, 0)
    d = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, beam_width=10, hotwords=["E A", ("BAD", 2.0)], hotword_weight=0.5)
    assert d.hotwords.phrases == [(5, 6, 1), (2, 1, 4)] and d.hotwords.weights == [0.5, 2.0]
    d.set_hotwords(["ACE"], 1.5)
    assert d.hotwords.phrases == [(1, 3, 5)] and d.hotwords.weights == [1.5] and d.hotword_weight == 1.5
    d.set_hotwords(None)
    assert d.hotwords is None and BeamCTCDecoder(LABELS).hotwords is None
    d.set_hotwords(h)
    assert d.hotwords is h


@pytest.mark.parametrize("T,C,seed", [(3, 4, 0), (4, 4, 1), (3, 5, 2), (5, 3, 3)])
def test_oracle_matches_brute_force(T, C, seed):
    """with an unbounded beam and no cutoff the restated search's best beam is the best labeling under the hotword terms"""
    chars = "_ABCDE"[:C - 1] + " "
    names = ["AA", "A "] if C == 3 else ["AB", "BA", "B "]
    f = HO.HotFusion([[chars.index(c) for c in p] for p in names], [1.0, 0.5, 1.5][:len(names)])
    probs = np.random.default_rng(seed).dirichlet(np.ones(C) * 0.7, size=T)
    want = HO.brute_force_best(probs, f, 0)
    res = HO.beam_search(probs, f, None, 0, 10 ** 6, C, 1.0)
    pr, _, s = res["beams"][0]
    assert pr == want[0] and abs(s - want[1]) < 1e-9
    truth = O.brute_force_label_logprobs(probs, 0)
    for pr, _, s in res["beams"]:
        assert abs(s - truth[pr] - f.credit(pr)) < 1e-6
    z = HO.HotFusion([[1, 2]], [0.0])            # zero weight: the plain search
    a = HO.beam_search(probs, z, None, 0, 4, C, 1.0)["beams"]
    b = O.beam_search(probs, None, 0, 4, C, 1.0)["beams"]
    assert [x[0] for x in a] == [x[0] for x in b] and all(abs(x[2] - y[2]) < 1e-12 for x, y in zip(a, b))
    assert LO.NEG == HO.NEG
