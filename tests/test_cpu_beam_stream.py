"""Streaming beam search without a GPU: the exported entries and their size queries, BeamStream's host logic (every refusal that needs
no device runs before any device call), and the stable-prefix oracle of tests/ctc_beam_stream_oracle.py against a brute force."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_stream_oracle as SO   # noqa: E402

LABELS = "_ABCDE "


def test_stream_symbols_are_exported():
    from asr_amd import _lib, ops
    from asr_amd.decoders import BeamCTCDecoder, BeamStream
    lib = _lib.load()
    for name in ("ds2_ctc_beam_stream_state_bytes", "ds2_ctc_beam_stream_nodes_bytes", "ds2_ctc_beam_stream_feed_f32"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert callable(ops.ctc_beam_stream_feed) and callable(BeamCTCDecoder.open_stream) and BeamStream.feed and BeamStream.finish


def test_size_queries_are_monotone_and_refuse_bad_sizes():
    from asr_amd import _lib
    lib = _lib.load()
    st, nd = lib.ds2_ctc_beam_stream_state_bytes, lib.ds2_ctc_beam_stream_nodes_bytes
    assert nd(3, 10, 7) == 12 * 3 * 10 * 7 and nd(1, 1, 1) == 12
    for bad in ((0, 10, 7), (3, 0, 7), (3, 10, 0), (-1, 10, 7)):
        assert nd(*bad) == 0
    for bad in ((0, 4, 0, 0), (3, 0, 0, 0), (-2, 4, 1, 1), (3, lib.ds2_ctc_beam_max_width() + 1, 0, 0)):
        assert st(*bad) == 0
    for lm, hot in itertools.product((0, 1), (0, 1)):
        for K in (1, 4, 100, 256):
            assert 0 < st(1, K, lm, hot) < st(2, K, lm, hot) == 2 * st(1, K, lm, hot)       # B
            if K < 256:
                assert st(3, K, lm, hot) < st(3, K + 1, lm, hot)                           # beam_width
    for K in (1, 100, 256):
        assert st(3, K, 0, 0) < st(3, K, 1, 0) <= st(3, K, 1, 1) and st(3, K, 0, 0) < st(3, K, 0, 1) <= st(3, K, 1, 1)
        assert st(3, K, 1, 0) < st(3, K, 1, 1)
        assert st(1, K, 0, 0) >= 64 + 40 * K          # a header and the eight per-beam fields
    assert nd(2, 11, 7) > nd(2, 10, 7) and nd(3, 10, 7) > nd(2, 10, 7) and nd(2, 10, 8) > nd(2, 10, 7)


def test_growth_plan_doubles_until_the_frames_fit():
    from asr_amd.decoders import stream_capacity
    assert stream_capacity(1, 1) == 1 and stream_capacity(1, 2) == 2 and stream_capacity(1, 3) == 4 and stream_capacity(1, 5) == 8
    assert stream_capacity(256, 10) == 256 and stream_capacity(256, 256) == 256 and stream_capacity(256, 257) == 512
    assert stream_capacity(256, 30000) == 32768 and stream_capacity(0, 3) == 4 and stream_capacity(6, 20) == 24
    cap, seen = 1, []
    for need in range(1, 40):            # one frame per feed from a capacity of one: it grows log2 times, never shrinks
        new = stream_capacity(cap, need)
        assert new >= need and new >= cap
        if new != cap:
            seen.append(new)
        cap = new
    assert seen == [2, 4, 8, 16, 32, 64]


def _decoder(**kw):
    from asr_amd.decoders import BeamCTCDecoder
    return BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, **kw)


def test_open_stream_refusals_and_snapshot():
    d = _decoder(beam_width=4, cutoff_top_n=5, cutoff_prob=0.99)
    for bad in (5, 0, -1, 1.5):
        with pytest.raises(ValueError, match="nbest"):
            d.open_stream(nbest=bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="batch"):
            d.open_stream(batch=bad)
    with pytest.raises(ValueError, match="capacity"):
        d.open_stream(capacity=0)
    s = d.open_stream(batch=3, nbest=4)
    assert (s.batch, s.nbest, s.closed, s.frames, s.C) == (3, 4, False, [0, 0, 0], None)
    d.beam_width, d.cutoff_top_n, d.cutoff_prob, d.alpha, d.beta = 9, 2, 0.5, 3.0, 4.0       # later changes do not reach the stream
    d.set_hotwords(["BAD"])
    assert s.search == dict(blank=0, beam_width=4, cutoff_top_n=5, cutoff_prob=0.99, lm=None, alpha=0, beta=0, hotwords=None)
    assert d.open_stream().search["hotwords"] is d.hotwords and d.open_stream().search["beam_width"] == 9


def test_feed_refusals_need_no_device():
    d = _decoder(beam_width=4)
    s = d.open_stream(batch=2)
    p = torch.full((2, 5, 7), 1.0 / 7)
    with pytest.raises(ValueError, match=r"probs must be \(2, T, C\)"):
        s.check_feed(torch.full((3, 5, 7), 1.0 / 7))                      # the wrong batch
    with pytest.raises(ValueError, match=r"probs must be \(2, T, C\)"):
        s.check_feed(p[0])                                                # (T, C) is for batch 1 only
    with pytest.raises(ValueError, match="at least one frame"):
        s.check_feed(p[:, :0])
    for bad in ([6, 0], [0, -1], [1], [1, 2, 3], [1.0, 2.0]):
        with pytest.raises(ValueError, match="sizes"):
            s.check_feed(p, bad)
    assert s.C is None                                                    # a refused chunk fixes nothing
    x, n = s.check_feed(p, [5, 0])
    assert x.shape == (2, 5, 7) and n == [5, 0] and s.C == 7
    assert s.check_feed(p, torch.tensor([0, 0]))[1] == [0, 0] and s.check_feed(p)[1] == [5, 5]
    with pytest.raises(ValueError, match="7 classes, this chunk has 8"):
        s.check_feed(torch.full((2, 5, 8), 0.125))                        # a changed C
    one = d.open_stream()
    assert one.check_feed(p[0])[0].shape == (1, 5, 7)
    s.closed = True                                                       # what finish() leaves
    with pytest.raises(ValueError, match="closed"):
        s.check_feed(p)
    with pytest.raises(ValueError, match="closed"):
        s.feed(p)
    with pytest.raises(ValueError, match="closed"):
        s.finish()


def test_stream_long_needs_a_beam_decoder():
    from asr_amd.decoders import GreedyDecoder
    from asr_amd.modules.deepspeech import DeepSpeech
    assert callable(DeepSpeech.stream_long)

    class Holder:
        decoder = None
    with pytest.raises(TypeError, match="BeamCTCDecoder"):
        DeepSpeech.stream_long(Holder(), torch.zeros((8, 30)))
    with pytest.raises(TypeError, match="BeamCTCDecoder"):
        DeepSpeech.stream_long(Holder(), torch.zeros((8, 30)), decoder=GreedyDecoder(LABELS))


def _brute_stable(beams):
    """the largest n such that the first n (label, offset) pairs exist in every beam and agree, by trying every n"""
    best = 0
    for n in range(0, 1 + min((len(b[0]) for b in beams), default=0)):
        if all(b[0][:n] == beams[0][0][:n] and b[1][:n] == beams[0][1][:n] for b in beams):
            best = n
    return best


HAND_BEAMS = [
    ([], 0),
    ([((), (), 0.0)], 0),
    ([((1, 2, 3), (0, 4, 7), -1.0)], 3),
    ([((1, 2, 3), (0, 4, 7), -1.0), ((1, 2), (0, 4), -2.0), ((1, 2, 4), (0, 4, 9), -3.0)], 2),
    ([((1, 2, 3), (0, 4, 7), -1.0), ((1, 2, 3), (0, 5, 7), -2.0)], 1),            # the same labels, another offset
    ([((1, 2), (3, 4), -1.0), ((1, 2), (2, 4), -1.5)], 0),                        # the same labels, the first offset differs
    ([((1, 2), (0, 4), -1.0), ((), (), -5.0)], 0),                                # the empty prefix is alive
    ([((2, 1), (0, 1), -1.0), ((1, 2), (0, 1), -1.0)], 0),
    ([((5, 5, 5), (1, 3, 5), -1.0), ((5, 5, 5, 5), (1, 3, 5, 7), -1.2), ((5, 5, 5, 1), (1, 3, 5, 6), -2.0)], 3),
    ([((1, 2, 3), (0, 4, 7), -1.0), ((1, 2, 3), (0, 4, 8), -1.0), ((1, 2, 3, 4), (0, 4, 7, 9), -1.0)], 2),
]


@pytest.mark.parametrize("beams,want", HAND_BEAMS, ids=[str(i) for i in range(len(HAND_BEAMS))])
def test_stable_prefix_on_hand_written_beams(beams, want):
    assert SO.stable_prefix(beams) == want == _brute_stable(beams)
    assert SO.stable_prefix(list(reversed(beams))) == want


def test_stable_prefix_of_the_oracles_beams_and_cuts():
    import ctc_beam_oracle as O
    g = torch.Generator().manual_seed(5)
    z = torch.randn((9, 7), generator=g) * 16.0
    z[:, 0] += 2.0
    probs = torch.softmax(z, -1).double().numpy()
    cuts = list(range(0, 10))
    res = SO.search_at_cuts(probs, cuts, None, 0, 4, 40, 1.0)
    assert [r["beams"] for r in res] == [O.beam_search(probs, t, 0, 4, 40, 1.0)["beams"] for t in cuts]
    st = [SO.stable_prefix(r["beams"]) for r in res]
    assert st == [_brute_stable(r["beams"]) for r in res] and st[0] == 0
    for i, r in enumerate(res):          # what is stable at a cut starts every beam of every later cut
        head = list(zip(r["beams"][0][0], r["beams"][0][1]))[:st[i]]
        for later in res[i:]:
            for b in later["beams"]:
                assert list(zip(b[0], b[1]))[:st[i]] == head
