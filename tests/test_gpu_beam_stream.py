"""-m gpu: the streaming beam search (ds2_ctc_beam_stream_feed_f32, csrc/ctc_beam_stream.h; BeamCTCDecoder.open_stream,
DeepSpeech.stream_long).  The yardstick is the one-call decode, which the existing tests hold to the fp64 oracles: after ANY cuts of
the frames into feeds, a read-out must have the BITS of ops.ctc_beam_decode on the frames consumed so far, in every arm (plain,
character LM, word LM, hotwords, hotwords + word LM).  One grid point is also compared with the oracles directly, by the rule of
test_gpu_ctc_beam.py (exact where every decision of the oracle cleared 1e-4, at least 90 % of the utterances compared exactly).
The stable prefix is checked against a host computation on the read-out, for monotonicity, against every later result, and against
tests/ctc_beam_stream_oracle.py."""
import math
import os
import tempfile
from types import SimpleNamespace

import pytest
import torch

import ctc_beam_hot_oracle as HO
import ctc_beam_lm_oracle as LO
import ctc_beam_stream_oracle as SO
from lm_fixtures import random_arpa

pytestmark = pytest.mark.gpu
WORDS = ["A", "AB", "BAD", "CAB", "DE", "EDA", "BEAD", "DEAD", "ACE", "Z"]
PHRASES, WEIGHTS = ["BAD", "DEAD", "ACE", "ABC", "BCD", "E A", "CC"], [1.0, 0.5, 2.0, 1.0, 1.5, 0.75, 1.25]
CHARS = {2: "_A", 7: "_ABCDE ", 29: "_ABCDEFGHIJKLMNOPQRSTUVWXYZ' "}
ALPHA, BETA = 0.8, 1.0
ARMS = ["plain", "char", "word", "hot", "hotword"]
ENTRY = "ds2_ctc_beam_stream_feed_f32"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lm_dir():
    with tempfile.TemporaryDirectory() as d:
        yield d


def _probs(B, T, C, seed, blank=0, scale=16.0):
    """peaked random per-frame distributions: softmax of scaled normal logits, the blank favoured as in a trained CTC model"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, T, C), generator=g) * scale
    z[..., blank] += 2.0
    return torch.softmax(z, dim=-1).float()


def _lengths(B, T, seed):
    """ragged total lengths: the first utterance full, then (from three utterances on) one of 0 frames and one of 1 frame"""
    g = torch.Generator().manual_seed(seed + 1)
    s = torch.randint(1, T + 1, (B,), generator=g)
    s[0] = T
    if B >= 3:
        s[1], s[2] = 0, 1
    return [int(v) for v in s]


def _arm(lm_dir, arm, C, words=WORDS):
    """the search arguments of an arm for CHARS[C] (blank 0) and the oracle's fusion (None: the plain oracle)"""
    from asr_amd.decoders import BeamCTCDecoder
    from asr_amd.decoders.hotwords import Hotwords
    chars = CHARS[C]
    lm = inner = hot = None
    if arm in ("char", "word", "hotword"):
        mode = "char" if arm == "char" else "word"
        name = os.path.join(lm_dir, f"{mode}_{C}_{'-'.join(words)}.arpa")
        if not os.path.exists(name):
            random_arpa(name, words if mode == "word" else sorted(set(chars) - {"_", " "}), 3, 60, 7)
        lm = BeamCTCDecoder({c: i for i, c in enumerate(chars)}, lm_path=name).lm
        inner = LO.Fusion(LO.NaiveLM(name), chars, 0, chars.index(" ") if " " in chars else None, ALPHA, BETA)
    fusion = inner
    if arm in ("hot", "hotword"):
        phrases, weights = (PHRASES, WEIGHTS) if C > 2 else (["AA"], [1.0])
        hot = Hotwords(list(zip(phrases, weights)), chars, 0)
        fusion = HO.HotFusion([[chars.index(c) for c in p] for p in phrases], weights, inner)
    return dict(lm=lm, alpha=ALPHA if lm is not None else 0.0, beta=BETA if lm is not None else 0.0, hotwords=hot), fusion


def _top_n(arm, C, K):
    """cutoff_top_n: 40, or on the full-grid arms the largest the 4096 candidate slots admit (K = 100: 38, K = 256: 14)"""
    return 40 if arm == "plain" else min(40, 4096 // K - 2)


def _plan(lengths, cuts):
    """cuts: chunk lengths along the time axis -> per chunk, the frames each utterance has in it"""
    plan, c0 = [], 0
    for a in cuts:
        plan.append([max(0, min(n - c0, a)) for n in lengths])
        c0 += a
    return plan


class Driver:
    """The stream at the level of ops: the state, the nodes grown by the plan BeamStream uses, every utterance's own cursor into probs."""

    def __init__(self, dev, probs, K, top_n, cut, search, cap=1, form="plain"):
        from asr_amd import ops
        self.ops, self.dev, self.probs, self.K, self.form = ops, dev, probs, K, form
        self.B, self.T, self.C = probs.shape
        self.args = dict(blank=0, beam_width=K, cutoff_top_n=top_n, cutoff_prob=cut, **search)
        self.state = ops.ctc_beam_stream_state(self.B, K, search["lm"], search["hotwords"], dev)
        self.cap, self.nodes, self.cur = 0, None, [0] * self.B
        self.first_cap = cap

    def _grow(self, need):
        from asr_amd.decoders import stream_capacity
        cap = stream_capacity(self.cap or self.first_cap, need)
        if cap != self.cap:
            self.nodes = self.ops.ctc_beam_stream_nodes(self.B, cap, self.K, self.dev, self.nodes, self.cap)
            self.cap = cap

    def feed(self, take, n_out, pad_frames=0):
        """every utterance consumes its next take[b] frames, in a chunk of max(take) + pad_frames frames whose other rows are NaN"""
        Tc = max(max(take) + pad_frames, 1)
        chunk = torch.full((self.B, Tc, self.C), float("nan"))
        for b, n in enumerate(take):
            chunk[b, :n] = self.probs[b, self.cur[b]:self.cur[b] + n]
        if self.form == "strided":
            x = chunk.transpose(0, 1).contiguous().to(self.dev).transpose(0, 1)
            assert not x.is_contiguous() or self.B == 1 or Tc == 1
        else:
            x = chunk.to(self.dev)
        bound = max(self.cur)
        self._grow(bound + Tc)
        out = self.ops.ctc_beam_stream_feed(x, torch.tensor(take, dtype=torch.int32), self.state, self.nodes, self.cap, bound, n_out, **self.args)
        self.cur = [c + n for c, n in zip(self.cur, take)]
        assert out[5].tolist() == self.cur
        return out

    def read(self, n_out):
        bound = max(self.cur)
        self._grow(max(bound, 1))
        out = self.ops.ctc_beam_stream_feed(None, None, self.state, self.nodes, self.cap, bound, n_out, classes=self.C, **self.args)
        assert out[5].tolist() == self.cur
        return out

    def decode(self, sizes=None):
        """the one-call decode of the frames consumed so far (or of `sizes`)"""
        return self.ops.ctc_beam_decode(self.probs.to(self.dev), torch.tensor(self.cur if sizes is None else sizes, dtype=torch.int32),
                                        **self.args)


def _same_bits(got, want, n_out):
    """the stream's read-out (rows of its own width) against the first n_out slots of a decode call's outputs"""
    gl, go, gn, gs = (x.cpu() for x in got[:4])
    wl, wo, wn, ws = (x.cpu()[:, :n_out] for x in want)
    assert torch.equal(gn, wn), (gn, wn)
    assert torch.equal(gs.view(torch.int32), ws.contiguous().view(torch.int32)), (gs, ws)
    w = min(gl.shape[2], wl.shape[2])
    assert torch.equal(gl[:, :, :w], wl[:, :, :w]) and torch.equal(go[:, :, :w], wo[:, :, :w])
    assert not gl[:, :, w:].any() and not go[:, :, w:].any() and not wl[:, :, w:].any() and not wo[:, :, w:].any()
    assert int(gn.max()) <= w


def _host_stable(out, b):
    """the common (label, offset) prefix of utterance b's live slots in a read-out of all K slots, or None with no live slot"""
    labels, offs, lens, scores = (x.cpu() for x in out[:4])
    live = [k for k in range(labels.shape[1]) if scores[b, k] > -math.inf]
    if not live:
        return None
    beams = [(tuple(labels[b, k, :lens[b, k]].tolist()), tuple(offs[b, k, :lens[b, k]].tolist()), 0.0) for k in live]
    return SO.stable_prefix(beams)


class StableTrack:
    """what check 3 asks of stable_len over the feeds of one stream"""

    def __init__(self, B):
        self.prev, self.head = [0] * B, [None] * B
        self.seen_zero = self.seen_inner = False

    def update(self, out, full):
        labels, offs, lens, scores = (x.cpu() for x in out[:4])
        stable = out[4].tolist()
        for b, s in enumerate(stable):
            assert s >= self.prev[b], (b, s, self.prev[b])                              # never decreases
            live = [k for k in range(labels.shape[1]) if scores[b, k] > -math.inf]
            if full:
                want = _host_stable(out, b)
                assert s == (self.prev[b] if want is None else want), (b, s, want)      # exactly the common prefix; kept with no live beam
            if self.head[b] is not None:                                                # every later result starts with what was stable
                n = len(self.head[b][0])
                for k in live:
                    assert labels[b, k, :n].tolist() == self.head[b][0] and offs[b, k, :n].tolist() == self.head[b][1], (b, k)
            if live:
                assert s <= int(lens[b, live].min())
                self.head[b] = (labels[b, live[0], :s].tolist(), offs[b, live[0], :s].tolist())
                self.seen_zero |= s == 0 and int(lens[b, 0]) > 0
                self.seen_inner |= 0 < s < int(lens[b, 0])
            self.prev[b] = s


GRID = [   # B, T, C, K, the arms the shape admits
    (7, 12, 7, 4, ARMS),
    (7, 40, 29, 100, ARMS),
    (3, 5, 2, 1, ["plain", "char", "hot"]),       # (two classes leave no room for a space: no word mode)
    (2, 6, 29, 256, ARMS),
]
POINTS = [(B, T, C, K, arm) for B, T, C, K, arms in GRID for arm in arms]


def _cut_sets(T):
    return {"each": [1] * T, "one": [T], "uneven": [1, T - 2, 1]}


@pytest.mark.parametrize("B,T,C,K,arm", POINTS, ids=[f"B{p[0]}-T{p[1]}-C{p[2]}-K{p[3]}-{p[4]}" for p in POINTS])
def test_resume_and_partials_have_the_bits_of_one_decode(dev, lm_dir, B, T, C, K, arm):
    """Checks 1-3 at every grid point: ragged lengths (0 and 1 frame among them), a node buffer that starts with one frame and grows at
    every feed, and per cut set: every partial read-out (all K slots) equals the decode of the frames so far; the final read-out equals
    the decode of everything; the same cuts without any read-out end in the same bits; stable_len as StableTrack checks it."""
    search, _ = _arm(lm_dir, arm, C)
    top_n, cut = _top_n(arm, C, K), 1.0 if K != 100 else 0.99
    probs, lengths = _probs(B, T, C, 1000 + B + T + C + K), _lengths(B, T, K)
    for name, cuts in _cut_sets(T).items():
        if name == "each" and T > 12:
            cuts = [3] * (T // 3) + [T % 3] * (T % 3 > 0)          # (the long point: thirteen feeds and one-call decodes, not forty)
        plan = _plan(lengths, cuts)
        form = "strided" if name == "uneven" else "plain"
        a, b = Driver(dev, probs, K, top_n, cut, search, 1, form), Driver(dev, probs, K, top_n, cut, search, 1, form)
        track = StableTrack(B)
        for take in plan:
            out = a.feed(take, K)
            _same_bits(out, a.decode(), K)
            track.update(out, True)
            assert b.feed(take, 0)[:4] == (None, None, None, None)
        want = a.decode(lengths)
        for d in (a, b):
            out = d.read(K)
            _same_bits(out, want, K)
        track.update(out, True)


def _oracle_compare(probs, sizes, out, fusion, K, top_n, cut):
    """test_gpu_ctc_beam.py::_compare's rule on a read-out -> (utterances, those whose best beam was compared exactly, those decisive)"""
    labels, offs, lens, scores = (x.cpu() for x in out[:4])
    exact = dec = 0
    for b in range(probs.shape[0]):
        res = SO.search_at_cuts(probs[b].double().numpy(), [sizes[b]], fusion, 0, K, top_n, cut)[0]
        beams = res["beams"]
        if SO.decisive(res, fusion):
            dec += 1
            got = {tuple(labels[b, k, :lens[b, k]].tolist()): k for k in range(K) if scores[b, k] > -math.inf}
            assert len(got) == len(beams), (b, len(got), len(beams))
            for k, (pr, off, s) in enumerate(beams):
                kk = got[pr]
                assert abs(float(scores[b, kk]) - s) <= 1e-4 * max(1.0, abs(s)), (b, k, float(scores[b, kk]), s)
                assert tuple(offs[b, kk, :lens[b, kk]].tolist()) == off, (b, k)
            for k in range(len(beams), K):
                assert int(lens[b, k]) == 0 and scores[b, k] == -math.inf
            if beams:                                                   # (with no live beam the stream keeps the value it had)
                assert int(out[4][b]) == SO.stable_prefix(beams), (b, int(out[4][b]), beams)
            ranks = LO.decisive_ranks(res)
        else:
            ranks = LO.decisive_ranks(res, 1e-5)
        for k in ranks:
            pr, off, s = beams[k]
            assert tuple(labels[b, k, :lens[b, k]].tolist()) == pr, (b, k)
            assert tuple(offs[b, k, :lens[b, k]].tolist()) == off, (b, k)
            assert abs(float(scores[b, k]) - s) <= 1e-4 * max(1.0, abs(s)), (b, k, float(scores[b, k]), s)
        exact += 0 in ranks
    return probs.shape[0], exact, dec


ORACLE_SEED, ORACLE_SCALE = 5, 8.0


@pytest.mark.parametrize("arm", ARMS)
def test_small_point_against_the_oracles(dev, lm_dir, arm):
    """(7, 12, 7, 4), one frame per feed, against the fp64 oracles at EVERY cut: the read-out by the one-call tests' rule, and on the
    utterances whose every oracle decision cleared 1e-4 stable_len equals the oracle's common prefix.  At least 90 % of the (utterance,
    cut) pairs must be decisive and have their best beam compared exactly.  On the CPU the oracles alone give, for these frames
    (seed 5, logits scaled by 8), of the 84 pairs: best beam decided 84 in every arm; decisive 84 (plain, character LM, word LM,
    hotwords) and 82 (hotwords + word LM).  The oracle's beams have 0 < stable prefix < the best beam's length at 16 to 22 of the pairs
    and a stable prefix of 0 under a non-empty best beam at 32 to 51, depending on the arm: both cases are asserted in every arm."""
    B, T, C, K = 7, 12, 7, 4
    search, fusion = _arm(lm_dir, arm, C)
    probs, lengths = _probs(B, T, C, ORACLE_SEED, 0, ORACLE_SCALE), _lengths(B, T, K)
    d, track = Driver(dev, probs, K, 40, 1.0, search, 1), StableTrack(B)
    n_all = exact_all = dec_all = 0
    for take in _plan(lengths, [1] * T):
        out = d.feed(take, K)
        track.update(out, True)
        n, exact, dec = _oracle_compare(probs, d.cur, out, fusion, K, 40, 1.0)
        n_all, exact_all, dec_all = n_all + n, exact_all + exact, dec_all + dec
    assert exact_all >= 0.9 * n_all and dec_all >= 0.9 * n_all, f"{arm}: {exact_all} exact, {dec_all} decisive of {n_all}"
    assert track.seen_inner and track.seen_zero


def test_chunks_that_skip_utterances_and_padded_chunks(dev, lm_dir):
    """sizes of 0 for some utterances while they still have frames (their streams simply stop advancing and fall behind the others), for
    all utterances (nothing changes but the read-out is still right), and chunks longer than any utterance's share (NaN rows past the
    sizes are never read)"""
    B, T, C, K = 7, 12, 7, 4
    probs = _probs(B, T, C, 77)
    for arm in ("plain", "word", "hotword"):
        search, _ = _arm(lm_dir, arm, C)
        d, track = Driver(dev, probs, K, 40, 1.0, search, 1), StableTrack(B)
        plans = [[3, 0, 2, 0, 1, 0, 4], [0] * B, [0, 5, 0, 5, 0, 5, 0], [2, 2, 2, 2, 2, 2, 2], [0] * B, [7, 5, 8, 5, 9, 5, 6]]
        for i, take in enumerate(plans):
            before = d.state.clone()
            out = d.feed(take, K, pad_frames=i % 3)
            _same_bits(out, d.decode(), K)
            track.update(out, True)
            if not any(take):
                assert torch.equal(d.state, before)                     # loaded and saved: not a byte differs
        assert d.cur == [12] * B
        _same_bits(d.read(K), d.decode(), K)


def test_n_out_below_k_and_a_partial_leaves_the_stream_alone(dev, lm_dir):
    """n_out < K returns the first n_out slots; stable_len still speaks for all live beams; reading (the end stage of the word-LM and
    hotword arms re-scores and re-sorts) changes nothing the next feed sees"""
    B, T, C, K = 7, 12, 7, 4
    probs, lengths = _probs(B, T, C, 5, 0, 4.0), [12, 0, 1, 7, 12, 9, 3]
    for arm in ARMS:
        search, _ = _arm(lm_dir, arm, C)
        a, b = Driver(dev, probs, K, 40, 1.0, search, 4), Driver(dev, probs, K, 40, 1.0, search, 4)
        for take in _plan(lengths, [5, 4, 3]):
            full, some = a.feed(take, K), b.feed(take, 1)
            a.read(K), a.read(2)                                     # extra read-outs in between
            _same_bits(some, a.decode(), 1)
            assert some[4].tolist() == full[4].tolist() and some[0].shape[1] == 1
        _same_bits(b.read(K), a.decode(lengths), K)
        _same_bits(a.read(K), a.decode(lengths), K)


def test_dead_stream_and_empty_stream(dev, lm_dir):
    """A word-LM stream whose dictionary rules out every extension dies and stays dead across feeds, with the one-call decode's outputs
    and the stable prefix it had; finish() / a read-out with no feed is the decode of 0 frames."""
    from asr_amd.decoders import BeamCTCDecoder
    C, K = 7, 4
    search, _ = _arm(lm_dir, "word", C, words=["AB", "B"])            # no word starts with C, D or E
    rows = [1, 3, 3, 0, 1, 2]                                          # "A", then only labels the dictionary rules out
    probs = torch.full((1, len(rows), C), 0.01)
    for t, c in enumerate(rows):
        probs[0, t, c] = 1.0 - 0.01 * (C - 1)
    d, track = Driver(dev, probs, K, 1, 1.0, search, 1), StableTrack(1)            # cutoff_top_n = 1: the peak alone is kept
    stables = []
    for take in _plan([len(rows)], [1] * len(rows)):
        out = d.feed(take, K)
        _same_bits(out, d.decode(), K)
        track.update(out, True)
        stables.append(int(out[4][0]))
    assert stables == [1] * len(rows)                                 # "A" was common to the one live beam; kept after the stream died
    assert (out[3].cpu() == -math.inf).all() and not out[2].cpu().any()
    _same_bits(d.read(K), d.decode(), K)
    for arm in ARMS:                                                  # no feed at all
        search, _ = _arm(lm_dir, arm, C)
        e = Driver(dev, _probs(3, 4, C, 1), K, 40, 1.0, search, 1)
        out = e.read(K)
        _same_bits(out, e.decode([0, 0, 0]), K)
        assert out[4].tolist() == [0, 0, 0] and out[5].tolist() == [0, 0, 0]
    dec = BeamCTCDecoder({c: i for i, c in enumerate(CHARS[C])}, beam_width=K)
    strings, offsets = dec.open_stream(batch=2).finish()
    want = dec.decode(_probs(2, 3, C, 1), torch.tensor([0, 0]))
    assert strings == want[0] == [[""] * K] * 2 and [[o.tolist() for o in u] for u in offsets] == [[[]] * K] * 2


def test_entry_refusals(dev, lm_dir):
    """the entry's own refusals, each with a message that begins with its name"""
    from asr_amd import _lib, ops
    lib = _lib.load()
    B, T, C, K = 2, 3, 7, 4
    x = _probs(B, T, C, 0).to(dev)
    search, _ = _arm(lm_dir, "char", C)
    tab = search["lm"].device_tables(dev)
    lm = (tab.data_ptr(), tab.numel(), search["lm"].order, search["lm"].mode, -1, ALPHA, BETA)
    no_lm = (None, 0, 0, 0, -1, 0.0, 0.0)
    state = ops.ctc_beam_stream_state(B, K, search["lm"], None, dev)
    nodes = ops.ctc_beam_stream_nodes(B, 8, K, dev)
    outs = [torch.zeros((B, K, 8), dtype=torch.int32, device=dev) for _ in range(2)] + [torch.zeros((B, K), dtype=torch.int32, device=dev),
                                                                                         torch.zeros((B, K), dtype=torch.float32, device=dev)]
    tail = torch.zeros((2, B), dtype=torch.int32, device=dev)

    def call(lm_args=no_lm, state_bytes=None, nodes_bytes=None, cap=8, bound=0, n_out=K, W=8, T=T, top_n=40, beam=K):
        return lib.ds2_ctc_beam_stream_feed_f32(x.data_ptr() if T else None, x.stride(0), x.stride(1), B, T, C, None, 0, beam, top_n, 1.0, *lm_args,
                                                None, None, 0, state.data_ptr(), state.numel() if state_bytes is None else state_bytes,
                                                nodes.data_ptr(), nodes.numel() * 4 if nodes_bytes is None else nodes_bytes, cap, bound, n_out, W,
                                                *(o.data_ptr() for o in outs), tail[0].data_ptr(), tail[1].data_ptr(), None)

    def refused(what, **kw):
        assert call(**kw) != 0
        msg = lib.ds2_last_error().decode()
        assert msg.startswith(ENTRY + ": ") and what in msg, msg

    refused("state too small", lm_args=lm, state_bytes=lib.ds2_ctc_beam_stream_state_bytes(B, K, 1, 0) - 1)
    refused("state too small", state_bytes=lib.ds2_ctc_beam_stream_state_bytes(B, K, 0, 0) - 1)
    refused("node buffer too small", nodes_bytes=12 * B * 8 * K - 1)
    refused("node buffer too small", cap=8, bound=6)                       # 6 + 3 frames in a capacity of 8
    refused("node buffer too small", cap=2)
    refused("cannot hold", W=2)
    refused("cannot hold", W=7, bound=5)
    refused("n_out", n_out=K + 1)
    refused("n_out", n_out=-1)
    refused("nothing to do", T=0, n_out=0)
    torch.cuda.synchronize()
    assert not tail.any() and not state.any()                              # nothing was launched
    assert call() == 0 and call(bound=3, n_out=0) == 0
    torch.cuda.synchronize()
    assert tail[1].tolist() == [6, 6]
    with pytest.raises(ValueError, match="ctc_beam_stream_feed: with a language model beam_width"):
        ops.ctc_beam_stream_feed(_probs(1, 2, 29, 0).to(dev), None, state, nodes, 8, 0, 0, beam_width=256, cutoff_top_n=40, lm=_arm(lm_dir, "char", 29)[0]["lm"])
    with pytest.raises(ValueError, match="n_out"):
        ops.ctc_beam_stream_feed(x, None, state, nodes, 8, 0, K + 1, beam_width=K)


def test_lm_candidate_limit_through_the_entry(dev, lm_dir):
    from asr_amd import _lib, ops
    lib = _lib.load()
    C, K = 29, 256
    search, _ = _arm(lm_dir, "char", C)
    tab = search["lm"].device_tables(dev)
    x = _probs(1, 2, C, 0).to(dev)
    state, nodes = ops.ctc_beam_stream_state(1, K, search["lm"], None, dev), ops.ctc_beam_stream_nodes(1, 4, K, dev)
    tail = torch.zeros((2, 1), dtype=torch.int32, device=dev)
    rc = lib.ds2_ctc_beam_stream_feed_f32(x.data_ptr(), x.stride(0), x.stride(1), 1, 2, C, None, 0, K, 15, 1.0, tab.data_ptr(), tab.numel(),
                                          search["lm"].order, search["lm"].mode, -1, ALPHA, BETA, None, None, 0, state.data_ptr(), state.numel(),
                                          nodes.data_ptr(), nodes.numel() * 4, 4, 0, 0, 0, None, None, None, None, tail[0].data_ptr(),
                                          tail[1].data_ptr(), None)
    msg = lib.ds2_last_error().decode()
    assert rc != 0 and msg.startswith(ENTRY + ": ") and "= 4352 exceeds the 4096 candidate slots" in msg, msg


@pytest.mark.parametrize("arm", ["plain", "hotword"])
def test_beam_stream_class_against_decode(dev, lm_dir, arm):
    """BeamCTCDecoder.open_stream: host and device chunks, nbest, partial=False, the growth from a capacity of one frame; finish() is
    decode() of the concatenated frames, last_scores included; every partial's stable_text starts every later text"""
    from asr_amd.decoders import BeamCTCDecoder
    B, T, C, K = 3, 12, 7, 4
    search, _ = _arm(lm_dir, arm, C)

    def decoder():
        d = BeamCTCDecoder({c: i for i, c in enumerate(CHARS[C])}, beam_width=K, alpha=search["alpha"], beta=search["beta"])
        d.lm = search["lm"]
        d.set_hotwords(search["hotwords"])
        return d
    dec, ref = decoder(), decoder()
    probs, lengths = _probs(B, T, C, 21, 0, 4.0), [12, 5, 9]
    want_s, want_o = dec.decode(probs, torch.tensor(lengths))
    want_scores = dec.last_scores.clone()
    for partial in (True, False):
        s = dec.open_stream(batch=B, nbest=3, capacity=1)
        dec.beam_width = 2                                              # the stream keeps the width it was opened with
        stable, c0 = [""] * B, 0
        for i, a in enumerate([1, 4, 2, 5]):
            chunk = probs[:, c0:c0 + a]
            sizes = [max(0, min(n - c0, a)) for n in lengths]
            recs = s.feed(chunk if i % 2 else chunk.to(dev), sizes, partial=partial)
            c0 += a
            assert s.frames == [min(n, c0) for n in lengths] and s.capacity >= c0
            if not partial:
                assert recs is None
                continue
            ref_s, ref_o = ref.decode(probs, torch.tensor(s.frames))
            for b, r in enumerate(recs):
                assert r["text"] == ref_s[b][0] and r["offsets"].tolist() == ref_o[b][0].tolist() and r["frames"] == s.frames[b]
                assert r["score"] == float(ref.last_scores[b, 0])
                assert [n[0] for n in r["nbest"]] == ref_s[b][:3] and r["stable_text"] == r["text"][:r["stable"]]
                assert r["text"].startswith(stable[b]) and len(r["stable_text"]) >= len(stable[b])
                stable[b] = r["stable_text"]
        dec.beam_width = K
        got_s, got_o = s.finish()
        assert got_s == want_s and [[o.tolist() for o in u] for u in got_o] == [[o.tolist() for o in u] for u in want_o]
        assert torch.equal(dec.last_scores.view(torch.int32), want_scores.view(torch.int32))
        assert all(t[0].startswith(p) for t, p in zip(got_s, stable)) and s.closed
        with pytest.raises(ValueError, match="closed"):
            s.feed(probs[:, :1])
    one = dec.open_stream()                                             # batch 1 takes (T, C)
    rec = one.feed(probs[0, :7])
    assert rec[0]["frames"] == 7 and one.frames == [7]
    one.feed(probs[0, 7:].to(dev), partial=False)
    assert one.finish()[0][0] == want_s[0]


def tiny_model():
    import pandas as pd
    from asr_amd import DeepSpeech
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                           spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    torch.manual_seed(3)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": chars}).to_csv(path, index=False)
        model = DeepSpeech(audio_conf=conf, decoder=None, label_path=path, rnn_type="gru", rnn_hidden_size=32, rnn_hidden_layers=2,
                           bidirectional=True)
    return model.to(torch.device("cuda", 0)).eval()


def test_stream_long_on_a_tiny_model(dev):
    """Four batches of windows: the final item is decode() of posteriors_long's result, every stable_text starts every later text, and
    posteriors_long still returns the stitched forwards of its documentation, bit for bit."""
    from asr_amd.decoders import BeamCTCDecoder, GreedyDecoder, words_from_offsets
    from asr_amd.functional import long_windows
    model = tiny_model()
    spect = torch.randn((161, 437), generator=torch.Generator().manual_seed(11))
    dec = BeamCTCDecoder(model.labels, beam_width=8)
    got = model.posteriors_long(spect, window=128, overlap=16, batch_size=2)
    wins = long_windows(437, 128, 16)
    assert len(wins) == 5
    want = torch.full((219, len(model.labels)), float("nan"), device=dev)
    with torch.no_grad():
        for chunk in (wins[:2], wins[2:4], wins[4:]):
            x = torch.zeros((len(chunk), 1, 161, max(w[1] for w in chunk)))
            for n, w in enumerate(chunk):
                x[n, 0, :, :w[1]] = spect[:, w[0]:w[0] + w[1]]
            out, _ = model.forward(x.to(dev), torch.tensor([w[1] for w in chunk], dtype=torch.int32))
            for n, (_, _, out_start, keep_from, keep_to) in enumerate(chunk):
                want[out_start:out_start + keep_to - keep_from] = out[n, keep_from:keep_to]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    strings, offsets = dec.decode(got[None])
    items = list(model.stream_long(spect, window=128, overlap=16, batch_size=2, decoder=dec))
    assert len(items) == 4 and [i["final"] for i in items] == [False, False, False, True]
    assert [i["frames"] for i in items] == [wins[1][2] + wins[1][4] - wins[1][3], wins[3][2] + wins[3][4] - wins[3][3], 219, 219]
    last = items[-1]
    assert last["text"] == strings[0][0] and last["seconds"] == 219 * 0.02
    assert last["words"] == [w + (w[1] * 0.02, w[2] * 0.02) for w in words_from_offsets(strings[0][0], offsets[0][0])]
    assert items[2]["text"] == last["text"]
    for i, item in enumerate(items):
        assert item["text"].startswith(item["stable_text"])
        for later in items[i:]:
            assert later["text"].startswith(item["stable_text"])
    model.decoder = dec
    assert list(model.stream_long(spect.to(dev)[None, None], 128, 16, 5))[-1]["text"] == last["text"]
    with pytest.raises(TypeError):
        model.stream_long(spect, decoder=GreedyDecoder(model.labels))
