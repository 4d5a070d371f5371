"""-m gpu: commit and compaction of the streaming beam search (ds2_ctc_beam_stream_commit, csrc/ctc_beam_commit.h;
ds2_ctc_beam_stream_feed_committed_f32; BeamCTCDecoder.open_stream(commit=True), BeamStream.finish(index)).  The yardstick without a
forced cut is the one-call decode, as in test_gpu_beam_stream.py: the committed pairs joined to the read-out must have its BITS after
any cuts, with a commit before every feed and a node storage that starts with one row.  The size of the live tree and the forced cut are
held to tests/ctc_beam_commit_oracle.py."""
import math

import pytest
import torch

import ctc_beam_commit_oracle as CO
import ctc_beam_oracle as O
import test_gpu_beam_stream as S
from test_gpu_beam_stream import dev, lm_dir, _probs   # noqa: F401  (the fixtures and the inputs of the streaming tests)

pytestmark = pytest.mark.gpu
ENTRY = "ds2_ctc_beam_stream_commit"
# the forced-cut test's point: B, T, C, K, chunk, max_lag, commit_every, seed, logit scale (test_cpu_beam_commit checks the oracle's share)
FORCED = (10, 160, 7, 8, 20, 40, 20, 31, 16.0)


def _silence(B, T, C, seed, peaked=40):
    """silence: the blank's logit +6 under unit-normal noise; the last `peaked` frames are test_gpu_beam_stream's peaked inputs"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, T, C), generator=g)
    z[..., 0] += 6.0
    x = torch.softmax(z, dim=-1).float()
    x[:, T - peaked:] = _probs(B, peaked, C, seed + 1)
    return x


class Driver:
    """A committing stream at the level of ops: a commit before every feed (once there are nodes), the plan BeamStream uses for the
    rows, the committed pairs kept per utterance and joined to every read-out."""

    def __init__(self, dev, probs, K, top_n, cut, search, cap=1):
        from asr_amd import ops
        self.ops, self.dev, self.probs, self.K, self.search = ops, dev, probs, K, search
        self.B, self.T, self.C = probs.shape
        self.args = dict(blank=0, beam_width=K, cutoff_top_n=top_n, cutoff_prob=cut, **search)
        self.state = ops.ctc_beam_stream_state(self.B, K, search["lm"], search["hotwords"], dev)
        self.cap, self.nodes, self.cur, self.first_cap = 0, None, [0] * self.B, cap
        self.rows, self.lab, self.done = [0] * self.B, [0] * self.B, [([], []) for _ in range(self.B)]
        self.max_rows = 0

    def commit(self, chunk, cut_frame=None):
        """-> (info (B, 4), dropped (B)) on the host, or None before the first feed"""
        from asr_amd.decoders import commit_capacity
        if self.nodes is None:
            return None
        width = max(self.lab)
        fresh = self.ops.ctc_beam_stream_nodes(self.B, self.cap, self.K, self.dev)
        cut = None if cut_frame is None else torch.tensor(cut_frame, dtype=torch.int32, device=self.dev)
        packed = self.ops.ctc_beam_stream_commit(self.state, self.nodes, self.cap, fresh, self.cap, self.K, self.search["lm"],
                                                 self.search["hotwords"], width, cut)[4]
        info, dropped, labels, offs = self.ops.commit_unpack(packed.cpu(), self.B, width)
        self.nodes = fresh
        for b in range(self.B):
            n = int(info[b, 0])
            assert 0 <= n <= width and not labels[b, n:].any() and not offs[b, n:].any()
            self.done[b][0].extend(labels[b, :n].tolist())
            self.done[b][1].extend(offs[b, :n].tolist())
            if self.done[b][1]:
                assert int(info[b, 3]) == self.done[b][1][-1]                 # the frame of the last committed pair
        self.lab = info[:, 2].tolist()
        rows, cap = commit_capacity(self.cap, info[:, 1].tolist(), self.K, chunk)
        self.rows = [(m + self.K - 1) // self.K for m in info[:, 1].tolist()]
        assert rows == max(self.rows)
        if cap != self.cap:
            self.nodes = self.ops.ctc_beam_stream_nodes(self.B, cap, self.K, self.dev, self.nodes, self.cap)
            self.cap = cap
        return info, dropped

    def _call(self, x, sizes, Tc, n_out):
        from asr_amd.decoders import stream_capacity
        cap = stream_capacity(self.cap or self.first_cap, max(self.rows) + Tc)
        if cap != self.cap:                                                   # (the first feed; later the commit has made room)
            self.nodes = self.ops.ctc_beam_stream_nodes(self.B, cap, self.K, self.dev, self.nodes, self.cap)
            self.cap = cap
        out = self.ops.ctc_beam_stream_feed_committed(x, sizes, self.state, self.nodes, self.cap, max(self.rows), max(self.lab), n_out,
                                                      classes=self.C, **self.args)
        self.rows, self.lab = [r + Tc for r in self.rows], [n + Tc for n in self.lab]
        self.max_rows = max(self.max_rows, max(self.rows))
        return out

    def feed(self, take, n_out):
        Tc = max(max(take), 1)
        chunk = torch.full((self.B, Tc, self.C), float("nan"))
        for b, n in enumerate(take):
            chunk[b, :n] = self.probs[b, self.cur[b]:self.cur[b] + n]
        out = self._call(chunk.to(self.dev), torch.tensor(take, dtype=torch.int32), Tc, n_out)
        self.cur = [c + n for c, n in zip(self.cur, take)]
        assert out[5].tolist() == self.cur
        return self.joined(out)

    def read(self, n_out):
        out = self._call(None, None, 0, n_out)
        assert out[5].tolist() == self.cur
        return self.joined(out)

    def joined(self, out):
        """a read-out -> (labels, offsets (B, n_out, W'), lens, scores, stable, frames) on the host with the committed pairs in front"""
        if out[0] is None:
            return out
        labels, offs, lens, scores = (x.cpu() for x in out[:4])
        B, n_out, W = labels.shape
        width = max(len(d[0]) for d in self.done) + W
        full_l, full_o = torch.zeros((B, n_out, width), dtype=torch.int32), torch.zeros((B, n_out, width), dtype=torch.int32)
        for b in range(B):
            n = len(self.done[b][0])
            for k in range(n_out):
                if scores[b, k] > -math.inf:
                    assert int(lens[b, k]) >= n and int(lens[b, k]) - n <= W
                    full_l[b, k, :n], full_o[b, k, :n] = torch.tensor(self.done[b][0], dtype=torch.int32), torch.tensor(self.done[b][1], dtype=torch.int32)
                    full_l[b, k, n:n + W], full_o[b, k, n:n + W] = labels[b, k], offs[b, k]
                else:
                    assert int(lens[b, k]) == 0 and not labels[b, k].any()
        return full_l, full_o, lens, scores, out[4].cpu(), out[5].cpu()

    def decode(self, sizes=None):
        return self.ops.ctc_beam_decode(self.probs.to(self.dev), torch.tensor(self.cur if sizes is None else sizes, dtype=torch.int32),
                                        **self.args)


def _beams(out, b):
    """utterance b's live slots of a joined read-out -> [(labels, offsets, score bits)] in slot order"""
    labels, offs, lens, scores = out[:4]
    bits = scores.view(torch.int32)
    return [(tuple(labels[b, k, :lens[b, k]].tolist()), tuple(offs[b, k, :lens[b, k]].tolist()), int(bits[b, k]))
            for k in range(labels.shape[1]) if scores[b, k] > -math.inf]


def _tree_size(out, b):
    """the live tree the contract leaves after a commit, counted on the read-out before it (0 with no live beam)"""
    beams = _beams(out, b)
    return CO.live_nodes(beams, int(out[4][b])) if beams else 0


GRID = [(7, 12, 7, 4, S.ARMS), (7, 40, 29, 100, S.ARMS), (2, 6, 29, 256, ["plain"])]
POINTS = [(B, T, C, K, arm) for B, T, C, K, arms in GRID for arm in arms]


@pytest.mark.parametrize("B,T,C,K,arm", POINTS, ids=[f"B{p[0]}-T{p[1]}-C{p[2]}-K{p[3]}-{p[4]}" for p in POINTS])
def test_committed_stream_has_the_bits_of_one_decode(dev, lm_dir, B, T, C, K, arm):
    """Ragged lengths (0 and 1 frame among them), a first capacity of one row, a commit before every feed, per cut set: after every
    feed the committed pairs plus the read-out of all K slots equal the decode of the frames so far (labels, offsets, lengths, score
    bits); the final read-out equals the decode of everything; at every commit info's M is live_nodes of the read-out before it, the
    pairs it commits are the stable ones, and the third field is the longest live beam less the committed length."""
    search, _ = S._arm(lm_dir, arm, C)
    top_n, cut = S._top_n(arm, C, K), 1.0 if K != 100 else 0.99
    probs, lengths = _probs(B, T, C, 1000 + B + T + C + K), S._lengths(B, T, K)
    step = 1 if T <= 12 else 3
    for cuts in ([step] * (T // step) + [T % step] * (T % step > 0), [1, T - 2, 1]):
        d, out, moved = Driver(dev, probs, K, top_n, cut, search, 1), None, 0
        for take in S._plan(lengths, cuts):
            got = d.commit(max(max(take), 1))
            if got is not None:
                info, dropped = got
                assert not dropped.any()
                for b in range(B):
                    assert int(info[b, 1]) == _tree_size(out, b), (b, info[b].tolist())
                    live = _beams(out, b)
                    if live:
                        assert len(d.done[b][0]) == int(out[4][b])                              # everything stable has left
                        assert int(info[b, 2]) == max(len(x[0]) for x in live) - int(out[4][b])
                    moved += int(info[b, 0])
            out = d.feed(take, K)
            S._same_bits(out, d.decode(), K)
        S._same_bits(d.read(K), d.decode(lengths), K)
        assert moved > 0 or K != 4                                                               # (pairs did leave the device on the way)


def test_bitmap_in_the_workspace(dev):
    """A storage of 2048 rows at K = 256 is 524288 nodes: past what the bitmap's LDS holds, so mark and scan run in the entry's workspace;
    with 4 rows at K = 4 beside it for the same frames in LDS.  Both keep the decode's bits and report the same tree."""
    from asr_amd import _lib
    B, T, C = 2, 9, 29
    probs = _probs(B, T, C, 77)
    plain = dict(lm=None, alpha=0.0, beta=0.0, hotwords=None)
    assert _lib.load().ds2_ctc_beam_stream_commit_workspace_bytes(B, 2048, 256) > 0 == _lib.load().ds2_ctc_beam_stream_commit_workspace_bytes(B, 64, 256)
    sizes = []
    for cap in (2048, 64):
        d, out, seen = Driver(dev, probs, 256, 40, 1.0, plain, cap), None, []
        for take in S._plan([T, 5], [3, 3, 3]):
            got = d.commit(3)
            if got is not None:
                seen.append(got[0][:, 1].tolist())
                assert seen[-1] == [_tree_size(out, b) for b in range(B)]
            out = d.feed(take, 256)
            S._same_bits(out, d.decode(), 256)
        assert d.cap == cap and max(seen[-1]) > 256
        sizes.append(seen)
    assert sizes[0] == sizes[1]


def test_silence_keeps_the_first_capacity(dev):
    """BeamStream(commit=True) over 360 frames of silence and 40 peaked ones, B = 2, K = 8, chunks of 20, a first capacity of 32 rows:
    live_nodes is the oracle's count at every commit, the capacity is what the plan gives for those counts, over the silent stretch it
    stays at 32 with a tree of a handful of nodes, the records and the result are those of an uncommitted twin, which ends at 512 rows."""
    from asr_amd.decoders import BeamCTCDecoder, commit_capacity
    B, T, C, K, chunk = 2, 400, 7, 8, 20
    probs = _silence(B, T, C, 3)
    dec = BeamCTCDecoder({c: i for i, c in enumerate(S.CHARS[C])}, beam_width=K)
    s, twin = dec.open_stream(batch=B, capacity=32, commit=True), dec.open_stream(batch=B, capacity=32)
    oracle = [CO.ForcedSearch(beam_width=K) for _ in range(B)]
    x, cap, silent_counts = probs.to(dev), 32, []
    for t0 in range(0, T, chunk):
        before = s.commits
        recs = s.feed(x[:, t0:t0 + chunk])
        if s.commits != before:
            counts = [CO.live_nodes(o.beams, o.stable) for o in oracle]                          # (the commit ran before the chunk)
            assert s.live_nodes == counts, (t0, s.live_nodes, counts)
            cap = commit_capacity(cap, counts, K, chunk)[1]
            if t0 <= T - 40:
                silent_counts += counts
        assert s.capacity == cap, (t0, s.capacity, cap)
        if t0 < T - 40:
            assert s.capacity == 32
        for o, b in zip(oracle, range(B)):
            o.feed(probs[b, t0:t0 + chunk].double().numpy())
        want = twin.feed(x[:, t0:t0 + chunk])
        for r, w in zip(recs, want):
            assert r["offsets"].tolist() == w["offsets"].tolist() and {k: v for k, v in r.items() if k != "offsets"} == \
                {k: v for k, v in w.items() if k != "offsets"}
    assert s.commits == T // chunk - 1 and silent_counts and max(silent_counts) <= 2 * K, silent_counts   # chunk 2 of 20 no longer fits 32 rows
    assert twin.capacity == 512 and s.capacity < 512
    got, want = s.finish(), twin.finish()
    assert got[0] == want[0] and [[o.tolist() for o in u] for u in got[1]] == [[o.tolist() for o in u] for u in want[1]]


def test_stall_grows_by_doubling_and_keeps_the_bits(dev):
    """The peaked inputs at T = 400, K = 8: the stable prefix stalls, so without max_lag the live tree outgrows the first 32 rows and the
    storage doubles AFTER compaction, by the plan; finish() still has decode()'s bits."""
    from asr_amd.decoders import BeamCTCDecoder, commit_capacity
    T, C, K, chunk = 400, 7, 8, 20
    probs = _probs(1, T, C, 9)
    dec = BeamCTCDecoder({c: i for i, c in enumerate(S.CHARS[C])}, beam_width=K)
    want_s, want_o = dec.decode(probs)
    want_scores = dec.last_scores.clone()
    s, x, cap, peak = dec.open_stream(capacity=32, commit=True), probs.to(dev), 32, 0
    for t0 in range(0, T, chunk):
        before = s.commits
        rec = s.feed(x[:, t0:t0 + chunk], partial=t0 + chunk == T)
        if s.commits != before:
            cap = commit_capacity(cap, s.live_nodes, K, chunk)[1]
            peak = max(peak, s.live_nodes[0])
        assert s.capacity == cap
    assert rec[0]["text"] == want_s[0][0] and 2 <= s.commits <= T // chunk - 1
    assert 32 < s.capacity < 512 and s.capacity == 1 << (s.capacity.bit_length() - 1) and peak > 32 * K - chunk * K
    got_s, got_o = s.finish()
    assert got_s == want_s and [[o.tolist() for o in u] for u in got_o] == [[o.tolist() for o in u] for u in want_o]
    assert torch.equal(dec.last_scores.view(torch.int32), want_scores.view(torch.int32))


def test_forced_cut_against_the_oracle(dev):
    """The plain arm driven through the cut_frame mask with max_lag = 40, commit_every = 20 and chunks of 20, to the end of the stream,
    against the restated search by the rule of test_gpu_ctc_beam.py: exact where every decision of the oracle cleared 1e-4 (the lead of
    the first slot at a cut among them), at least 90 % of the utterances compared exactly.  The rows never exceed max_lag +
    commit_every + 1 + chunk."""
    B, T, C, K, chunk, lag, every, seed, scale = FORCED
    probs = _probs(B, T, C, seed, 0, scale)
    d = Driver(dev, probs, K, 40, 1.0, dict(lm=None, alpha=0.0, beta=0.0, hotwords=None), 1)
    forced = [0] * B
    for t0 in range(0, T, chunk):
        got = d.commit(chunk, [t0 - lag] * B)
        if got is not None:
            forced = [f + (int(n) > 0) for f, n in zip(forced, got[1])]
        d.feed([chunk] * B, 0)
        assert max(d.rows) <= lag + every + 1 + chunk, (t0, d.rows)
    labels, offs, lens, scores, stable, _ = d.read(K)
    exact = dec = 0
    for b in range(B):
        o, _ = CO.run(probs[b].double().numpy(), chunk, lag, every, beam_width=K)
        res, beams = o.result(), o.beams
        if O.decisive(res):
            dec += 1
            assert forced[b] == o.forced, (b, forced[b], o.forced)
            got = {tuple(labels[b, k, :lens[b, k]].tolist()): k for k in range(K) if scores[b, k] > -math.inf}
            assert len(got) == len(beams), (b, len(got), len(beams))
            for k, (pr, off, sc) in enumerate(beams):
                kk = got[pr]
                assert abs(float(scores[b, kk]) - sc) <= 1e-4 * max(1.0, abs(sc)), (b, k, float(scores[b, kk]), sc)
                assert tuple(offs[b, kk, :lens[b, kk]].tolist()) == off, (b, k)
            assert int(stable[b]) == o.stable, (b, int(stable[b]), o.stable)
            ranks = O.decisive_ranks(res)
        else:
            ranks = O.decisive_ranks(res, 1e-5)
        for k in ranks:
            pr, off, sc = beams[k]
            assert tuple(labels[b, k, :lens[b, k]].tolist()) == pr and tuple(offs[b, k, :lens[b, k]].tolist()) == off, (b, k)
            assert abs(float(scores[b, k]) - sc) <= 1e-4 * max(1.0, abs(sc)), (b, k, float(scores[b, k]), sc)
        exact += O.decisive(res) and 0 in ranks
    assert exact >= 0.9 * B and dec >= 0.9 * B, f"{exact} exact, {dec} decisive of {B}"
    assert sum(forced) >= B and d.max_rows <= lag + every + 1 + chunk


@pytest.mark.parametrize("arm", S.ARMS)
def test_forced_cut_keeps_the_beams_that_agree(dev, lm_dir, arm):
    """The K-slot read-out after a cut is the read-out before it restricted to the beams that agree with one of them on its m pairs
    before the cut frame, order and score bits kept (on plain and char that beam is the read-out's first slot), and the stable prefix
    becomes m; a cut with m <= stable_len changes nothing."""
    B, T, C, K = 7, 24, 7, 4 if arm != "plain" else 8
    search, _ = S._arm(lm_dir, arm, C)
    probs = _probs(B, T, C, 50, 0, 4.0)
    d = Driver(dev, probs, K, 40, 1.0, search, 1)
    before = d.feed([T] * B, K)
    stable0 = before[4].tolist()
    # a cut that reaches nothing above the stable prefix: the frame after the first slot's last stable pair
    low = []
    for b in range(B):
        first = _beams(before, b)[0]
        low.append(first[1][stable0[b] - 1] + 1 if stable0[b] else 0)
    info, dropped = d.commit(1, low)
    same = d.read(K)
    assert not dropped.any() and same[4].tolist() == stable0
    for b in range(B):
        assert _beams(same, b) == _beams(before, b)
    cut = [T - 4] * B
    info, dropped = d.commit(1, cut)
    after = d.read(K)
    changed = 0
    for b in range(B):
        old, new = _beams(before, b), _beams(after, b)
        picks = []
        for r in (old[:1] if arm in ("plain", "char") else old):
            m = sum(1 for f in r[1] if f < cut[b])
            if m <= stable0[b]:
                m, keep = stable0[b], old
            else:
                keep = [x for x in old if (x[0][:m], x[1][:m]) == (r[0][:m], r[1][:m])]
            picks.append((m, keep))
        # the cut makes those m pairs stable and the commit takes them; the read-out then reports the survivors' common prefix
        assert any(new == keep and len(d.done[b][0]) == m and int(info[b, 1]) == CO.live_nodes(new, m) for m, keep in picks), (b, old, new)
        assert int(dropped[b]) == len(old) - len(new) and int(after[4][b]) == S.SO.stable_prefix(new) >= len(d.done[b][0])
        changed += len(new) < len(old)
    assert changed >= 2, changed                                                                 # (the cut did drop beams somewhere)
    d2 = Driver(dev, probs[:, :T], K, 40, 1.0, search, 1)                                        # the survivors go on as a search would
    d2.feed([T] * B, 0)
    d2.commit(1, cut)
    more = _probs(B, 6, C, 51, 0, 4.0)
    d.probs = d2.probs = torch.cat((probs, more), 1)
    a, b2 = d.feed([6] * B, K), d2.feed([6] * B, K)
    for b in range(B):
        assert _beams(a, b) == _beams(b2, b)


@pytest.mark.parametrize("commit", [False, True])
def test_finish_one_utterance_of_a_batch(dev, commit):
    """finish(1) in a batch of 3, mid-stream: decode() of utterance 1's frames so far; the frames fed to that slot afterwards decode as
    a fresh utterance; the other two end with the bits of an undisturbed stream."""
    from asr_amd.decoders import BeamCTCDecoder
    B, T, C, K = 3, 30, 7, 4
    probs = _probs(B, T, C, 61, 0, 4.0)
    dec, ref = (BeamCTCDecoder({c: i for i, c in enumerate(S.CHARS[C])}, beam_width=K) for _ in range(2))
    s = dec.open_stream(batch=B, capacity=4, commit=commit, commit_every=5 if commit else None)
    x = probs.to(dev)
    for t0 in (0, 6, 12):
        s.feed(x[:, t0:t0 + 6], partial=False)
    dec.last_scores = None
    strings, offsets, scores = s.finish(1)
    want_s, want_o = ref.decode(probs[1:2, :18])
    assert strings == want_s[0] and [o.tolist() for o in offsets] == [o.tolist() for o in want_o[0]]
    assert torch.equal(scores.view(torch.int32), ref.last_scores[0].view(torch.int32)) and dec.last_scores is None
    assert s.frames == [18, 0, 18] and not s.closed and s.committed[1] == ([], [])
    if commit:
        assert s.commits >= 2
    recs = s.feed(x[:, 18:24])
    want_s, want_o = ref.decode(probs[1:2, 18:24])
    assert recs[1]["text"] == want_s[0][0] and recs[1]["offsets"].tolist() == want_o[0][0].tolist() and recs[1]["frames"] == 6
    assert recs[1]["score"] == float(ref.last_scores[0, 0])
    s.feed(x[:, 24:], partial=False)
    got_s, got_o = s.finish()
    mixed = probs.clone()
    mixed[1, :12] = probs[1, 18:]
    want_s, want_o = ref.decode(mixed, torch.tensor([30, 12, 30]))
    assert got_s == want_s and [[o.tolist() for o in u] for u in got_o] == [[o.tolist() for o in u] for u in want_o]
    assert torch.equal(dec.last_scores.view(torch.int32), ref.last_scores.view(torch.int32))
    with pytest.raises(ValueError, match="closed"):
        s.finish(0)
    never = dec.open_stream(batch=2, commit=commit)                                              # a slot that was never fed
    assert never.finish(0)[0] == [""] * K and never.frames == [0, 0]


def test_entry_refusals_and_no_ops(dev, lm_dir):
    """the commit entry's refusals, each with a message that begins with its name and before any launch; dead and never-fed streams are
    no-ops with M = 0"""
    from asr_amd import _lib, ops
    lib = _lib.load()
    B, C, K = 2, 7, 4
    state = ops.ctc_beam_stream_state(B, K, None, None, dev)
    nodes, out = ops.ctc_beam_stream_nodes(B, 8, K, dev), ops.ctc_beam_stream_nodes(B, 16, K, dev)
    nodes.zero_(), out.fill_(-7)
    rows = torch.full((2, B, 5), -7, dtype=torch.int32, device=dev)
    info = torch.full((B, 4), -7, dtype=torch.int32, device=dev)

    def call(state_ptr=state.data_ptr(), state_bytes=state.numel(), src=nodes.data_ptr(), src_bytes=nodes.numel() * 4, cap=8, dst=out.data_ptr(),
             dst_bytes=out.numel() * 4, cap_out=16, Wc=5, lab=rows[0].data_ptr(), info_ptr=info.data_ptr(), beam=K, batch=B):
        return lib.ds2_ctc_beam_stream_commit(state_ptr, state_bytes, batch, beam, 0, 0, src, src_bytes, cap, dst, dst_bytes, cap_out, None, Wc,
                                              lab, rows[1].data_ptr(), info_ptr, None, None, 0, None)

    def refused(what, **kw):
        assert call(**kw) != 0
        msg = lib.ds2_last_error().decode()
        assert msg.startswith(ENTRY + ": ") and what in msg, msg

    refused("destination too small", cap_out=7)
    refused("destination too small", dst_bytes=12 * B * 16 * K - 1)
    refused("node buffer too small", src_bytes=12 * B * 8 * K - 1)
    refused("aliases the source", dst=nodes.data_ptr(), dst_bytes=nodes.numel() * 4, cap_out=8)
    refused("aliases the source", dst=nodes.data_ptr() + 4 * K, dst_bytes=out.numel() * 4)
    refused("null pointer", state_ptr=None)
    refused("null pointer", src=None)
    refused("null pointer", dst=None)
    refused("null pointer", info_ptr=None)
    refused("null pointer", lab=None)
    refused("state too small", state_bytes=lib.ds2_ctc_beam_stream_state_bytes(B, K, 0, 0) - 1)
    refused("bad dims", beam=lib.ds2_ctc_beam_max_width() + 1)
    refused("bad dims", Wc=-1)
    refused("bad dims", batch=0)
    refused("outside", cap=0)
    torch.cuda.synchronize()
    assert (info == -7).all() and (out == -7).all() and (rows == -7).all() and not state.any()   # nothing was launched
    assert call() == 0 and call(Wc=0, lab=None) == 0                                             # never fed: a no-op
    torch.cuda.synchronize()
    assert not info.any() and (out == -7).all() and (rows == -7).all() and not state.any()
    with pytest.raises(ValueError, match="width"):
        ops.ctc_beam_stream_commit(state, nodes, 8, out, 16, K, None, None, -1)
    x = _probs(B, 3, C, 0).to(dev)

    def feed(cap=8, rows_bound=0, labels_bound=0, W=8):                                          # the committed feed entry's own bounds
        outs = [torch.zeros((B, K, 8), dtype=torch.int32, device=dev) for _ in range(2)] + [torch.zeros((B, K), dtype=torch.int32, device=dev),
                                                                                             torch.zeros((B, K), dtype=torch.float32, device=dev)]
        tail = torch.zeros((2, B), dtype=torch.int32, device=dev)
        rc = lib.ds2_ctc_beam_stream_feed_committed_f32(x.data_ptr(), x.stride(0), x.stride(1), B, 3, C, None, 0, K, 40, 1.0, None, 0, 0, 0, -1, 0.0,
                                                        0.0, None, None, 0, state.data_ptr(), state.numel(), nodes.data_ptr(), nodes.numel() * 4,
                                                        cap, rows_bound, labels_bound, K, W, *(o.data_ptr() for o in outs), tail[0].data_ptr(),
                                                        tail[1].data_ptr(), None)
        return rc, lib.ds2_last_error().decode()
    for what, kw in (("node buffer too small", dict(rows_bound=6)), ("uncommitted labels", dict(labels_bound=6)), ("uncommitted labels", dict(W=2)),
                     ("labels_bound", dict(labels_bound=-1))):
        rc, msg = feed(**kw)
        assert rc != 0 and msg.startswith("ds2_ctc_beam_stream_feed_committed_f32: ") and what in msg, msg
    torch.cuda.synchronize()
    assert not state.any()
    assert feed(rows_bound=5, labels_bound=5)[0] == 0                                            # 5 + 3 rows and labels in 8: accepted
    state.zero_()
    # a dead stream (test_gpu_beam_stream's: a dictionary that rules out every extension) commits what was stable and keeps no node
    search, _ = S._arm(lm_dir, "word", C, words=["AB", "B"])
    seq = [1, 3, 3, 0, 1, 2]
    probs = torch.full((1, len(seq), C), 0.01)
    for t, c in enumerate(seq):
        probs[0, t, c] = 1.0 - 0.01 * (C - 1)
    d = Driver(dev, probs, K, 1, 1.0, search, 1)
    for t in range(len(seq)):
        got = d.commit(1)
        if got is not None:
            assert int(got[0][0, 1]) == (1 if t == 1 else 0)                                      # "A" alone, then nothing lives
        S._same_bits(d.feed([1], K), d.decode(), K)
    assert d.done[0] == ([1], [0]) and d.cap <= 2
    S._same_bits(d.read(K), d.decode(), K)


def test_stream_long_with_commit_yields_the_same_items(dev):
    from asr_amd.decoders import BeamCTCDecoder
    model = S.tiny_model()
    spect = torch.randn((161, 437), generator=torch.Generator().manual_seed(11))
    dec = BeamCTCDecoder(model.labels, beam_width=8)
    want = list(model.stream_long(spect, window=128, overlap=16, batch_size=2, decoder=dec))
    got = list(model.stream_long(spect, window=128, overlap=16, batch_size=2, decoder=dec, commit=True))
    assert len(got) == len(want) == 4 and got == want and got[-1]["final"]
