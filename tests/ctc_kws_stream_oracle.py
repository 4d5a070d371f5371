"""NumPy restatement of the streaming keyword-search contract of `ds2_ctc_kws_stream_feed_f32` (include/ds2hip.h), written from that
text — TEST ORACLE, not the product.  One `KwsStream` is one (utterance, keyword).  The frames come from `ctc_kws_oracle.kws_lattice`
on the whole utterance, computed once: the lattice is causal (row t depends on the rows up to t only), so its first n rows are the
lattice of the first n frames, and a feed reads the rows of its own frames.  What is kept from feed to feed is what the contract
keeps: the frames consumed, the tail, the pending list, the two counters."""
import numpy as np

import ctc_kws_oracle as K

NEG = -np.inf


def pick_two_pass(pend, c, max_hits):
    """Step 5 on a pending list [(t, start, score)] ascending in t: the greedy rule on the candidates with t < c (final), then on the
    rest (tentative), into the same max_hits slots -> ([(start, end, score, final)], n_hits)."""
    hits, n = [], 0
    for final in (1, 0):
        live = [p for p in pend if (p[0] < c) == bool(final)]
        while live:
            if n == max_hits:
                return hits, max_hits + 1
            t, s, v = max(live, key=lambda p: (p[2], -p[0]))     # the largest score, a tie to the smallest t
            hits.append((s, t + 1, v, final))
            n += 1
            live = [p for p in live if not (p[1] <= t and s <= p[0])]
    return hits, n


class KwsStream:
    def __init__(self, e, labels, thr, max_hits, pending=1024, max_lag=None):
        """e (T, C) log emissions of the WHOLE utterance (float32), of which feed() consumes the next rows; thr: the keyword's threshold"""
        self.e = np.asarray(e)
        self.lat = K.kws_lattice(self.e, labels)                # None: a keyword without a lattice has no candidate
        self.thr, self.max_hits, self.pending = self.e.dtype.type(thr), int(max_hits), int(pending)
        self.max_lag = -1 if max_lag is None else int(max_lag)
        self.n = self.tail = self.forced = self.dropped = 0
        self.pend = []

    def feed(self, frames, finish=False):
        """The next `frames` rows, then steps 2 to 6 -> {"frame_score", "frame_start" (frames each), "hits": [(start, end, score,
        final)] in order of acceptance, "n_hits", "tail", "frames", "forced", "dropped"}"""
        n0, n = self.n, self.n + int(frames)
        assert n <= self.e.shape[0]
        fs, fst = np.full(n - n0, NEG, self.e.dtype), np.full(n - n0, -1, np.int32)
        if self.lat is not None:
            fs[:], fst[:] = self.lat[0][n0:n, -1], self.lat[1][n0:n, -1]
        for i in range(n - n0):                                  # 2. intake
            if np.isfinite(fs[i]) and fs[i] >= self.thr:
                if fst[i] < self.tail or len(self.pend) >= self.pending:
                    self.dropped += 1
                else:
                    self.pend.append((n0 + i, int(fst[i]), fs[i]))
        h = n                                                    # 3. horizon
        if self.lat is not None and n > 0:
            v, s = self.lat[0][n - 1], self.lat[1][n - 1]
            alive = np.isfinite(v) & (v >= self.thr)
            if alive.any():
                h = min(n, int(s[alive].min()))
        if finish:                                               # 4. settle
            c = n
        else:
            c = max(self.tail, h)
            while any(s < c <= t for t, s, _ in self.pend):
                c = min(s for t, s, _ in self.pend if s < c <= t)
            assert c >= self.tail
        if self.max_lag >= 0 and n - c > self.max_lag:
            c = n - self.max_lag
            self.forced += 1
            keep = [p for p in self.pend if not (p[1] < c <= p[0])]
            self.dropped += len(self.pend) - len(keep)
            self.pend = keep
        hits, n_hits = pick_two_pass(self.pend, c, self.max_hits)   # 5. pick
        self.pend = [p for p in self.pend if p[0] >= c]             # 6.
        self.n, self.tail = n, c
        return dict(frame_score=fs, frame_start=fst, hits=hits, n_hits=n_hits, tail=c, frames=n, forced=self.forced, dropped=self.dropped)
