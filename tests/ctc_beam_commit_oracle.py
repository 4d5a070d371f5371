"""Host side of the tests of the streaming beam search's commit and compaction (ds2_ctc_beam_stream_commit, csrc/ctc_beam_commit.h),
written from the contract in include/ds2hip.h:
  live_nodes   how many back-pointer nodes a stream still needs, counted on a read-out;
  compact      the mark-and-renumber of a back-pointer tree in plain Python;
  ForcedSearch the plain search of ctc_beam_oracle restated frame by frame, in fp64, with the tree of nodes the kernel keeps and with
               the forced cut.  Without a cut it must give ctc_beam_oracle.beam_search's beams and totals exactly (test_cpu_beam_commit
               pins that), so what it says with a cut is the contract's rule applied to the pinned search."""
from __future__ import annotations

import math

import numpy as np

import ctc_beam_oracle as O
from ctc_beam_stream_oracle import stable_prefix

NEG = -math.inf


def live_nodes(beams, stable) -> int:
    """beams: [(labels tuple, offsets tuple, ...)] of the live beams; stable: their stable prefix's length -> the nodes of the live tree:
    the distinct (label, offset)-pair prefixes of length >= max(stable, 1) among the beams.  A node is made once per (prefix, frame),
    so two chains share a node exactly where they share the pairs up to it; the stable node itself (length `stable`) is kept."""
    seen = set()
    for b in beams:
        pairs = tuple(zip(b[0], b[1]))
        for n in range(max(int(stable), 1), len(pairs) + 1):
            seen.add(pairs[:n])
    return len(seen)


def compact(parent, label, frame, beam_nodes, stable_node):
    """parent / label / frame: a tree of nodes by id (parent -1: a first label); beam_nodes: the live beams' nodes (-1: the empty
    prefix); stable_node: the node every chain passes, or -1 -> (parent, label, frame, beam_nodes, stable_node) renumbered: only the
    nodes on the chains from the beams down to and including stable_node are kept, in the order of their ids, and stable_node's parent
    becomes -1."""
    keep = set()
    for x in beam_nodes:
        while x >= 0 and x not in keep:
            keep.add(x)
            if x == stable_node:
                break
            x = parent[x]
    order = sorted(keep)
    new = {old: i for i, old in enumerate(order)}
    new[-1] = -1
    return ([-1 if old == stable_node else new[parent[old]] for old in order], [label[old] for old in order], [frame[old] for old in order],
            [new[x] for x in beam_nodes], new[stable_node] if stable_node in keep else -1)


def chain(parent, label, frame, node):
    """the (labels, offsets) a node's chain spells, first label first"""
    labels, offs = [], []
    while node >= 0:
        labels.append(label[node])
        offs.append(frame[node])
        node = parent[node]
    return tuple(reversed(labels)), tuple(reversed(offs))


class ForcedSearch:
    """One utterance of the plain search, fed frame by frame.  beams: [(labels, offsets, total)] in the search's order; nodes: the beams'
    nodes in the tree (parent, label, frame), a node per new (prefix, frame) as the kernel makes them; stable: the length of the stable
    prefix as the stream reports it (the common (label, offset) prefix of the live beams after the last feed, kept with no live beam,
    raised by a cut).  The margins are ctc_beam_oracle's, with one more entry in frame_margins per cut that dropped a beam: the lead of
    the first slot, whose choice the cut made final."""

    def __init__(self, blank=0, beam_width=100, cutoff_top_n=40, cutoff_prob=1.0):
        self.blank, self.K, self.top_n, self.cutoff_prob = int(blank), int(beam_width), int(cutoff_top_n), float(cutoff_prob)
        self.prefixes, self.offsets, self.nodes = [()], [()], [-1]
        self.pb, self.pnb = np.array([0.0]), np.array([NEG])
        self.parent, self.label, self.frame = [], [], []
        self.t, self.stable, self.forced = 0, 0, 0
        self.frame_margins, self.cut_margin = [], math.inf

    def feed(self, probs):
        for p in np.asarray(probs, dtype=np.float64):
            if self.prefixes:
                self._frame(p)
            self.t += 1
        if self.prefixes:
            self.stable = max(self.stable, stable_prefix(self.beams))

    def _frame(self, p):
        K, blank, t = self.K, self.blank, self.t
        prefixes, offsets, nodes, pb, pnb = self.prefixes, self.offsets, self.nodes, self.pb, self.pnb
        with np.errstate(divide="ignore", invalid="ignore"):
            kept, m = O.prune(p, self.top_n, self.cutoff_prob)
            self.cut_margin = min(self.cut_margin, m)
            lp = np.log(p)
            kept = [int(c) for c in kept]
            lp_blank = lp[blank] if blank in kept else NEG
            tot = np.logaddexp(pb, pnb)
            index = {pr: i for i, pr in enumerate(prefixes)}
            ext = [c for c in kept if c != blank]
            # every candidate: [prefix, pb', pnb', offsets, source beam (an extension) or -1 (a beam that stays), node]
            stay = []
            for i, pr in enumerate(prefixes):
                rep = pnb[i] + lp[pr[-1]] if pr and pr[-1] in ext else NEG
                stay.append([pr, tot[i] + lp_blank, rep, offsets[i], -1, nodes[i]])
            cands = []
            for i, pr in enumerate(prefixes):
                for c in ext:
                    s = (pb[i] if pr and pr[-1] == c else tot[i]) + lp[c]
                    k = index.get(pr + (c,))
                    if k is not None:          # the extension is a beam already: its mass joins that beam
                        stay[k][2] = np.logaddexp(stay[k][2], s)
                    else:
                        cands.append([pr + (c,), NEG, s, offsets[i] + (t,), i, -1])
            cands = stay + cands
            for x in cands:
                x.append(float(np.logaddexp(x[1], x[2])))
        cands = [x for x in cands if x[6] > NEG]
        cands.sort(key=lambda x: (-x[6], len(x[0]), x[0]))
        self.frame_margins.append(cands[K - 1][6] - cands[K][6] if len(cands) > K else math.inf)
        cands = cands[:K]
        for x in cands:
            if x[4] >= 0:                      # a new prefix: a node
                self.parent.append(nodes[x[4]])
                self.label.append(x[0][-1])
                self.frame.append(t)
                x[5] = len(self.parent) - 1
        self.prefixes, self.offsets, self.nodes = [x[0] for x in cands], [x[3] for x in cands], [x[5] for x in cands]
        self.pb, self.pnb = np.array([float(x[1]) for x in cands]), np.array([float(x[2]) for x in cands])

    @property
    def totals(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.logaddexp(self.pb, self.pnb) if self.prefixes else np.zeros(0)

    @property
    def beams(self):
        return [(pr, off, float(s)) for pr, off, s in zip(self.prefixes, self.offsets, self.totals)]

    def cut(self, cut_frame) -> int:
        """the forced cut of the contract at frame cut_frame (< 0: none) -> the beams dropped"""
        if cut_frame < 0 or not self.prefixes:
            return 0
        m = sum(1 for f in self.offsets[0] if f < cut_frame)
        if m <= self.stable:
            return 0
        head = (self.prefixes[0][:m], self.offsets[0][:m])
        keep = [i for i in range(len(self.prefixes)) if (self.prefixes[i][:m], self.offsets[i][:m]) == head]
        dropped = len(self.prefixes) - len(keep)
        if dropped:
            tot = self.totals
            self.frame_margins.append(float(tot[0] - tot[1]))
            self.forced += 1
        self.prefixes, self.offsets, self.nodes = ([v[i] for i in keep] for v in (self.prefixes, self.offsets, self.nodes))
        self.pb, self.pnb = self.pb[keep], self.pnb[keep]
        self.stable = m
        return dropped

    def result(self):
        """what ctc_beam_oracle.beam_search returns, for the frames so far"""
        beams = self.beams
        gaps = [beams[k][2] - beams[k + 1][2] for k in range(len(beams) - 1)]
        return dict(beams=beams, frame_margins=list(self.frame_margins), final_gaps=gaps, cutoff_margin=self.cut_margin)

    def live_tree(self):
        """compact() of the tree as it is now -> its result; its first list's length is the live tree's size"""
        stable_node = -1
        if self.stable > 0 and self.nodes:
            stable_node = self.nodes[0]
            for _ in range(len(self.prefixes[0]) - self.stable):
                stable_node = self.parent[stable_node]
        return compact(self.parent, self.label, self.frame, self.nodes, stable_node)


def run(probs, chunk, max_lag=None, commit_every=None, **search):
    """One utterance's frames through ForcedSearch in chunks of `chunk`, with BeamStream's plan for the cuts: before a feed, when
    commit_every frames (default: every feed) have passed since the last commit, a cut at frame (frames so far - max_lag) (none with
    max_lag None) -> (the search, [per commit: (frames so far, live nodes after the commit)])."""
    s, commits, since = ForcedSearch(**search), [], 0
    every = chunk if commit_every is None else commit_every
    for t0 in range(0, len(probs), chunk):
        if t0 and since >= every:
            if max_lag is not None:
                s.cut(s.t - max_lag)
            commits.append((s.t, live_nodes(s.beams, s.stable) if s.prefixes else 0))
            since = 0
        s.feed(probs[t0:t0 + chunk])
        since += len(probs[t0:t0 + chunk])
    return s, commits
