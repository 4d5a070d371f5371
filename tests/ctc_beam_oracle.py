"""fp64 restatement of the CTC prefix beam search contract of `ds2_ctc_beam_decode_f32` (include/ds2hip.h), written from the
contract, not from the kernel.  Also reports how decisive each decision was, so that a test can tell where an fp32 device result
must agree exactly:
  - `frame_margins[t]`: at frame t, the gap between the K-th and the (K+1)-th candidate totals (inf when nothing was cut);
  - `final_gaps[k]`: total[k] - total[k+1] of the returned beams;
  - `cutoff_margin`: the smallest |running sum - cutoff_prob| over the class lists the cutoff walked (inf when cutoff_prob >= 1).
"""
from __future__ import annotations

import math

import numpy as np

NEG = -math.inf


def prune(p: np.ndarray, top_n: int, cutoff_prob: float):
    """Kept classes of one frame, in order (probability desc, index asc), and the cutoff decision margin."""
    C = p.shape[0]
    order = np.lexsort((np.arange(C), -p))[: min(top_n, C)]
    margin = math.inf
    if cutoff_prob < 1.0:
        cs = np.cumsum(p[order])
        hit = np.nonzero(cs >= cutoff_prob)[0]
        n = int(hit[0]) + 1 if hit.size else order.size
        order = order[:n]
        margin = float(np.min(np.abs(cs[:n] - cutoff_prob)))
    return order, margin


def _order_key(prefix, total):
    return (-total, len(prefix), prefix)


def beam_search(probs, size=None, blank=0, beam_width=100, cutoff_top_n=40, cutoff_prob=1.0):
    """probs (T, C) probabilities of one utterance -> dict(beams=[(labels tuple, offsets tuple, total)], frame_margins, final_gaps,
    cutoff_margin).  Exactly beam_width entries are NOT padded here: `beams` holds the survivors only."""
    probs = np.asarray(probs, dtype=np.float64)
    T, C = probs.shape
    n = T if size is None else max(0, min(int(size), T))
    K = int(beam_width)
    # beams: parallel lists, sorted by the contract's order
    prefixes, offsets = [()], [()]
    pb, pnb = np.array([0.0]), np.array([NEG])
    frame_margins, cut_margin = [], math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(n):
            p = probs[t]
            kept, m = prune(p, cutoff_top_n, cutoff_prob)
            cut_margin = min(cut_margin, m)
            lp_all = np.log(p)
            kept_set = set(int(c) for c in kept)
            lp_blank = lp_all[blank] if blank in kept_set else NEG
            tot = np.logaddexp(pb, pnb)
            index = {pr: i for i, pr in enumerate(prefixes)}
            nb = len(prefixes)
            last = np.array([pr[-1] if pr else -1 for pr in prefixes], dtype=np.int64)
            ext_c = np.array([c for c in kept.tolist() if c != blank], dtype=np.int64)
            lp_c = lp_all[ext_c]
            # pb'(l) from the blank; pnb'(l) from the repeat of l's last label
            spb = tot + lp_blank
            rep = (last[:, None] == ext_c[None, :])
            spnb = np.full(nb, NEG)
            for i, j in zip(*np.nonzero(rep)):
                spnb[i] = np.logaddexp(spnb[i], pnb[i] + lp_c[j])
            # l + c: pb(l) + lp when c is l's last label, total(l) + lp otherwise
            S = np.where(rep, pb[:, None] + lp_c[None, :], tot[:, None] + lp_c[None, :]) if ext_c.size else np.zeros((nb, 0))
            # an extension that is already a beam is summed into that beam
            col = {int(c): j for j, c in enumerate(ext_c.tolist())}
            for k, pr in enumerate(prefixes):
                if pr:
                    i, j = index.get(pr[:-1]), col.get(pr[-1])
                    if i is not None and j is not None:
                        spnb[k] = np.logaddexp(spnb[k], S[i, j])
                        S[i, j] = NEG
            stay = np.logaddexp(spb, spnb)
            scores = np.concatenate([stay, S.reshape(-1)])
            lens = np.concatenate([[len(pr) for pr in prefixes], np.repeat([len(pr) + 1 for pr in prefixes], ext_c.size)])
            live = np.nonzero(scores > NEG)[0]
            live = live[np.lexsort((lens[live], -scores[live]))]
            if live.size > K:   # every candidate tied with the (K+1)-th on (total, length) goes to the full ordering
                cut = live[K]
                live = live[(scores[live] > scores[cut]) | ((scores[live] == scores[cut]) & (lens[live] <= lens[cut]))]
            cands = []
            for q in live.tolist():
                if q < nb:
                    cands.append((prefixes[q], float(spb[q]), float(spnb[q]), float(stay[q]), offsets[q]))
                else:
                    i, j = divmod(q - nb, ext_c.size)
                    cands.append((prefixes[i] + (int(ext_c[j]),), NEG, float(S[i, j]), float(S[i, j]), offsets[i] + (t,)))
            cands.sort(key=lambda x: _order_key(x[0], x[3]))
            frame_margins.append(cands[K - 1][3] - cands[K][3] if len(cands) > K else math.inf)
            cands = cands[:K]
            prefixes = [x[0] for x in cands]
            pb = np.array([x[1] for x in cands])
            pnb = np.array([x[2] for x in cands])
            offsets = [x[4] for x in cands]
            if not prefixes:
                break
        tot = np.logaddexp(pb, pnb) if prefixes else np.zeros(0)
    beams = [(pr, off, float(s)) for pr, off, s in zip(prefixes, offsets, tot)]
    gaps = [beams[k][2] - beams[k + 1][2] for k in range(len(beams) - 1)]
    return dict(beams=beams, frame_margins=frame_margins, final_gaps=gaps, cutoff_margin=cut_margin)


def decisive(res, tol=1e-4) -> bool:
    """Every pruning and selection decision of the search cleared `tol` (relative to the scores' magnitude, at least 1)."""
    scale = max([1.0] + [abs(b[2]) for b in res["beams"]])
    fm = min(res["frame_margins"], default=math.inf)
    return fm > tol * scale and res["cutoff_margin"] > tol


def decisive_ranks(res, tol=1e-4):
    """Ranks k whose position is decided: the gaps to both neighbours exceed tol (relative, at least 1)."""
    beams, gaps = res["beams"], res["final_gaps"]
    out = []
    for k in range(len(beams)):
        scale = max(1.0, abs(beams[k][2]))
        if (k == 0 or gaps[k - 1] > tol * scale) and (k == len(beams) - 1 or gaps[k] > tol * scale):
            out.append(k)
    return out


def brute_force_label_logprobs(probs, blank=0):
    """log P(labeling) for every labeling reachable from (T, C) probs, by enumerating all C**T alignments (tiny T, C only)."""
    probs = np.asarray(probs, dtype=np.float64)
    T, C = probs.shape
    acc = {}
    for path in np.ndindex(*([C] * T)):
        pr = float(np.prod([probs[t, c] for t, c in enumerate(path)]))
        if pr == 0.0:
            continue
        lab, prev = [], None
        for c in path:
            if c != blank and c != prev:
                lab.append(c)
            prev = c
        acc[tuple(lab)] = acc.get(tuple(lab), 0.0) + pr
    return {k: math.log(v) for k, v in acc.items()}
