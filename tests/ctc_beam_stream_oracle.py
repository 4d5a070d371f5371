"""Host side of the streaming beam search's tests (ds2_ctc_beam_stream_feed_f32, csrc/ctc_beam_stream.h), written from the contract.
The stream's promise is that a read-out after any cuts is the one-call search on the frames so far, so its oracle is the one-call
oracles run on prefixes of the frames; what is new is the stable prefix: the longest run of (label, offset) pairs that every live beam
starts with."""
from __future__ import annotations

import ctc_beam_lm_oracle as LO
import ctc_beam_oracle as O


def stable_prefix(beams) -> int:
    """beams: [(labels tuple, offsets tuple, total)] as ctc_beam_oracle.beam_search and ctc_beam_lm_oracle.beam_search (with an LM
    fusion or a ctc_beam_hot_oracle.HotFusion) return them -> the length of the longest common prefix of (label, offset) pairs.
    No beam: 0 (the stream then keeps the value it had)."""
    if not beams:
        return 0
    pairs = [list(zip(b[0], b[1])) for b in beams]
    n = 0
    for column in zip(*pairs):          # stops at the shortest beam
        if any(p != column[0] for p in column):
            break
        n += 1
    return n


def search_at_cuts(probs, cuts, fusion=None, blank=0, beam_width=100, cutoff_top_n=40, cutoff_prob=1.0):
    """probs (T, C) of one utterance; cuts: frame counts t -> [the oracle's result dict on probs[:t] for every t].  fusion None: the
    plain search of ctc_beam_oracle; otherwise ctc_beam_lm_oracle's with that fusion (language model, hotwords or both)."""
    out = []
    for t in cuts:
        if fusion is None:
            out.append(O.beam_search(probs, t, blank, beam_width, cutoff_top_n, cutoff_prob))
        else:
            out.append(LO.beam_search(probs, fusion, t, blank, beam_width, cutoff_top_n, cutoff_prob))
    return out


def decisive(res, fusion=None) -> bool:
    return O.decisive(res) if fusion is None else LO.decisive(res)
