"""Greedy and beam CTC decoders + WER/CER (host-side mirror of asr_deepspeech/decoders/{decoder,greedy_decoder,beam_decoder}.py).
`decode()` runs on the GPU (csrc/decode.hip, csrc/ctc_beam.h); process_string / convert_to_strings are the host utilities the
reference uses for TARGET strings.  Eval-only, not on the train step.
`wer` / `cer` keep a small pure-Python DP (the reference imports the `Levenshtein` C package) as the reference API; evaluate()
scores a whole batch with `Decoder.score_batch`, one HIP launch (csrc/edit_distance.h) on ids packed by `pack_scoring`.
`CTCAligner.align` places a KNOWN transcript in time (csrc/ctc_align.h); its record assembly is the pure host function
`assemble_alignments`.  `KeywordSpotter.search` finds WHERE keywords were said without a decode or a transcript (csrc/ctc_kws.h); its
record assembly is `assemble_detections`.  `transcribe_posteriors` turns ONE long recording's posteriors into timed segments: cut at
pauses and packed into decode batches on the GPU (csrc/ctc_segment.h); its host half is `plan_segment_batches`, `words_from_offsets`
and `assemble_transcript`.  `CTCConfidence.score` says HOW SURE a text is of each word or character, as a conditional probability
(csrc/ctc_conf.h); its host half is `confidence_units`.  `Decoder.align_batch` says WHICH words and characters are wrong: the edit
alignment behind the distances (csrc/edit_align.h); its host half is `assemble_edit_alignments`, `ErrorReport` adds the records up and
`reliability` bins confidences against their right / wrong flags.  `NBestRescorer` re-ranks a beam search's n-best list under any LM
weights, or a larger LM, from per-hypothesis features (csrc/lm_score.h) and `tune_lm_weights` sweeps an (alpha, beta) grid over
them after ONE decode; its host half is `tune_summary`."""
from __future__ import annotations

import math

import numpy as np
import torch


def _edit_distance(a, b) -> int:
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def pack_scoring(hypotheses, references):
    """Host half of Decoder.score_batch: the B (hypothesis, reference) string pairs as 2B edit-distance problems over int32 ids, in
    O(length).  Problem b < B is pair b's word problem, whose words are `s.split()` mapped to ids by a per-pair dict (two words share
    an id exactly when they are equal, as in `wer`); problem B + b is its character problem, over the code points of
    `s.replace(" ", "")` (only U+0020 is removed, as in `cer`).  Side a is the hypothesis, side b the reference.
    Returns (seq int32, a_off int64, a_len int32, b_off int64, b_len int32, ref_words int64, ref_chars int64), numpy arrays."""
    if len(hypotheses) != len(references):
        raise ValueError(f"{len(hypotheses)} hypotheses for {len(references)} references")
    B = len(hypotheses)
    pieces, ref_w, ref_c = [None] * (4 * B), np.empty(B, np.int64), np.empty(B, np.int64)
    for b, (h, r) in enumerate(zip(hypotheses, references)):
        ids = {}
        hw = [ids.setdefault(w, len(ids)) for w in h.split()]
        rw = [ids.setdefault(w, len(ids)) for w in r.split()]
        pieces[2 * b], pieces[2 * b + 1] = np.array(hw, np.int32), np.array(rw, np.int32)
        hc, rc = (np.frombuffer(x.replace(" ", "").encode("utf-32-le", "surrogatepass"), np.uint32).view(np.int32) for x in (h, r))
        pieces[2 * B + 2 * b], pieces[2 * B + 2 * b + 1] = hc, rc
        ref_w[b], ref_c[b] = len(rw), len(rc)
    lens = np.fromiter((len(x) for x in pieces), np.int64, count=4 * B)
    offs = np.zeros(4 * B, np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    seq = np.concatenate(pieces) if B else np.zeros(0, np.int32)
    return seq, offs[0::2].copy(), lens[0::2].astype(np.int32), offs[1::2].copy(), lens[1::2].astype(np.int32), ref_w, ref_c


def _upload_scoring(dev, seq, a_off, a_len, b_off, b_len):
    """pack_scoring's arrays on the device, as ops.edit_distance / ops.edit_align take them: one pinned int32 image (a_off, b_off as
    int64, 8-byte aligned at the front, then a_len, b_len, the symbols), one asynchronous copy -> (seq, a_off, a_len, b_off, b_len)."""
    P = len(a_len)
    host = torch.empty(6 * P + len(seq), dtype=torch.int32, pin_memory=True)
    h = host.numpy()
    h[:2 * P], h[2 * P:4 * P] = a_off.view(np.int32), b_off.view(np.int32)
    h[4 * P:5 * P], h[5 * P:6 * P], h[6 * P:] = a_len, b_len, seq
    d = host.to(dev, non_blocking=True)
    return d[6 * P:], d[:2 * P].view(torch.int64), d[4 * P:5 * P], d[2 * P:4 * P].view(torch.int64), d[5 * P:6 * P]


def _check_align_unit(unit):
    if unit not in ("word", "char", "both"):
        raise ValueError(f"unit must be 'word', 'char' or 'both', got {unit!r}")


def _edit_ops(hyp, ref, a_map, b_map):
    """The path in forward order from the two maps: every unpaired token in front of the next pair.  (Between two pairs an optimal
    path leaves tokens of one side only unpaired: one of each would be a cheaper substitution.)"""
    ops, i, j = [], 0, 0
    m, n = len(hyp), len(ref)
    while i < m or j < n:
        if j < n and int(b_map[j]) < 0:
            ops.append(("del", None, ref[j], None, j))
            j += 1
        elif i < m and int(a_map[i]) < 0:
            ops.append(("ins", hyp[i], None, i, None))
            i += 1
        else:
            if not (i < m and j < n and int(a_map[i]) == j and int(b_map[j]) == i):
                raise ValueError(f"assemble_edit_alignments: the maps do not describe one path (hypothesis token {i}, reference token {j})")
            ops.append(("hit" if hyp[i] == ref[j] else "sub", hyp[i], ref[j], i, j))
            i, j = i + 1, j + 1
    return ops


def assemble_edit_alignments(hypotheses, references, counts, a_map, b_map, unit="both"):
    """Pure host half of Decoder.align_batch: the strings + ops.edit_align's arrays on pack_scoring's 2B problems (problem b: pair b's
    words, problem B + b: its characters; counts (2B,4), a_map / b_map (2B,max_len)) -> one record per pair, {"words": {...}, "chars":
    {...}} cut to `unit`.  A unit holds "hits", "substitutions", "deletions", "insertions", "distance" (their last three summed),
    "ref_len", "ops": the path in forward order as (op, hyp_token | None, ref_token | None, hyp_index | None, ref_index | None) with op
    one of "hit" / "sub" / "del" / "ins", and "hyp_correct": one bool per hypothesis token, True for a hit.  Tokens are `s.split()` and
    the code points of `s.replace(" ", "")`, as in wer / cer."""
    _check_align_unit(unit)
    if len(hypotheses) != len(references):
        raise ValueError(f"{len(hypotheses)} hypotheses for {len(references)} references")
    B = len(hypotheses)
    counts, a_map, b_map = np.asarray(counts), np.asarray(a_map), np.asarray(b_map)
    if counts.shape != (2 * B, 4) or a_map.shape[0] != 2 * B or b_map.shape[0] != 2 * B:
        raise ValueError(f"assemble_edit_alignments: arrays of {counts.shape} / {a_map.shape} / {b_map.shape} for {B} pairs")
    records = []
    for b, (h, r) in enumerate(zip(hypotheses, references)):
        rec = {}
        for key, p, hyp, ref in (("words", b, h.split(), r.split()), ("chars", B + b, list(h.replace(" ", "")), list(r.replace(" ", "")))):
            if unit != "both" and not key.startswith(unit):
                continue
            hits, subs, dels, ins = (int(v) for v in counts[p])
            path = _edit_ops(hyp, ref, a_map[p], b_map[p])
            if [sum(o[0] == k for o in path) for k in ("hit", "sub", "del", "ins")] != [hits, subs, dels, ins]:
                raise ValueError(f"assemble_edit_alignments: the counts of pair {b} ({key}) do not match its maps")
            correct = [False] * len(hyp)
            for o in path:
                if o[0] == "hit":
                    correct[o[3]] = True
            rec[key] = {"hits": hits, "substitutions": subs, "deletions": dels, "insertions": ins, "distance": subs + dels + ins,
                        "ref_len": len(ref), "ops": path, "hyp_correct": correct}
        records.append(rec)
    return records


class ErrorReport:
    """The error breakdown over an evaluation: feed it Decoder.align_batch's records batch by batch (`add`), read `summary()` or the text
    block `format()`.  Host code only.  `top`: how many of the most frequent substitution pairs, deleted tokens and inserted tokens
    are listed; equal counts are ordered by token, so the output is deterministic."""

    def __init__(self, top=20):
        if isinstance(top, bool) or int(top) != top or int(top) < 0:
            raise ValueError(f"ErrorReport: top must be an integer >= 0, got {top!r}")
        self.top = int(top)
        self.units = {}

    def add(self, records):
        for rec in records:
            for key, u in rec.items():
                t = self.units.setdefault(key, {"hits": 0, "substitutions": 0, "deletions": 0, "insertions": 0, "ref_len": 0,
                                                "sub": {}, "del": {}, "ins": {}})
                for k in ("hits", "substitutions", "deletions", "insertions", "ref_len"):
                    t[k] += u[k]
                for op, hyp, ref, _, _ in u["ops"]:
                    if op != "hit":
                        tok = (ref, hyp) if op == "sub" else ref if op == "del" else hyp
                        t[op][tok] = t[op].get(tok, 0) + 1
        return self

    def summary(self):
        """Per unit fed so far ("words", "chars"): the four totals, "ref_len", "rate" = (S + D + I) / ref_len and the three partial
        rates (a ref_len of 0 divides as 1, as in evaluate()), "top_substitutions" [(ref, hyp, count)], "top_deletions" and
        "top_insertions" [(token, count)]."""
        out = {}
        for key in sorted(self.units, reverse=True):      # words before chars
            t = self.units[key]
            n = max(t["ref_len"], 1)
            s, d, i = t["substitutions"], t["deletions"], t["insertions"]
            first = lambda table: sorted(table.items(), key=lambda kv: (-kv[1], kv[0]))[:self.top]   # noqa: E731
            out[key] = {"hits": t["hits"], "substitutions": s, "deletions": d, "insertions": i, "ref_len": t["ref_len"],
                        "rate": (s + d + i) / n, "substitution_rate": s / n, "deletion_rate": d / n, "insertion_rate": i / n,
                        "top_substitutions": [(ref, hyp, c) for (ref, hyp), c in first(t["sub"])],
                        "top_deletions": first(t["del"]), "top_insertions": first(t["ins"])}
        return out

    def format(self):
        lines = []
        for key, u in self.summary().items():
            lines += [f"----- ERRORS: {key} -----",
                      f"rate {100 * u['rate']:.2f} = substitutions {100 * u['substitution_rate']:.2f} + deletions {100 * u['deletion_rate']:.2f}"
                      f" + insertions {100 * u['insertion_rate']:.2f}",
                      f"hits {u['hits']}  substitutions {u['substitutions']}  deletions {u['deletions']}  insertions {u['insertions']}"
                      f"  reference {key} {u['ref_len']}"]
            if u["top_substitutions"]:
                lines += ["substitutions (reference -> hypothesis):"] + [f"{c:>7}  {ref!r} -> {hyp!r}" for ref, hyp, c in u["top_substitutions"]]
            for name in ("deletions", "insertions"):
                if u["top_" + name]:
                    lines += [name + ":"] + [f"{c:>7}  {tok!r}" for tok, c in u["top_" + name]]
        return "\n".join(lines) + ("\n" if lines else "")


def reliability(confidences, correct, bins=10):
    """A reliability table: do the tokens with confidence near c turn out right a fraction c of the time?  confidences: floats in
    [0, 1] (e.g. DeepSpeech.confidence's), correct: one bool each (e.g. align_batch's "hyp_correct").  `bins` equal-width bins over
    [0, 1], the last one closed at 1.  Returns {"bins": [(lo, hi, count, mean_conf, accuracy)] (NaN for an empty bin), "ece": the
    expected calibration error sum_k count_k / N * |accuracy_k - mean_conf_k| (NaN without a token), "skipped": how many NaN
    confidences (units that were not scored) were dropped}."""
    if isinstance(bins, bool) or int(bins) != bins or int(bins) < 1:
        raise ValueError(f"reliability: bins must be a positive integer, got {bins!r}")
    bins = int(bins)
    conf = np.asarray(list(confidences), np.float64).reshape(-1)
    right = np.asarray(list(correct), bool).reshape(-1)
    if conf.shape != right.shape:
        raise ValueError(f"reliability: {conf.size} confidences for {right.size} flags")
    keep = ~np.isnan(conf)
    skipped = int(conf.size - keep.sum())
    conf, right = conf[keep], right[keep]
    if conf.size and (conf.min() < 0.0 or conf.max() > 1.0):
        raise ValueError("reliability: a confidence lies outside [0, 1]")
    which = np.minimum((conf * bins).astype(np.int64), bins - 1)
    rows, ece = [], 0.0
    for k in range(bins):
        sel = which == k
        cnt = int(sel.sum())
        mean, acc = (float(conf[sel].mean()), float(right[sel].mean())) if cnt else (float("nan"), float("nan"))
        rows.append((k / bins, (k + 1) / bins, cnt, mean, acc))
        if cnt:
            ece += cnt / conf.size * abs(acc - mean)
    return {"bins": rows, "ece": ece if conf.size else float("nan"), "skipped": skipped}


class Decoder:
    """decoder.py:4-72: labels is {char: index}; index 0 is the CTC blank."""

    def __init__(self, labels, blank_index=0):
        self.labels = labels
        self.int_to_char = dict((i, c) for c, i in labels.items()) if isinstance(labels, dict) else dict(enumerate(labels))
        self.blank_index = blank_index
        space_index = len(self.int_to_char)
        if isinstance(labels, dict) and " " in labels:
            space_index = labels[" "]
        self.space_index = space_index

    def wer(self, s1, s2):
        b = set(s1.split() + s2.split())
        word2char = dict(zip(b, range(len(b))))
        w1 = [chr(word2char[w]) for w in s1.split()]
        w2 = [chr(word2char[w]) for w in s2.split()]
        return _edit_distance(w1, w2)

    def cer(self, s1, s2):
        s1, s2 = s1.replace(" ", ""), s2.replace(" ", "")
        return _edit_distance(s1, s2)

    def score_batch(self, hypotheses, references):
        """The `wer` and `cer` of B (hypothesis, reference) pairs in one HIP launch -> CPU int64 tensor (B, 4) of (word distance,
        reference words, char distance, reference chars), every entry equal to wer(h, r), len(r.split()), cer(h, r),
        len(r.replace(" ", "")).  One pinned host-to-device copy of the packed ids (pack_scoring), one launch
        (ops.edit_distance), one device-to-host copy.  There is no CPU implementation: without a GPU this raises."""
        from .. import ops
        dev = _device("Decoder.score_batch", "")
        seq, a_off, a_len, b_off, b_len, ref_w, ref_c = pack_scoring(hypotheses, references)
        B = len(ref_w)
        out = torch.empty((B, 4), dtype=torch.int64)
        if B == 0:
            return out
        max_len = int(max(a_len.max(), b_len.max()))
        dist = ops.edit_distance(*_upload_scoring(dev, seq, a_off, a_len, b_off, b_len), max_len=max_len).cpu().long()
        if int(dist.min()) < 0:
            raise RuntimeError("Decoder.score_batch: the edit-distance kernel rejected a problem")
        out[:, 0], out[:, 2] = dist[:B], dist[B:]
        out[:, 1], out[:, 3] = torch.from_numpy(ref_w), torch.from_numpy(ref_c)
        return out

    def align_batch(self, hypotheses, references, unit="both"):
        """WHICH words and characters of B (hypothesis, reference) pairs are right: the edit alignment behind score_batch's distances,
        in one HIP launch -> one record per pair, {"words": {...}, "chars": {...}} cut to `unit` ("word", "char" or "both"); the unit
        records are assemble_edit_alignments'.  One pinned host-to-device copy of the packed ids (pack_scoring), one launch
        (ops.edit_align), one device-to-host copy.  The tie rule among equally cheap alignments is ds2_edit_align_i32's
        (include/ds2hip.h).  There is no CPU implementation: without a GPU this raises."""
        from .. import ops
        _check_align_unit(unit)
        dev = _device("Decoder.align_batch", "")
        seq, a_off, a_len, b_off, b_len, ref_w, _ = pack_scoring(hypotheses, references)
        B, P = len(ref_w), 2 * len(ref_w)
        if B == 0:
            return []
        max_len = int(max(a_len.max(), b_len.max()))
        counts, a_map, b_map = ops.edit_align(*_upload_scoring(dev, seq, a_off, a_len, b_off, b_len), max_len=max_len)
        out = torch.cat((counts.reshape(-1), a_map.reshape(-1), b_map.reshape(-1))).cpu().numpy()
        n = P * max_len
        counts_h, a_map_h, b_map_h = out[:4 * P].reshape(P, 4), out[4 * P:4 * P + n].reshape(P, max_len), out[4 * P + n:].reshape(P, max_len)
        if int(counts_h.min()) < 0:
            raise RuntimeError("Decoder.align_batch: the edit-alignment kernel rejected a problem")
        return assemble_edit_alignments(hypotheses, references, counts_h, a_map_h, b_map_h, unit)

    def decode(self, probs, sizes=None):
        raise NotImplementedError


class GreedyDecoder(Decoder):
    """greedy_decoder.py:6-68: per-frame argmax, collapse repeats, drop blanks."""

    def convert_to_strings(self, sequences, sizes=None, remove_repetitions=False, return_offsets=False):
        """Restates the reference's loop (greedy_decoder.py:12-26) statement for statement: same signature, same nested-list results — the
        evaluation loop and the reference's tests index them as `out[i][0]`."""
        strings, offsets = [], []
        for x in range(len(sequences)):
            seq_len = sizes[x] if sizes is not None else len(sequences[x])
            string, string_offsets = self.process_string(sequences[x], seq_len, remove_repetitions)
            strings.append([string])
            if return_offsets:
                offsets.append([string_offsets])
        return (strings, offsets) if return_offsets else strings

    def process_string(self, sequence, size, remove_repetitions=False):
        string, offsets = "", []
        seq = [int(v) for v in (sequence.tolist() if torch.is_tensor(sequence) else sequence)][: int(size)]
        for i, idx in enumerate(seq):
            char = self.int_to_char.get(idx, "")
            if idx != self.blank_index:
                if remove_repetitions and i != 0 and idx == seq[i - 1]:
                    continue
                string += " " if idx == self.space_index else char
                offsets.append(i)
        return string, torch.tensor(offsets, dtype=torch.int)

    def decode(self, probs, sizes=None):
        """probs (B,T,C) -> ([[str]], [[offsets]]) (greedy_decoder.py:48-68).

        Arg-max, repeat collapse and blank removal run as two HIP kernels (`ds2_greedy_decode_f32`); the host does
        ONE device->host copy of the compacted ids and maps them to characters.  Host tensors are uploaded first —
        there is no CPU implementation of decode()."""
        from .. import ops
        probs = torch.as_tensor(probs)
        if not probs.is_cuda:
            probs = probs.to(_device())
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        if sizes is not None:
            sizes = torch.as_tensor(sizes)
        ids, offs, lens = ops.greedy_decode(probs, sizes, self.blank_index)
        B, T = ids.shape
        host = torch.cat((ids.reshape(-1), offs.reshape(-1), lens)).cpu()
        if ops.rnn_poison_seen(ids.device):
            # the copy above synchronised with the stream: if the forward that produced `probs` was poisoned (a persistent recurrence
            # launch starved: NaN logits -> empty transcripts), say so here instead of returning garbage silently
            ops.rnn_persistent_check(ids.device)
        ids_h, offs_h, lens_h = host[:B * T].view(B, T), host[B * T:2 * B * T].view(B, T), host[2 * B * T:].tolist()
        strings, offsets = [], []
        for b in range(B):
            n = lens_h[b]
            strings.append(["".join(" " if i == self.space_index else self.int_to_char.get(i, "") for i in ids_h[b, :n].tolist())])
            offsets.append([offs_h[b, :n].clone()])
        return strings, offsets


class BeamCTCDecoder(Decoder):
    """beam_decoder.py: the reference's constructor and decode(), without its external `ctcdecode` dependency.  The prefix beam search
    runs as one HIP kernel (`ds2_ctc_beam_decode_f32`, contract in include/ds2hip.h).  `num_processes` is accepted and unused.

    With `lm_path` (an ARPA n-gram model, plain or .gz, loaded here as ctcdecode loads its scorer) the kernel fuses
    alpha * log10 lm(token | context) + beta per scored token (`ds2_ctc_beam_decode_lm_f32`): a model whose vocabulary is single
    characters scores every label (character mode, e.g. for JSUT's unspaced transcripts); otherwise it scores words between spaces
    and keeps only prefixes spelling dictionary words (word mode, which needs a space label).  KenLM binary files raise
    NotImplementedError.  With an LM, beam_width * (min(cutoff_top_n, C - 1) + 2) must stay within 4096.  ctcdecode's min_cutoff
    heuristic and approx_ctc score are not reproduced: `last_scores` are the fused totals, and parity with ctcdecode is not pinned.

    With `hotwords` (phrases as decoders.hotwords.Hotwords takes them: `str`, `(str, weight)` or label-id sequences, or a Hotwords
    object) the search prefers prefixes that spell those phrases (`ds2_ctc_beam_decode_hot_f32`), with or without an LM:
    `hotword_weight` (natural log, per label, >= 0) is the weight of a phrase given without one.  A broken partial match gives its
    lead back, a phrase that is a proper prefix of another is refused, matching knows no word boundary, and the candidate limit
    above applies without an LM too.  `set_hotwords` changes the list between calls.  Which weight serves real recordings has not
    been measured, and parity with pyctcdecode, WeNet or icefall biasing is not pinned."""

    def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100, num_processes=4,
                 blank_index=0, hotwords=None, hotword_weight=1.0):
        super().__init__(labels, blank_index)
        self.lm_path, self.alpha, self.beta, self.num_processes = lm_path, alpha, beta, num_processes
        self.cutoff_top_n, self.cutoff_prob, self.beam_width = int(cutoff_top_n), float(cutoff_prob), int(beam_width)
        self.last_scores = None
        self.lm = None
        if lm_path is not None:
            from .lm import NgramLM
            self.lm = NgramLM(lm_path, self.int_to_char, self.blank_index, self._space_label())
        self.hotwords, self.hotword_weight = None, hotword_weight
        self.set_hotwords(hotwords)

    def _space_label(self):
        """the id of the space label, None when the labels have none"""
        return self.space_index if self.int_to_char.get(self.space_index) == " " else next(
            (i for i, c in sorted(self.int_to_char.items()) if c == " "), None)

    def fit_lm(self, sentences, order=3, mode=None, path=None, alpha=None, beta=None, device=None, prune=None, min_count=None):
        """Estimate an n-gram model from `sentences` (strings spelt with this decoder's labels), write it as an ARPA file and load it as
        this decoder's language model, as `lm_path=` would: -> the lm_train.NgramEstimate.  mode: "word" or "char"; by default "word"
        when the labels have a space and "char" when they have none.  A character model covers the labels only (other characters are
        dropped) and spells the space as U+2581.  path: where the file is kept (.gz compresses); by default a temporary file that is
        removed once loaded.  alpha / beta, when given, replace the decoder's weights; device as estimate_ngram takes it.  prune (an
        entropy threshold) and min_count (count cuts per order) shrink the model before it is written: NgramEstimate.prune, whose
        perplexity() on held-out text is how to choose them.  Which order, threshold and weights serve real recordings is unmeasured:
        tune_decoder / tune_lm_weights find the weights."""
        import os
        import tempfile
        from .lm import NgramLM
        from .lm_train import estimate_ngram
        space = self._space_label()
        mode = ("word" if space is not None else "char") if mode is None else mode
        labels = [c for i, c in sorted(self.int_to_char.items()) if i != self.blank_index]
        est = estimate_ngram(sentences, order=order, mode=mode, labels=labels if mode == "char" else None, device=device, prune=prune,
                             min_count=min_count)
        if path is None:
            with tempfile.TemporaryDirectory() as d:
                lm = NgramLM(est.write_arpa(os.path.join(d, "fit_lm.arpa")), self.int_to_char, self.blank_index, space)
            lm.path = None
        else:
            lm = NgramLM(est.write_arpa(path), self.int_to_char, self.blank_index, space)
        self.lm, self.lm_path = lm, path
        if alpha is not None:
            self.alpha = alpha
        if beta is not None:
            self.beta = beta
        return est

    def set_hotwords(self, hotwords, hotword_weight=None):
        """Replace the hotword list (None or an empty list: no hotwords); hotword_weight, when given, becomes the default weight."""
        from .hotwords import Hotwords
        if hotword_weight is not None:
            self.hotword_weight = hotword_weight
        if hotwords is None or isinstance(hotwords, Hotwords):
            self.hotwords = hotwords
            return
        hotwords = [hotwords] if isinstance(hotwords, str) else list(hotwords)
        if not hotwords:
            self.hotwords = None
            return
        chars = {c: i for i, c in self.int_to_char.items()}
        space = self.space_index if self.int_to_char.get(self.space_index) == " " else None
        self.hotwords = Hotwords(hotwords, chars, self.blank_index, self.hotword_weight, space_index=space)

    def _char(self, i):
        return " " if i == self.space_index else self.int_to_char.get(i, "")

    def convert_to_strings(self, out, seq_len):
        """beam_decoder.py: out[b][k] label ids, seq_len[b][k] their lengths -> strings[b][k]."""
        return [["".join(self._char(int(i)) for i in (utt[:int(seq_len[b][k])].tolist() if torch.is_tensor(utt) else utt[:int(seq_len[b][k])]))
                 for k, utt in enumerate(batch)] for b, batch in enumerate(out)]

    def convert_tensor(self, offsets, sizes):
        """beam_decoder.py: offsets[b][k] cut to sizes[b][k] (an empty int tensor for an empty beam)."""
        return [[torch.as_tensor(utt[:int(sizes[b][k])], dtype=torch.int) for k, utt in enumerate(batch)] for b, batch in enumerate(offsets)]

    def decode(self, probs, sizes=None):
        """probs (B,T,C) probabilities -> (strings[b][k], offsets[b][k]), best beam first, beam_width entries per utterance
        (an empty string past the surviving beams).  One device->host copy; the beams' log-probabilities stay in
        `last_scores` (B, beam_width) on the host.  Host tensors are uploaded first: there is no CPU implementation."""
        from .. import ops
        probs = torch.as_tensor(probs)
        if not probs.is_cuda:
            probs = probs.to(_device("BeamCTCDecoder"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        if sizes is not None:
            sizes = torch.as_tensor(sizes)
        labels, offs, lens, scores = ops.ctc_beam_decode(probs, sizes, self.blank_index, self.beam_width, self.cutoff_top_n,
                                                         self.cutoff_prob, self.lm, self.alpha, self.beta, self.hotwords)
        B, K, T = labels.shape
        host = torch.cat((labels.reshape(-1), offs.reshape(-1), lens.reshape(-1), scores.view(torch.int32).reshape(-1))).cpu()
        if ops.rnn_poison_seen(labels.device):
            # as in GreedyDecoder.decode: a poisoned forward (a starved persistent recurrence launch) raises here
            ops.rnn_persistent_check(labels.device)
        n = B * K * T
        labels_h, offs_h = host[:n].view(B, K, T), host[n:2 * n].view(B, K, T)
        lens_h = host[2 * n:2 * n + B * K].view(B, K)
        self.last_scores = host[2 * n + B * K:].view(torch.float32).view(B, K).clone()
        return self.convert_to_strings(labels_h, lens_h), self.convert_tensor(offs_h, lens_h)

    def open_stream(self, batch=1, nbest=1, capacity=256, commit=False, commit_every=None, max_lag=None):
        """A BeamStream over `batch` utterances that are fed chunk by chunk (see there).  The stream keeps the settings the decoder has
        now: width, cut-offs, language model, alpha / beta, hotwords; changing them on the decoder later leaves an open stream as it
        is.  nbest: how many hypotheses a partial result lists (at most beam_width).  capacity: the frames (with commit: the rows of
        beam_width nodes) the back-pointer storage holds at first; it doubles when a feed needs more.  commit=True: the stream commits
        its stable prefix to the host and compacts its back-pointers to the live tree, before a feed that does not fit and every
        commit_every frames (default: capacity); results keep decode()'s bits.  max_lag (frames; needs commit=True): at a commit, the
        best hypothesis decides the text older than max_lag frames (a forced cut: the one place a stream may differ from decode())."""
        return BeamStream(self, batch, nbest, capacity, commit, commit_every, max_lag)


def stream_capacity(capacity, need):
    """The growth plan of BeamStream's node storage: the capacity (>= 1 frame) doubled until it holds `need` frames."""
    capacity = max(int(capacity), 1)
    while capacity < int(need):
        capacity *= 2
    return capacity


def commit_due(capacity, rows, chunk, since, commit_every):
    """BeamStream's commit plan, first half: a committing stream whose storage holds `capacity` rows, of which at most `rows` are in
    use, commits before a feed of `chunk` frames when the chunk does not fit, or when `since` >= commit_every frames were fed since the
    last commit."""
    return int(rows) + int(chunk) > int(capacity) or int(since) >= int(commit_every)


def commit_capacity(capacity, live_nodes, beam_width, chunk):
    """BeamStream's commit plan, second half: after a commit that left live_nodes[b] nodes per utterance -> (rows in use: the fullest
    utterance's ceil(M / beam_width), the capacity in rows that holds them and the next `chunk` frames, by stream_capacity's doubling)."""
    K = int(beam_width)
    rows = max((int(m) + K - 1) // K for m in live_nodes)
    return rows, stream_capacity(capacity, rows + int(chunk))


class BeamStream:
    """A running beam search over `batch` utterances (BeamCTCDecoder.open_stream): feed() consumes posteriors chunk by chunk and
    returns the best text so far and how much of it is final; finish() returns what BeamCTCDecoder.decode() returns for the
    concatenated frames, with the same bits, whatever the cuts.  The search's state (the beams of the kernel, with the language model's
    and the hotwords' per-beam state) lives on the device between calls (`ds2_ctc_beam_stream_feed_f32`, contract in
    include/ds2hip.h), and so do the back-pointers: 12 * beam_width bytes per frame and utterance (216 MB for an hour at width 100), in
    storage that doubles when a feed needs more.  Without commit=True nothing compacts them, and a partial result copies nbest rows
    of the stream's length to the host, so the partials of a long stream cost more as it grows; feed(..., partial=False) copies nothing.

    commit=True bounds both by what is still undecided.  Before a feed whose chunk does not fit the storage, and at the latest
    every commit_every frames (default: capacity), one launch (`ds2_ctc_beam_stream_commit`, csrc/ctc_beam_commit.h) writes the stable
    (label, offset) pairs that have not left yet to the host (`committed[b]`: (labels, offsets), the text every later result starts
    with) and renumbers the LIVE TREE, the chains from the live beams down to the last committed pair, into the front of a fresh
    buffer; one device-to-host copy brings the pairs and the tree's size (`live_nodes[b]`).  The storage (`capacity`, in rows of
    beam_width nodes) doubles only when live tree + chunk still do not fit; read-outs are sized by the uncommitted labels, not by the
    stream.  Records and finish() are those of an uncommitted stream, bit for bit: node ids never enter the search's arithmetic.
    That is exact, and it bounds memory whenever the tree is small: over silence it is a handful of nodes, but a full beam of peaked
    frames can keep an early low-margin alternative alive for as long as the stream runs, and then the tree grows with it.
    max_lag (frames) is the stated bound for that case: at a commit, the first slot of the search decides the text older than max_lag
    frames, beams that disagree are dropped (`forced[b]` counts the commits at which one was), and every node older than the cut
    leaves.  With max_lag a result may differ from decode(); without it, it never does.  `commits`: commit launches so far.

    finish(index) ends ONE utterance of the batch: decode()'s result for its frames so far, and its slot reopened for the next call.
    `frames`: the frames consumed per utterance; `closed`: finish() has run.
    Limits that remain: 2^20 - 1 labels per utterance between two finish(index) (the length field of the candidate key); fp32
    totals are absolute, not rebased, so their resolution falls as a stream's total grows.
    NOT MEASURED: how far the stable prefix lags the best hypothesis on real recordings; what max_lag costs in WER; how large the live
    tree gets on real recordings at width 100."""

    def __init__(self, decoder, batch=1, nbest=1, capacity=256, commit=False, commit_every=None, max_lag=None):
        from ..ops import _is_int
        for name, v in (("commit_every", commit_every), ("max_lag", max_lag)):
            if v is None:
                continue
            try:
                ok = _is_int(v, 1)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"BeamStream: {name} must be a positive integer number of frames, got {v!r}")
            if not commit:
                raise ValueError(f"BeamStream: {name} needs commit=True")
        if not _is_int(batch, 1):
            raise ValueError(f"BeamStream: batch must be a positive integer, got {batch!r}")
        if not _is_int(nbest, 1, decoder.beam_width):
            raise ValueError(f"BeamStream: nbest must be an integer in 1..beam_width ({decoder.beam_width}), got {nbest!r}")
        if not _is_int(capacity, 1):
            raise ValueError(f"BeamStream: capacity must be a positive number of frames, got {capacity!r}")
        self.decoder, self.batch, self.nbest = decoder, int(batch), int(nbest)
        self.search = dict(blank=decoder.blank_index, beam_width=decoder.beam_width, cutoff_top_n=decoder.cutoff_top_n,
                           cutoff_prob=decoder.cutoff_prob, lm=decoder.lm, alpha=decoder.alpha, beta=decoder.beta, hotwords=decoder.hotwords)
        self.C, self.frames, self.closed = None, [0] * self.batch, False
        self.capacity, self._first_capacity = 0, int(capacity)
        self._state = self._nodes = None
        self.commit = bool(commit)
        self.commit_every = None if not commit else int(commit_every) if commit_every is not None else int(capacity)
        self.max_lag = None if max_lag is None else int(max_lag)
        self.commits, self.live_nodes, self.forced = 0, [0] * self.batch, [0] * self.batch
        self.committed = [([], []) for _ in range(self.batch)]      # per utterance: the labels and offsets that left the device
        self._commit_frame = [0] * self.batch                       # the frame of each utterance's last committed pair
        self._rows, self._lab, self._since = [0] * self.batch, [0] * self.batch, 0   # bounds: rows in use, uncommitted labels; frames since

    def check_feed(self, probs, sizes=None):
        """The host half of feed(), before any device call: refuses a closed stream, a shape that is not (batch, T, C) (or (T, C) with
        batch 1), a C other than the first feed's, and sizes outside [0, T] -> (probs (B, T, C), the chunk's frames per utterance as a
        list).  The first call fixes C."""
        if self.closed:
            raise ValueError("BeamStream.feed: the stream is closed (finish() has run)")
        probs = torch.as_tensor(probs)
        if probs.dim() == 2 and self.batch == 1:
            probs = probs[None]
        if probs.dim() != 3 or probs.size(0) != self.batch:
            raise ValueError(f"BeamStream.feed: probs must be ({self.batch}, T, C){' or (T, C)' if self.batch == 1 else ''}, "
                             f"got {tuple(probs.shape)}")
        T, C = probs.size(1), probs.size(2)
        if T < 1:
            raise ValueError("BeamStream.feed: a chunk needs at least one frame (sizes may be 0)")
        if self.C is not None and C != self.C:
            raise ValueError(f"BeamStream.feed: the stream was opened with {self.C} classes, this chunk has {C}")
        if sizes is None:
            n = [T] * self.batch
        else:
            sizes = torch.as_tensor(sizes).reshape(-1)
            if sizes.numel() != self.batch or sizes.dtype.is_floating_point:
                raise ValueError(f"BeamStream.feed: sizes must hold {self.batch} integers")
            n = [int(v) for v in sizes.tolist()]
            if any(v < 0 or v > T for v in n):
                raise ValueError(f"BeamStream.feed: sizes {n} outside [0, {T}], the chunk's frames")
        self.C = C
        return probs, n

    def _device_state(self, dev, need):
        """the state (zeros: a fresh stream) and node storage for `need` frames, grown by doubling with the nodes copied over"""
        from .. import ops
        K = self.search["beam_width"]
        if self._state is None:
            self._state = ops.ctc_beam_stream_state(self.batch, K, self.search["lm"], self.search["hotwords"], dev)
        cap = stream_capacity(self.capacity or self._first_capacity, need)
        if cap != self.capacity:
            self._nodes = ops.ctc_beam_stream_nodes(self.batch, cap, K, dev, self._nodes, self.capacity)
            self.capacity = cap

    def _commit(self, dev, chunk):
        """one commit launch and one device-to-host copy; then the storage grows if the live tree and `chunk` frames do not fit"""
        from .. import ops
        K, B = self.search["beam_width"], self.batch
        cut = None
        if self.max_lag is not None:
            cut = torch.tensor([f - self.max_lag for f in self.frames], dtype=torch.int32).to(dev)   # (< 0: no cut yet)
        width = max(self._lab)
        fresh = ops.ctc_beam_stream_nodes(B, self.capacity, K, dev)
        packed = ops.ctc_beam_stream_commit(self._state, self._nodes, self.capacity, fresh, self.capacity, K, self.search["lm"],
                                            self.search["hotwords"], width, cut)[4]
        info, dropped, labels, offs = ops.commit_unpack(packed.cpu(), B, width)
        self._nodes = fresh
        for b in range(B):
            n = int(info[b, 0])
            self.committed[b][0].extend(labels[b, :n].tolist())
            self.committed[b][1].extend(offs[b, :n].tolist())
            self.live_nodes[b], self._lab[b], self._commit_frame[b] = int(info[b, 1]), int(info[b, 2]), int(info[b, 3])
            self.forced[b] += int(dropped[b]) > 0
        self.commits += 1
        self._since = 0
        rows, cap = commit_capacity(self.capacity, self.live_nodes, K, chunk)
        self._rows = [(m + K - 1) // K for m in self.live_nodes]
        if cap != self.capacity:
            self._nodes = ops.ctc_beam_stream_nodes(B, cap, K, dev, self._nodes, self.capacity)
            self.capacity = cap

    def _call(self, probs, sizes, n_out, dev, index=None):
        """one feed launch (probs None: a pure read-out; index: of that utterance alone, through views of its state and nodes)"""
        from .. import ops
        T = 0 if probs is None else probs.size(1)
        classes = self.C if self.C is not None else len(self.decoder.labels)
        if not self.commit:
            bound = max(self.frames) if index is None else self.frames[index]
            self._device_state(dev, max(self.frames) + T)
            state, nodes = self._slot(index)
            return ops.ctc_beam_stream_feed(probs, sizes, state, nodes, self.capacity, bound, n_out, classes=classes, **self.search)
        if self._nodes is not None and T and commit_due(self.capacity, max(self._rows), T, self._since, self.commit_every):
            self._commit(dev, T)
        self._device_state(dev, max(self._rows) + T)      # (the first feed, or a chunk the doubling has yet to make room for)
        state, nodes = self._slot(index)
        rows, lab = (max(self._rows), max(self._lab)) if index is None else (self._rows[index], self._lab[index])
        out = ops.ctc_beam_stream_feed_committed(probs, sizes, state, nodes, self.capacity, rows, lab, n_out, classes=classes, **self.search)
        self._rows, self._lab, self._since = [r + T for r in self._rows], [n + T for n in self._lab], self._since + T
        return out

    def _slot(self, index):
        """the state and the nodes of the whole batch, or contiguous views of one utterance's"""
        if index is None:
            return self._state, self._nodes
        stride = self._state.numel() // self.batch
        return self._state[index * stride:(index + 1) * stride], self._nodes[index:index + 1]

    def _join(self, b, labels, offs, lens, scores):
        """utterance b's read-out rows (n_out, W) of a committing stream -> full rows: the committed pairs, then the read-out's.  A slot
        past the surviving beams stays empty, as decode() leaves it."""
        head_l, head_o = self.committed[b]
        n = len(head_l)
        if n == 0:
            return labels, offs
        alive = ((lens >= n) & (scores > -math.inf)).to(labels.dtype)[:, None]      # (n_out, 1)
        return (torch.cat((torch.tensor(head_l, dtype=labels.dtype)[None] * alive, labels * alive), 1),
                torch.cat((torch.tensor(head_o, dtype=offs.dtype)[None] * alive, offs * alive), 1))

    def _joined(self, labels, offs, lens, scores, only=None):
        """the download of a read-out -> per utterance rows that start at the utterance's first label (lists over the batch)"""
        ids = range(self.batch) if only is None else [only]
        if not self.commit:
            return [labels[i] for i in range(len(ids))], [offs[i] for i in range(len(ids))]
        pairs = [self._join(b, labels[i], offs[i], lens[i], scores[i]) for i, b in enumerate(ids)]
        return [p[0] for p in pairs], [p[1] for p in pairs]

    def _download(self, out, dev):
        """one device-to-host copy of a read-out -> labels, offsets (B, n_out, W), lens (B, n_out), scores (B, n_out) fp32, stable (B)"""
        from .. import ops
        labels, offs, lens, scores, stable, _ = out
        B, n_out, W = labels.shape
        host = torch.cat((labels.reshape(-1), offs.reshape(-1), lens.reshape(-1), scores.view(torch.int32).reshape(-1), stable)).cpu()
        if ops.rnn_poison_seen(dev):
            ops.rnn_persistent_check(dev)    # as in BeamCTCDecoder.decode: a poisoned forward raises here
        n, m = B * n_out * W, B * n_out
        return (host[:n].view(B, n_out, W), host[n:2 * n].view(B, n_out, W), host[2 * n:2 * n + m].view(B, n_out),
                host[2 * n + m:2 * n + 2 * m].view(torch.float32).view(B, n_out).clone(), host[2 * n + 2 * m:].tolist())

    def feed(self, probs, sizes=None, partial=True):
        """probs (B, T, C) or, with batch 1, (T, C) probabilities, on the host or the device, as decode() takes them; sizes: the chunk's
        valid frames per utterance (0: the utterance has nothing in this chunk).  One launch.  partial=True: one device-to-host copy and
        one record per utterance: {"text", "offsets", "score": the best hypothesis so far, as decode() of the frames so far gives it;
        "stable": how many of its characters are final, in every later result and in finish(), with their offsets; "stable_text": those
        characters; "frames": the frames consumed; with nbest > 1 "nbest": [(text, offsets, score)]}.  partial=False: nothing is copied,
        None is returned."""
        probs, n = self.check_feed(probs, sizes)
        if not probs.is_cuda:
            probs = probs.to(_device("BeamStream", ".feed"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        dev = probs.device
        out = self._call(probs, None if sizes is None else torch.tensor(n, dtype=torch.int32), self.nbest if partial else 0, dev)
        self.frames = [f + v for f, v in zip(self.frames, n)]
        if not partial:
            return None
        labels, offs, lens, scores, stable = self._download(out, dev)
        labels, offs = self._joined(labels, offs, lens, scores)
        strings, offsets = self.decoder.convert_to_strings(labels, lens), self.decoder.convert_tensor(offs, lens)
        records = []
        for b in range(self.batch):
            rec = {"text": strings[b][0], "offsets": offsets[b][0], "score": float(scores[b, 0]), "stable": stable[b],
                   "stable_text": strings[b][0][:stable[b]], "frames": self.frames[b]}
            if self.nbest > 1:
                rec["nbest"] = [(strings[b][k], offsets[b][k], float(scores[b, k])) for k in range(self.nbest)]
            records.append(rec)
        return records

    def finish(self, index=None):
        """Ends the stream -> (strings[b][k], offsets[b][k]) with beam_width entries per utterance, as BeamCTCDecoder.decode() returns
        them for the concatenated frames; the decoder's `last_scores` are set as decode() sets them.  A stream that was never fed
        gives decode()'s result for utterances of 0 frames.  A later feed() raises ValueError.
        finish(index) ends utterance `index` alone -> (strings[k], offsets[k], scores (beam_width) fp32): decode()'s result for its
        frames so far, read out and copied to the host for that utterance only.  Its slot is reopened (its state zeroed, frames[index]
        = 0, its committed text cleared): the next frames fed to it start a new utterance.  The other utterances are untouched, the
        stream stays open and the decoder's last_scores are left alone."""
        if self.closed:
            raise ValueError("BeamStream.finish: the stream is closed already")
        if index is not None:
            from ..ops import _is_int
            try:
                ok = _is_int(index, 0, self.batch - 1)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"BeamStream.finish: index must be an integer in 0..{self.batch - 1}, got {index!r}")
            index = int(index)
        dev = self._state.device if self._state is not None else _device("BeamStream", ".finish")
        out = self._call(None, None, self.search["beam_width"], dev, index)
        labels, offs, lens, scores, _ = self._download(out, dev)
        labels, offs = self._joined(labels, offs, lens, scores, index)
        strings, offsets = self.decoder.convert_to_strings(labels, lens), self.decoder.convert_tensor(offs, lens)
        if index is not None:
            self._slot(index)[0].zero_()
            self.frames[index] = self.live_nodes[index] = self._rows[index] = self._lab[index] = self._commit_frame[index] = 0
            self.committed[index] = ([], [])
            return strings[0], offsets[0], scores[0]
        self.closed = True
        self._state = self._nodes = None
        self.decoder.last_scores = scores
        return strings, offsets


def _reference_strings(references):
    """references as tune_lm_weights takes them: strings, or evaluate()'s output_data form [[str]] -> a list of strings"""
    out = []
    for r in references:
        if not isinstance(r, str):
            r = list(r)
            if len(r) != 1 or not isinstance(r[0], str):
                raise ValueError("references must be strings, or one-element lists of a string as evaluate()'s output_data holds them")
            r = r[0]
        out.append(r)
    return out


def _check_grid(who, alphas, betas, metric):
    alphas, betas = (np.asarray(list(np.ravel(g)), np.float64) for g in (alphas, betas))
    if alphas.size < 1 or betas.size < 1 or not (np.isfinite(alphas).all() and np.isfinite(betas).all()):
        raise ValueError(f"{who}: alphas and betas must be non-empty and finite")
    if metric not in ("wer", "cer"):
        raise ValueError(f"{who}: metric must be 'wer' or 'cer', got {metric!r}")
    return alphas, betas


def tune_summary(total, ref_words, ref_chars, alphas, betas, metric="wer", first_pass=(0, 0), oracle=(0, 0)):
    """Pure host half of tune_lm_weights: total (Ga,Gb,2) the summed (word, character) errors of the picks at every grid point,
    ref_words / ref_chars the references' summed lengths (0 divides as 1, as in evaluate()), first_pass / oracle the summed (word,
    character) errors of slot 0 and of the best slot per utterance -> the dict tune_lm_weights returns.  Rates are percentages, as
    evaluate() returns them.  The winner is the lowest error count on `metric`; ties go to the first point in row-major (alpha, beta)
    order."""
    alphas, betas = _check_grid("tune_summary", alphas, betas, metric)
    total = np.asarray(total)
    if total.shape != (alphas.size, betas.size, 2):
        raise ValueError(f"tune_summary: totals of {total.shape} for a {alphas.size} x {betas.size} grid")
    nw, nc = max(int(ref_words), 1), max(int(ref_chars), 1)
    col = 0 if metric == "wer" else 1
    a, b = np.unravel_index(int(np.argmin(total[:, :, col])), total.shape[:2])   # argmin: the first of equal minima, row-major
    rate = lambda pair: (100.0 * int(pair[0]) / nw, 100.0 * int(pair[1]) / nc)   # noqa: E731
    return {"alpha": float(alphas[a]), "beta": float(betas[b]), "wer": rate(total[a, b])[0], "cer": rate(total[a, b])[1],
            "grid_wer": 100.0 * total[:, :, 0].astype(np.float64) / nw, "grid_cer": 100.0 * total[:, :, 1].astype(np.float64) / nc,
            "first_pass": rate(first_pass), "oracle": rate(oracle)}


class NBestRescorer:
    """Second pass over a BeamCTCDecoder's n-best list: every hypothesis gets the feature vector (acoustic log-likelihood, LM log10 sum,
    token count, OOV count), and a score (ac + alpha * (lm_sum + oov_score * n_oov)) + beta * n_tok under ANY weights, without decoding
    again (contracts: include/ds2hip.h, ds2_lm_score_seqs and ds2_nbest_sweep).
      decoder   the first pass, run with its own settings (LM, hotwords, width);
      lm        the rescoring model: an ARPA path, an NgramLM, or None = the decoder's own.  It may be larger than what the first pass
                could carry (any order up to 6: the search's candidate limit does not apply here);
      acoustic  "exact": the CTC likelihood of every hypothesis recomputed from the posteriors (ops.ctc_mwer's lattices), free of the LM
                and hotword terms that only chose the list; "beam": the first pass's scores, refused when the decoder has an LM or
                hotwords, whose terms are inside those scores;
      oov_score the log10 price of an out-of-vocabulary token (the search's is -1000);
      workspace_bytes  bound on the exact likelihoods' workspace: the batch is cut into chunks of utterances that stay within it (at
                least one utterance per chunk).
    Exact: the likelihoods (fp32 lattices of the loss) and the LM sums (the search's own cond_score, added in token order).  NOT part of
    the score: hotword terms.  NOT pinned: parity with ctcdecode's or KenLM's scoring; OOV is a constant, not an <unk> probability.
    NOT measured: whether weights tuned this way lower the WER of a real corpus, and how far the optimum on n-best lists lies from
    the optimum of decoding again at every grid point."""

    def __init__(self, decoder, lm=None, acoustic="exact", oov_score=-1000.0, workspace_bytes=2 << 30):
        if not isinstance(decoder, BeamCTCDecoder):
            raise ValueError("NBestRescorer: decoder must be a BeamCTCDecoder")
        if acoustic not in ("exact", "beam"):
            raise ValueError(f"NBestRescorer: acoustic must be 'exact' or 'beam', got {acoustic!r}")
        if acoustic == "beam" and (decoder.lm is not None or decoder.hotwords is not None):
            raise ValueError("NBestRescorer: acoustic='beam' takes the first pass's scores as the acoustic term, but this decoder's scores "
                             "hold its language-model or hotword terms; use acoustic='exact'")
        if acoustic == "exact" and decoder.blank_index != 0:
            raise ValueError("NBestRescorer: acoustic='exact' needs blank_index 0 (the lattice kernels take class 0 as the blank)")
        if isinstance(lm, str):
            from .lm import NgramLM
            space = decoder.space_index if decoder.int_to_char.get(decoder.space_index) == " " else next(
                (i for i, c in sorted(decoder.int_to_char.items()) if c == " "), None)
            lm = NgramLM(lm, decoder.int_to_char, decoder.blank_index, space)
        lm = decoder.lm if lm is None else lm
        if lm is None:
            raise ValueError("NBestRescorer: no language model: pass lm=, or a decoder that has one")
        if lm.blank != decoder.blank_index:
            raise ValueError(f"NBestRescorer: the language model was bound to blank {lm.blank}, the decoder has blank {decoder.blank_index}")
        oov_score = float(oov_score)
        if math.isnan(oov_score):
            raise ValueError("NBestRescorer: oov_score is NaN")
        if isinstance(workspace_bytes, bool) or int(workspace_bytes) != workspace_bytes or int(workspace_bytes) < 1:
            raise ValueError(f"NBestRescorer: workspace_bytes must be a positive integer, got {workspace_bytes!r}")
        self.decoder, self.lm, self.acoustic, self.oov_score, self.workspace_bytes = decoder, lm, acoustic, oov_score, int(workspace_bytes)
        self.last_scores = None

    def _chunks(self, lens_h, T, K):
        """utterance ranges [b0, b1) whose exact-likelihood workspace, at the range's longest hypothesis, stays within workspace_bytes"""
        from .. import _lib
        need = _lib.load().ds2_ctc_mwer_workspace_bytes
        longest = lens_h.max(axis=1) if lens_h.size else np.zeros(0, np.int64)
        out, b0, B = [], 0, lens_h.shape[0]
        while b0 < B:
            b1, mh = b0 + 1, int(longest[b0])
            while b1 < B and need(T, b1 + 1 - b0, K, max(mh, int(longest[b1]))) <= self.workspace_bytes:
                mh = max(mh, int(longest[b1]))
                b1 += 1
            out.append((b0, b1, mh))
            b0 = b1
        return out

    def exact_likelihoods(self, logp, labels, off, lens, valid, in_lens, lens_host):
        """log p_ctc of every slot, (B,K) fp32 on the GPU: ops.ctc_mwer's lattices (want_grad=False) on logp (B,T,C), chunk by chunk
        (_chunks), max_hyp_len the chunk's longest hypothesis.  labels (B,K,T) i32, off (B,K) i64 into it, lens (B,K) i32, valid
        (B,K) bool, in_lens (B) i32 on the GPU; lens_host: the lengths as a NumPy array.  An invalid slot gets -inf."""
        from .. import ops
        B, K, T = labels.shape
        valid_i = valid.to(torch.int32)
        risk = torch.zeros((B, K), dtype=torch.float32, device=labels.device)
        ac = torch.empty((B, K), dtype=torch.float32, device=labels.device)
        for b0, b1, mh in self._chunks(lens_host, T, K):
            x = torch.empty((T, b1 - b0, logp.shape[2]), dtype=torch.float32, device=logp.device)   # (fresh: canonical strides at b1 - b0 = 1 too)
            x.copy_(logp[b0:b1].transpose(0, 1))
            _, nll, _, _ = ops.ctc_mwer(x, labels, off[b0:b1], lens[b0:b1], valid_i[b0:b1], in_lens[b0:b1], mh, risk[b0:b1], want_grad=False)
            ac[b0:b1] = -nll
        return ac

    def features(self, probs, sizes=None, is_log=False):
        """probs (B,T,C) as decode() takes them (probabilities, or log-probabilities with is_log=True), sizes (B) valid frames or None
        -> a dict of GPU tensors: "labels" / "offsets" (B,K,T) i32, "lens" (B,K) i32 and "scores" (B,K) fp32 of the first pass,
        "ac" (B,K) fp32 natural log (-inf for an empty slot), "lm_sum" (B,K) fp32 log10, "n_tok", "n_oov" (B,K) i32; and "lens_host", the
        lengths as a NumPy array.  The labels make no host round trip; the lengths are copied once."""
        from .. import ops
        dec = self.decoder
        probs = torch.as_tensor(probs)
        if probs.dim() != 3:
            raise ValueError(f"NBestRescorer.features: probs must be (B,T,C), got {tuple(probs.shape)}")
        if not probs.is_cuda:
            probs = probs.to(_device("NBestRescorer", ".features"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        B, T, C = probs.shape
        dev = probs.device
        sizes = None if sizes is None else torch.as_tensor(sizes)
        logp = probs if is_log else None
        if is_log:
            probs = torch.exp(probs)
        labels, offs, lens, scores = ops.ctc_beam_decode(probs, sizes, dec.blank_index, dec.beam_width, dec.cutoff_top_n, dec.cutoff_prob,
                                                         dec.lm, dec.alpha, dec.beta, dec.hotwords)
        K = labels.shape[1]
        off = torch.arange(B * K, device=dev, dtype=torch.int64) * T
        lm_sum, n_tok, n_oov = (t.view(B, K) for t in ops.lm_score(labels, off, lens.view(-1), self.lm, T))
        lens_h = lens.cpu().numpy()
        if ops.rnn_poison_seen(dev):
            # as in GreedyDecoder.decode: a poisoned forward (a starved persistent recurrence launch) raises here
            ops.rnn_persistent_check(dev)
        valid = scores > -math.inf
        if self.acoustic == "beam":
            ac = scores.clone()
        else:
            in_lens = torch.full((B,), T, dtype=torch.int32, device=dev) if sizes is None else ops._sizes_i32(sizes, B, dev)
            ac = self.exact_likelihoods(torch.log(probs) if logp is None else logp, labels, off.view(B, K), lens, valid, in_lens, lens_h)
        ac = torch.where(valid, ac, torch.full_like(ac, -math.inf))
        return {"labels": labels, "offsets": offs, "lens": lens, "scores": scores, "ac": ac, "lm_sum": lm_sum, "n_tok": n_tok,
                "n_oov": n_oov, "lens_host": lens_h}

    def strings(self, features):
        """the hypotheses of `features` as strings[b][k] (one device-to-host copy of the labels; kept in features["strings"])"""
        if "strings" not in features:
            features["strings"] = self.decoder.convert_to_strings(features["labels"].cpu(), features["lens_host"])
        return features["strings"]

    def scores(self, features, alpha, beta):
        """(B,K) fp32 on the GPU: the score of every slot at (alpha, beta), rounded as ds2_nbest_sweep rounds it; NaN counts as -inf"""
        f = features
        w = lambda v: torch.full((), float(v), dtype=torch.float32, device=f["ac"].device)   # noqa: E731
        lm = f["lm_sum"] + w(self.oov_score) * f["n_oov"].float()
        s = (f["ac"] + w(alpha) * lm) + w(beta) * f["n_tok"].float()
        return torch.where(torch.isnan(s), torch.full_like(s, -math.inf), s)

    def rescore(self, probs, sizes=None, alpha=0.0, beta=0.0, is_log=False):
        """What decode() returns, (strings[b][k], offsets[b][k]), K per utterance, reordered by the rescored total at (alpha, beta):
        highest first, equal totals in first-pass order (the sweep's tie rule).  The totals stay in `last_scores` (B,K) on the host."""
        f = self.features(probs, sizes, is_log)
        s, order = torch.sort(self.scores(f, alpha, beta), dim=1, descending=True, stable=True)
        B, K, T = f["labels"].shape
        idx = order[:, :, None].expand(B, K, T)
        lens = torch.gather(f["lens"], 1, order)
        host = torch.cat((torch.gather(f["labels"], 1, idx).reshape(-1), torch.gather(f["offsets"], 1, idx).reshape(-1), lens.reshape(-1),
                          s.contiguous().view(torch.int32).reshape(-1))).cpu()
        n = B * K * T
        lens_h = host[2 * n:2 * n + B * K].view(B, K)
        self.last_scores = host[2 * n + B * K:].view(torch.float32).view(B, K).clone()
        return (self.decoder.convert_to_strings(host[:n].view(B, K, T), lens_h),
                self.decoder.convert_tensor(host[n:2 * n].view(B, K, T), lens_h))

    def errors(self, features, references):
        """The word and character distances of every slot against its utterance's reference (pack_scoring, one ops.edit_distance launch)
        -> (B,K,2) int32 on the GPU; features["ref_len"] receives the (B,2) reference lengths (words, characters) as a NumPy array."""
        from .. import ops
        references = _reference_strings(references)
        strings = self.strings(features)
        B, K = len(strings), len(strings[0]) if strings else 0
        if len(references) != B:
            raise ValueError(f"NBestRescorer.errors: {len(references)} references for a batch of {B}")
        dev = features["ac"].device
        seq, a_off, a_len, b_off, b_len, ref_w, ref_c = pack_scoring([h for row in strings for h in row], [r for r in references for _ in range(K)])
        features["ref_len"] = np.stack((ref_w[::K], ref_c[::K]), axis=1) if B else np.zeros((0, 2), np.int64)
        if B * K == 0:
            return torch.zeros((B, K, 2), dtype=torch.int32, device=dev)
        max_len = int(max(a_len.max(), b_len.max()))
        dist = ops.edit_distance(*_upload_scoring(dev, seq, a_off, a_len, b_off, b_len), max_len=max_len)
        return torch.stack((dist[:B * K].view(B, K), dist[B * K:].view(B, K)), dim=2).contiguous()


def tune_lm_weights(rescorer, batches, alphas, betas, metric="wer"):
    """Choose the LM weights of a BeamCTCDecoder on a dev set from ONE decode: `batches` yields (probs, sizes, reference strings), and a
    list of evaluate()'s output_data triples is accepted as it is.  Every batch gives rescorer.features and rescorer.errors, which
    stay on the GPU; then one ops.nbest_sweep runs over the whole alphas x betas grid.  Returns {"alpha", "beta", "wer", "cer" at that
    point, "grid_wer", "grid_cer" (Ga,Gb), "first_pass": (wer, cer) of slot 0, "oracle": (wer, cer) of the best slot per utterance},
    rates as percentages (tune_summary).  What the chosen weights do to the WER of decoding again is not measured here: rescoring
    only sees the hypotheses the first pass kept."""
    from .. import ops
    alphas, betas = _check_grid("tune_lm_weights", alphas, betas, metric)
    feats, errs, ref = {k: [] for k in ("ac", "lm_sum", "n_tok", "n_oov")}, [], np.zeros(2, np.int64)
    for probs, sizes, references in batches:
        f = rescorer.features(probs, sizes)
        errs.append(rescorer.errors(f, references))
        ref += f["ref_len"].sum(axis=0)
        for k in feats:
            feats[k].append(f[k])
    if not errs:
        raise ValueError("tune_lm_weights: no batch")
    ac, lm_sum, n_tok, n_oov = (torch.cat(feats[k]).contiguous() for k in ("ac", "lm_sum", "n_tok", "n_oov"))
    err = torch.cat(errs).contiguous()
    _, total = ops.nbest_sweep(ac, lm_sum, n_tok, n_oov, err, alphas, betas, rescorer.oov_score, want_pick=False)
    # the best slot per utterance among the surviving ones (slot 0 where none survived), per error kind
    big = torch.iinfo(torch.int32).max
    live = (ac > -math.inf)[:, :, None].expand_as(err)
    best = torch.where(live, err, torch.full_like(err, big)).min(dim=1).values
    best = torch.where(best == big, err[:, 0, :], best)
    host = torch.cat((total.reshape(-1), err[:, 0, :].sum(0, dtype=torch.int64), best.sum(0, dtype=torch.int64))).cpu().numpy()
    return tune_summary(host[:-4].reshape(alphas.size, betas.size, 2), ref[0], ref[1], alphas, betas, metric, host[-4:-2], host[-2:])


def encode_transcripts(transcripts, labels, star=None, unknown="error"):
    """Transcripts (strings, or sequences of label ids) -> one list of ids each.  Strings are mapped through `labels` ({char: id} or a
    sequence of characters); a character that is not a label raises ValueError naming it.
    Wildcards (CTCAligner.align's star / unknown): the id len(labels), one past the last class, is the wildcard.  `star`, a single
    character that is not a label, maps to it; with unknown="star" so does every character that is not a label.  With either option
    runs of adjacent wildcards collapse to one (in id sequences too, where the id len(labels) is the wildcard)."""
    char_to_int = labels if isinstance(labels, dict) else {c: i for i, c in enumerate(labels)}
    if unknown not in ("error", "star"):
        raise ValueError(f"unknown must be 'error' or 'star', got {unknown!r}")
    if star is not None:
        if not isinstance(star, str) or len(star) != 1:
            raise ValueError(f"star must be a single character, got {star!r}")
        if star in char_to_int:
            raise ValueError(f"star {star!r} is a label: choose a character outside the label set")
    star_id = len(char_to_int)
    wild = star is not None or unknown == "star"
    out = []
    for n, tr in enumerate(transcripts):
        if isinstance(tr, str):
            ids = []
            for ch in tr:
                if ch in char_to_int:
                    ids.append(int(char_to_int[ch]))
                elif ch == star or unknown == "star":
                    ids.append(star_id)
                else:
                    raise ValueError(f"transcript {n}: character {ch!r} is not in the labels")
        else:
            ids = [int(i) for i in (tr.tolist() if hasattr(tr, "tolist") else tr)]
        if wild:
            ids = [i for k, i in enumerate(ids) if not (i == star_id and k > 0 and ids[k - 1] == star_id)]
        out.append(ids)
    return out


def wildcard_ends(targets, star_id, free_start=False, free_end=False, distinct_paths=False):
    """The free_start / free_end rule of CTCAligner.align and asr_amd.CTCLoss on id lists: a wildcard (star_id) is put at the front /
    back of every target unless one is there, runs of adjacent wildcards collapse to one, and the per-utterance flags say which end
    token is optional (bit 0 the first, bit 1 the last).  Returns (targets, flags).
    distinct_paths (the loss, which SUMS over state paths where the aligner takes the best one): a target of ONE token does not get
    both bits — its first token is its last, and with both the all-blank path would exist twice, in state 0 and in state 2 — it
    keeps bit 0, which already makes that token optional."""
    out = []
    for t in targets:
        t = [int(i) for i in t]
        if free_start and t[:1] != [star_id]:
            t = [star_id] + t
        if free_end and t[-1:] != [star_id]:
            t = t + [star_id]
        out.append([i for k, i in enumerate(t) if not (i == star_id and k > 0 and t[k - 1] == star_id)])
    flag = (1 if free_start else 0) | (2 if free_end else 0)
    flags = [1 if (distinct_paths and flag == 3 and len(t) < 2) else flag for t in out]
    return out, flags


def group_words(tokens, star=None):
    """tokens [(char, start, end, logp, ...)] -> words [(word, start, end, logp)]: a word is the run of tokens between space tokens
    (leading, trailing and doubled spaces make no word), from its first token's start to its last token's end, logp summed in fp64.
    `star`: the character of wildcard tokens, which end a word like a space and make none."""
    words, run = [], []
    for tok in list(tokens) + [(" ",)]:
        if tok[0] == " " or (star is not None and tok[0] == star):
            if run:
                words.append(("".join(t[0] for t in run), run[0][1], run[-1][2], float(sum(np.float64(t[3]) for t in run))))
            run = []
        else:
            run.append(tok)
    return words


def assemble_alignments(score, states, tok_start, tok_end, tok_logp, targets, sizes, int_to_char, space_index, star_id=None,
                        star_char="*"):
    """Pure host half of CTCAligner.align: the kernel's raw arrays (score (B), states (B,T), tok_* flat over all targets, in target
    order) + the targets (a list of id lists) and valid frame counts -> one record per utterance: {"score": float, "states": int tensor
    (T_b), "tokens": [(char, start, end, logp)], "words": [(word, start, end, logp)]}.  An infeasible utterance (score -inf) has empty
    states / tokens / words.
    star_id (None: no wildcards, the records above): the target id of the wildcard.  A token whose span is (-1, -1) (an optional first
    or last token that the path left out) does not appear; a wildcard that took frames appears in "tokens" as (star_char, start, end,
    logp), ends a word and makes none, and every record gains "unaligned": the (start, end) spans of its wildcards."""
    score, states = np.asarray(score, np.float32), np.asarray(states, np.int32)
    tok_start, tok_end, tok_logp = np.asarray(tok_start), np.asarray(tok_end), np.asarray(tok_logp, np.float32)
    records, off = [], 0
    for b, ids in enumerate(targets):
        U = len(ids)
        sc = float(score[b])
        if sc == float("-inf"):
            records.append({"score": sc, "states": torch.zeros(0, dtype=torch.int32), "tokens": [], "words": []})
            if star_id is not None:
                records[-1]["unaligned"] = []
        elif star_id is None:
            Tb = max(min(int(sizes[b]), states.shape[1]), 0)
            tokens = [(" " if i == space_index else int_to_char.get(i, ""), int(tok_start[off + u]), int(tok_end[off + u]),
                       float(tok_logp[off + u])) for u, i in enumerate(ids)]
            records.append({"score": sc, "states": torch.from_numpy(states[b, :Tb].copy()), "tokens": tokens, "words": group_words(tokens)})
        else:
            Tb = max(min(int(sizes[b]), states.shape[1]), 0)
            tokens, breaks, unaligned = [], [], []              # breaks: the tokens with every wildcard as a space, for the words
            for u, i in enumerate(ids):
                s, e, lp = int(tok_start[off + u]), int(tok_end[off + u]), float(tok_logp[off + u])
                if s < 0:
                    continue
                ch = star_char if i == star_id else (" " if i == space_index else int_to_char.get(i, ""))
                tokens.append((ch, s, e, lp))
                breaks.append((" ", s, e, lp) if i == star_id else tokens[-1])
                if i == star_id:
                    unaligned.append((s, e))
            records.append({"score": sc, "states": torch.from_numpy(states[b, :Tb].copy()), "tokens": tokens, "words": group_words(breaks),
                            "unaligned": unaligned})
        off += U
    return records


def add_seconds(records, frame_seconds):
    """Every token and word tuple of the records gains (start_s, end_s) = (start, end) * frame_seconds, and so does every (start, end)
    span of "unaligned" where a record has that key.  An utterance's list of KeywordSpotter detections gains "start_s" / "end_s"."""
    for r in records:
        if isinstance(r, list):                          # KeywordSpotter.search: a list of detections per utterance
            for d in r:
                d["start_s"], d["end_s"] = d["start"] * frame_seconds, d["end"] * frame_seconds
            continue
        for key in ("tokens", "words"):
            r[key] = [t + (t[1] * frame_seconds, t[2] * frame_seconds) for t in r[key]]
        if "unaligned" in r:
            r["unaligned"] = [t + (t[0] * frame_seconds, t[1] * frame_seconds) for t in r["unaligned"]]
    return records


class CTCAligner(Decoder):
    """CTC forced alignment: WHEN a known transcript was spoken.  `align` runs the Viterbi lattice, its backtrace and the token spans as
    one HIP launch (`ds2_ctc_align_f32`, contract in include/ds2hip.h; restated by tests/ctc_align_oracle.py); the host packs the targets
    and assembles the records.  The reference has no aligner and parity with any external one is not pinned."""

    def __init__(self, labels, blank_index=0):
        if blank_index != 0:
            raise ValueError("CTCAligner: the alignment kernel takes class 0 as the blank (blank_index must be 0)")
        super().__init__(labels, blank_index)
        if self.int_to_char.get(self.space_index) != " ":
            self.space_index = next((i for i, c in sorted(self.int_to_char.items()) if c == " "), -1)

    def align(self, probs, sizes, transcripts, is_log=False, variant=0, star=None, star_penalty=math.log(0.5), unknown="error",
              free_start=False, free_end=False):
        """probs (B,T,C) as decode() takes them (probabilities, or log-probabilities with is_log=True), sizes (B) valid frames or None,
        transcripts: B strings (mapped through the labels) or id sequences.  One pinned upload of the packed targets, one launch, one
        device-to-host copy.  Returns one record per utterance (assemble_alignments).  Host tensors are uploaded first: there is no CPU
        implementation.  variant 0 - 2 as ops.ctc_forced_align takes them (one launch, targets up to about 3 275 labels); variant 3
        is ops.ctc_forced_align_tiled with the default tiles: the same records for a recording and a transcript of any length.
        Imperfect transcripts (contract: include/ds2hip.h, ds2_ctc_align_star_f32); with the four options at their defaults nothing
        below applies, the call takes the plain entries and star_penalty is unused:
          star="*"        that character (any single one that is not a label) in a transcript is a WILDCARD: a token that takes at
                          least one frame and matches anything, each of its frames scoring the frame's best class + star_penalty;
          unknown="star"  a character that is not a label becomes a wildcard instead of raising (in id sequences the id len(labels) is
                          the wildcard); runs of adjacent wildcards collapse to one;
          free_start / free_end  put a wildcard at the front / back (unless one is there) and make that token optional: audio before
                          the first or after the last word goes to it, and with none it is left out.
        star_penalty (<= 0, natural log): log(0.5) gives a frame to the transcript's token while that token has at least half the
        probability of the frame's best class.  That default is a starting point, NOT a measured one: what value serves real
        recordings has not been measured.  Records then hold the wildcards that took frames as (star or "*", start, end, logp) tokens,
        no word for them, and "unaligned": their (start, end) spans.  Variant 3 is ops.ctc_forced_align_star_tiled."""
        from .. import ops
        probs = torch.as_tensor(probs)
        B, T = int(probs.shape[0]), int(probs.shape[1])
        if len(transcripts) != B:
            raise ValueError(f"{len(transcripts)} transcripts for a batch of {B}")
        wild = star is not None or unknown != "error" or bool(free_start) or bool(free_end)
        targets = encode_transcripts(transcripts, self.labels, star, unknown)
        star_id = len(self.labels)
        flags = None
        if wild:
            if int(probs.shape[2]) != star_id:
                raise ValueError(f"probs has {int(probs.shape[2])} classes for {star_id} labels: the wildcard is the id one past the last class")
            sp = float(star_penalty)
            if not (sp <= 0.0 and math.isfinite(sp)):
                raise ValueError(f"star_penalty must be finite and <= 0, got {star_penalty}")
            targets, flags = wildcard_ends(targets, star_id, free_start, free_end)
        sizes_h = [T] * B if sizes is None else [int(v) for v in torch.as_tensor(sizes).reshape(-1).tolist()]
        if len(sizes_h) != B:
            raise ValueError(f"sizes has {len(sizes_h)} entries for a batch of {B}")
        if not probs.is_cuda:
            probs = probs.to(_device("CTCAligner", ".align"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        dev = probs.device
        lens = [len(t) for t in targets]
        n_tok, max_u = sum(lens), max(lens, default=0)
        # one int32 image: tgt_off, tgt_lens, in_lens, labels (, flags)
        host = torch.empty(3 * B + n_tok + (B if wild else 0), dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[:B] = np.cumsum([0] + lens[:-1]) if B else []
        h[B:2 * B], h[2 * B:3 * B] = lens, np.clip(sizes_h, -1, T)
        h[3 * B:3 * B + n_tok] = [i for t in targets for i in t]
        if wild:
            h[3 * B + n_tok:] = flags
        d = host.to(dev, non_blocking=True)
        if wild:                                         # the wildcard entries (ds2_ctc_align_star_*): a pre-pass and the same lattice
            if variant not in (0, 1, 2, 3):
                raise ValueError(f"variant must be 0, 1, 2 or 3, got {variant}")
            args = (probs, d[3 * B:3 * B + n_tok], d[:B], d[2 * B:3 * B], d[B:2 * B], max_u, is_log)
            if variant == 3:
                score, states, ts, te, lp = ops.ctc_forced_align_star_tiled(*args, star_penalty=sp, flags=d[3 * B + n_tok:])
            else:
                score, states, ts, te, lp = ops.ctc_forced_align_star(*args, variant, star_penalty=sp, flags=d[3 * B + n_tok:])
        elif variant == 3:                                 # the tiled lattice (ds2_ctc_align_tiled_f32, default tiles): any T, any target length
            score, states, ts, te, lp = ops.ctc_forced_align_tiled(probs, d[3 * B:], d[:B], d[2 * B:3 * B], d[B:2 * B], max_u, is_log)
        else:
            score, states, ts, te, lp = ops.ctc_forced_align(probs, d[3 * B:], d[:B], d[2 * B:3 * B], d[B:2 * B], max_u, is_log, variant)
        out = torch.cat((score.view(torch.int32), states.reshape(-1), ts, te, lp.view(torch.int32))).cpu()
        if ops.rnn_poison_seen(dev):
            # as in GreedyDecoder.decode: a poisoned forward (a starved persistent recurrence launch) raises here
            ops.rnn_persistent_check(dev)
        o = out.numpy()
        n = B + B * T
        return assemble_alignments(o[:B].view(np.float32), o[B:n].reshape(B, T), o[n:n + n_tok], o[n + n_tok:n + 2 * n_tok],
                                   o[n + 2 * n_tok:].view(np.float32), targets, sizes_h, self.int_to_char, self.space_index,
                                   star_id if wild else None, star or "*")


KWS_MAX_LEN, KWS_MAX_HITS = 63, 1024


def assemble_detections(hit_start, hit_end, hit_score, n_hits, keywords, kw_lens, max_hits):
    """Pure host half of KeywordSpotter.search: the kernel's hit arrays ((B,K,max_hits) each, n_hits (B,K)) -> per utterance the list
    of {"keyword", "start", "end" (exclusive), "score", "confidence": exp(score / U)} over all keywords, sorted by (start, end,
    keyword index).  Returns (records, overflowed): overflowed lists the (utterance, keyword) pairs whose n_hits is max_hits + 1."""
    hit_start, hit_end = np.asarray(hit_start), np.asarray(hit_end)
    hit_score, n_hits = np.asarray(hit_score, np.float32), np.asarray(n_hits)
    records, overflowed = [], []
    for b in range(n_hits.shape[0]):
        found = []
        for k, kw in enumerate(keywords):
            n = int(n_hits[b, k])
            if n > max_hits:
                overflowed.append((b, kw))
            for h in range(min(n, max_hits)):
                sc = float(hit_score[b, k, h])
                found.append((int(hit_start[b, k, h]), int(hit_end[b, k, h]), k, sc))
        records.append([{"keyword": keywords[k], "start": s, "end": e, "score": sc, "confidence": math.exp(sc / kw_lens[k])}
                        for s, e, k, sc in sorted(found)])
    return records, overflowed


class KeywordSpotter(Decoder):
    """Keyword search on CTC posteriors: WHERE a phrase was said, and whether at all, without a decode and without a transcript
    (Lengerich & Hannun 2016).  `search` runs every keyword against every utterance as one library call (`ds2_ctc_kws_f32`, contract in
    include/ds2hip.h; restated by tests/ctc_kws_oracle.py): a Viterbi lattice entered at any frame whose scores are log-likelihood
    ratios against the frame-wise best path (0 = the keyword's labels are the best class of every frame they take), then a greedy pick
    of non-overlapping detections.  The reference has no keyword search.
    keywords: strings over the labels (encode_transcripts, unknown="error"), 1 .. 63 labels each, no duplicates.
    threshold: a per-label probability ratio in (0, 1]: a detection of a keyword of U labels needs score >= U * log(threshold).  The
    default 0.5 mirrors the aligner's star_penalty and is a starting point, NOT a measured one: which value serves real recordings has
    not been measured.
    Matching is on the label stream and knows no word boundary: "cat" fires inside "catalog", as with the beam search's hotwords."""

    def __init__(self, labels, keywords, threshold=0.5, max_hits=32, blank_index=0):
        if blank_index != 0:
            raise ValueError("KeywordSpotter: the kernel takes class 0 as the blank (blank_index must be 0)")
        super().__init__(labels, blank_index)
        if isinstance(max_hits, bool) or int(max_hits) != max_hits or not 1 <= int(max_hits) <= KWS_MAX_HITS:
            raise ValueError(f"KeywordSpotter: max_hits must be an integer in [1, {KWS_MAX_HITS}], got {max_hits!r}")
        self.max_hits = int(max_hits)
        self.set_keywords(keywords, threshold)

    def set_keywords(self, keywords, threshold=None):
        """Replace the keyword list (and the threshold, unless None).  Nothing is kept on a refusal."""
        thr = self.threshold if threshold is None else float(threshold)
        if not (0.0 < thr <= 1.0):                       # (NaN fails too)
            raise ValueError(f"KeywordSpotter: threshold must lie in (0, 1], got {threshold!r}")
        if isinstance(keywords, str):
            raise ValueError("KeywordSpotter: keywords must be a list of strings, not one string")
        keywords = list(keywords)
        if not keywords:
            raise ValueError("KeywordSpotter: no keyword")
        if not all(isinstance(k, str) for k in keywords):
            raise ValueError("KeywordSpotter: keywords must be strings")
        ids = encode_transcripts(keywords, self.labels, unknown="error")
        for kw, i in zip(keywords, ids):
            if not i:
                raise ValueError("KeywordSpotter: empty keyword")
            if len(i) > KWS_MAX_LEN:
                raise ValueError(f"KeywordSpotter: keyword {kw!r} has {len(i)} labels, the kernel holds at most {KWS_MAX_LEN}")
            if self.blank_index in i:
                raise ValueError(f"KeywordSpotter: keyword {kw!r} contains the blank label")
        if len(set(keywords)) != len(keywords):
            dup = sorted(k for k in set(keywords) if keywords.count(k) > 1)
            raise ValueError(f"KeywordSpotter: duplicate keyword {dup[0]!r}")
        self.threshold, self.keywords, self.kw_ids = thr, keywords, ids
        self.kw_lens = [len(i) for i in ids]
        self.thr = np.array([u * math.log(thr) for u in self.kw_lens], np.float64).astype(np.float32)

    def search(self, probs, sizes=None, is_log=False, frame_seconds=None):
        """probs (B,T,C) as decode() takes them (probabilities, or log-probabilities with is_log=True), sizes (B) valid frames or None.
        One pinned upload of the packed keywords, one library call, one device-to-host copy of the hits.  Returns, per utterance, the
        detections of all keywords sorted by start: {"keyword", "start", "end" (frames, end exclusive), "score" (the path's
        log-likelihood ratio, <= 0), "confidence" (exp(score / U), the geometric mean per label, in (0, 1])}; with frame_seconds every
        record gains "start_s" / "end_s" (add_seconds).  Detections of ONE keyword never overlap; those of different keywords may.
        Warns when a keyword had more than max_hits detections in an utterance (the best max_hits in greedy order are kept).
        Host tensors are uploaded first: there is no CPU implementation.  T has no limit beyond the (B,K,T) frame arrays."""
        import warnings

        from .. import ops
        probs = torch.as_tensor(probs)
        if probs.dim() != 3:
            raise ValueError(f"KeywordSpotter.search: probs must be (B,T,C), got {tuple(probs.shape)}")
        B, T = int(probs.shape[0]), int(probs.shape[1])
        sizes_h = [T] * B if sizes is None else [int(v) for v in torch.as_tensor(sizes).reshape(-1).tolist()]
        if len(sizes_h) != B:
            raise ValueError(f"sizes has {len(sizes_h)} entries for a batch of {B}")
        if not probs.is_cuda:
            probs = probs.to(_device("KeywordSpotter", ".search"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        dev = probs.device
        K, n_lab = len(self.keywords), sum(self.kw_lens)
        # one int32 image: kw_off, kw_lens, thr (its bits), in_lens, labels
        host = torch.empty(3 * K + B + n_lab, dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[:K] = np.cumsum([0] + self.kw_lens[:-1])
        h[K:2 * K], h[2 * K:3 * K] = self.kw_lens, self.thr.view(np.int32)
        h[3 * K:3 * K + B] = np.clip(sizes_h, -1, T)
        h[3 * K + B:] = [i for ids in self.kw_ids for i in ids]
        d = host.to(dev, non_blocking=True)
        _, _, hs, he, hsc, nh = ops.ctc_keyword_search(probs, d[3 * K + B:], d[:K], d[K:2 * K], max(self.kw_lens), d[2 * K:3 * K].view(torch.float32),
                                                       d[3 * K:3 * K + B], is_log, self.max_hits)
        out = torch.cat((hs.reshape(-1), he.reshape(-1), hsc.view(torch.int32).reshape(-1), nh.reshape(-1))).cpu()
        if ops.rnn_poison_seen(dev):
            # as in GreedyDecoder.decode: a poisoned forward (a starved persistent recurrence launch) raises here
            ops.rnn_persistent_check(dev)
        o, n = out.numpy(), B * K * self.max_hits
        shape = (B, K, self.max_hits)
        records, overflowed = assemble_detections(o[:n].reshape(shape), o[n:2 * n].reshape(shape), o[2 * n:3 * n].view(np.float32).reshape(shape),
                                                  o[3 * n:].reshape(B, K), self.keywords, self.kw_lens, self.max_hits)
        if overflowed:
            b, kw = overflowed[0]
            warnings.warn(f"KeywordSpotter.search: more than max_hits={self.max_hits} detections for {len(overflowed)} (utterance, keyword) "
                          f"pair(s), the first: utterance {b}, keyword {kw!r}; the rest were dropped", RuntimeWarning, stacklevel=2)
        return records if frame_seconds is None else add_seconds(records, float(frame_seconds))

    def open_stream(self, batch=1, max_lag=None, pending=1024):
        """A running search over `batch` utterances that reports detections while the frames arrive: a KeywordStream (see there).
        max_lag: the most frames the settled part of the stream (the tail) may end behind the frames consumed after a feed, kept by
        forced cuts, which can lose a detection instead of releasing it (None: no cut, and the stream's detections are exactly
        search()'s); pending: the candidates kept per utterance and keyword between feeds.  The stream keeps its own copy of the
        keywords and thresholds: a later set_keywords does not touch it."""
        return KeywordStream(self, batch, max_lag, pending)


def assemble_stream_detections(hit_start, hit_end, hit_score, hit_final, n_hits, keywords, kw_lens, max_hits):
    """Pure host half of KeywordStream.feed: assemble_detections' records and order, every record with "final": True (reported now,
    once, and never changed) or False (tentative: the search's detection on the frames so far, which a later frame may still replace)."""
    hit_start, hit_end, hit_final = np.asarray(hit_start), np.asarray(hit_end), np.asarray(hit_final)
    hit_score, n_hits = np.asarray(hit_score, np.float32), np.asarray(n_hits)
    records, overflowed = [], []
    for b in range(n_hits.shape[0]):
        found = []
        for k, kw in enumerate(keywords):
            n = int(n_hits[b, k])
            if n > max_hits:
                overflowed.append((b, kw))
            for h in range(min(n, max_hits)):
                found.append((int(hit_start[b, k, h]), int(hit_end[b, k, h]), k, float(hit_score[b, k, h]), bool(hit_final[b, k, h])))
        records.append([{"keyword": keywords[k], "start": s, "end": e, "score": sc, "confidence": math.exp(sc / kw_lens[k]), "final": f}
                        for s, e, k, sc, f in sorted(found)])
    return records, overflowed


class KeywordStream:
    """A running keyword search over `batch` utterances (KeywordSpotter.open_stream): feed() consumes posteriors chunk by chunk and
    returns the detections that became FINAL with this chunk, each exactly once, and the TENTATIVE ones, which are the search's
    detections on the frames so far that a later frame may still replace; finish() flushes.  Without max_lag the final detections of
    the whole stream are exactly those of KeywordSpotter.search() on the concatenated frames, whatever the cuts
    (`ds2_ctc_kws_stream_feed_f32`, contract in include/ds2hip.h; restated by tests/ctc_kws_stream_oracle.py).  The state on the device
    is 4 * (264 + 3 * pending) bytes per utterance and keyword; memory and time per feed depend on the chunk, not on the stream's length.
    A detection is withheld while a path above the threshold that began before it is still alive (the keyword spoken up to its last
    label but one, then silence, keeps such a path for as long as the silence lasts).  max_lag bounds how far the settled part of the stream
    may end behind the frames consumed, by forced cuts, the only place where a stream may differ from search(): a cut that falls into a
    pending candidate's span loses that detection, so max_lag is no bound on how long a detection is withheld.  `detections`: the final records per utterance so far; `forced`, `dropped`:
    (batch, K) counts of forced cuts and of candidates lost to one or to a full pending list; `frames`; `closed`.
    NOT MEASURED: which max_lag serves real recordings, and how long detections are withheld on them without one."""

    def __init__(self, spotter, batch=1, max_lag=None, pending=1024):
        from ..ops import KWS_MAX_PENDING, _is_int
        if not _is_int(batch, 1):
            raise ValueError(f"KeywordStream: batch must be a positive integer, got {batch!r}")
        if max_lag is not None and not _is_int(max_lag, 0, 0x7fffffff):
            raise ValueError(f"KeywordStream: max_lag must be None or a number of frames >= 0, got {max_lag!r}")
        if not _is_int(pending, 1, KWS_MAX_PENDING):
            raise ValueError(f"KeywordStream: pending must be an integer in [1, {KWS_MAX_PENDING}], got {pending!r}")
        self.batch, self.max_lag, self.pending = int(batch), None if max_lag is None else int(max_lag), int(pending)
        self.keywords, self.kw_ids, self.kw_lens = list(spotter.keywords), [list(i) for i in spotter.kw_ids], list(spotter.kw_lens)
        self.max_hits, self.n_labels = spotter.max_hits, len(spotter.labels)
        K = len(self.keywords)
        # the constant part of the int32 image: kw_off, kw_lens, thr (its bits), labels; the chunk's sizes follow per feed
        self._image = np.concatenate([np.cumsum([0] + self.kw_lens[:-1]), self.kw_lens, spotter.thr.view(np.int32),
                                      [i for ids in self.kw_ids for i in ids]]).astype(np.int32)
        self.C, self.frames, self.closed = None, [0] * self.batch, False
        self.detections = [[] for _ in range(self.batch)]
        self.forced, self.dropped = np.zeros((self.batch, K), np.int64), np.zeros((self.batch, K), np.int64)
        self._state = None

    def check_feed(self, probs, sizes=None):
        """The host half of feed(), before any device call: refuses a closed stream, a shape that is not (batch, T, C) (or (T, C) with
        batch 1), a C other than the first feed's, and sizes outside [0, T] -> (probs (B, T, C), the chunk's frames per utterance as a
        list).  The first call fixes C."""
        if self.closed:
            raise ValueError("KeywordStream.feed: the stream is closed (finish() has run)")
        probs = torch.as_tensor(probs)
        if probs.dim() == 2 and self.batch == 1:
            probs = probs[None]
        if probs.dim() != 3 or probs.size(0) != self.batch:
            raise ValueError(f"KeywordStream.feed: probs must be ({self.batch}, T, C){' or (T, C)' if self.batch == 1 else ''}, "
                             f"got {tuple(probs.shape)}")
        T, C = probs.size(1), probs.size(2)
        if T < 1:
            raise ValueError("KeywordStream.feed: a chunk needs at least one frame (sizes may be 0)")
        if self.C is not None and C != self.C:
            raise ValueError(f"KeywordStream.feed: the stream was opened with {self.C} classes, this chunk has {C}")
        if sizes is None:
            n = [T] * self.batch
        else:
            sizes = torch.as_tensor(sizes).reshape(-1)
            if sizes.numel() != self.batch or sizes.dtype.is_floating_point:
                raise ValueError(f"KeywordStream.feed: sizes must hold {self.batch} integers")
            n = [int(v) for v in sizes.tolist()]
            if any(v < 0 or v > T for v in n):
                raise ValueError(f"KeywordStream.feed: sizes {n} outside [0, {T}], the chunk's frames")
        if max(self.frames) + T > 0x7fffffff:
            raise ValueError(f"KeywordStream.feed: {max(self.frames)} frames so far + {T} now pass 2^31 - 1")
        self.C = C
        return probs, n

    def _call(self, who, probs, n, is_log, finish, dev, frame_seconds):
        """one pinned upload (the packed keywords and the chunk's sizes), one library call, one device-to-host copy of the hits"""
        import warnings

        from .. import ops
        K, B = len(self.keywords), self.batch
        if self._state is None:
            self._state = ops.ctc_kws_stream_state(B, K, self.pending, dev)
        host = torch.empty(self._image.size + B, dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[:self._image.size], h[self._image.size:] = self._image, n
        d = host.to(dev, non_blocking=True)
        hs, he, hsc, hf, nh, _, _, forced, dropped, _, _ = ops.ctc_kws_stream_feed(
            probs, d[self._image.size:], self._state, d[3 * K:self._image.size], d[:K], d[K:2 * K], max(self.kw_lens),
            d[2 * K:3 * K].view(torch.float32), self.pending, max(self.frames), is_log, self.max_hits, self.max_lag, finish,
            classes=self.C if self.C is not None else self.n_labels, batch=B)
        out = torch.cat((hs.reshape(-1), he.reshape(-1), hsc.view(torch.int32).reshape(-1), hf.reshape(-1), nh.reshape(-1), forced.reshape(-1),
                         dropped.reshape(-1))).cpu()
        if ops.rnn_poison_seen(dev):
            ops.rnn_persistent_check(dev)    # as in KeywordSpotter.search: a poisoned forward raises here
        self.frames = [f + v for f, v in zip(self.frames, n)]
        o, m = out.numpy(), B * K * self.max_hits
        shape = (B, K, self.max_hits)
        records, overflowed = assemble_stream_detections(o[:m].reshape(shape), o[m:2 * m].reshape(shape), o[2 * m:3 * m].view(np.float32).reshape(shape),
                                                         o[3 * m:4 * m].reshape(shape), o[4 * m:4 * m + B * K].reshape(B, K), self.keywords,
                                                         self.kw_lens, self.max_hits)
        forced, dropped = (o[4 * m + (i + 1) * B * K:4 * m + (i + 2) * B * K].reshape(B, K).astype(np.int64) for i in (0, 1))
        lost = np.argwhere(dropped > self.dropped)
        self.forced, self.dropped = forced, dropped
        if overflowed:
            b, kw = overflowed[0]
            warnings.warn(f"{who}: more than max_hits={self.max_hits} detections for {len(overflowed)} (utterance, keyword) "
                          f"pair(s), the first: utterance {b}, keyword {kw!r}; the rest were dropped", RuntimeWarning, stacklevel=3)
        if len(lost):
            b, k = (int(v) for v in lost[0])
            why = f"more than pending={self.pending} candidates" if self.max_lag is None else \
                f"more than pending={self.pending} candidates, or candidates cut by max_lag={self.max_lag}"
            warnings.warn(f"{who}: {why} for {len(lost)} (utterance, keyword) pair(s), the first: utterance {b}, keyword "
                          f"{self.keywords[k]!r}; the rest were dropped", RuntimeWarning, stacklevel=3)
        for b, utt in enumerate(records):
            self.detections[b] += [r for r in utt if r["final"]]
        return records if frame_seconds is None else add_seconds(records, float(frame_seconds))

    def feed(self, probs, sizes=None, is_log=False, frame_seconds=None):
        """probs (B, T, C) or, with batch 1, (T, C), on the host or the device, as KeywordSpotter.search takes them (probabilities, or
        log-probabilities with is_log=True); sizes: the chunk's valid frames per utterance (0: the utterance has nothing in this chunk).
        Returns, per utterance, the records of search() (frames counted from the stream's first frame) with "final": True for a
        detection that is reported now and never again or changed, False for a tentative one, which every feed reports anew while it
        stands; sorted by (start, end, keyword).  Warns when a keyword had more than max_hits detections to report (final ones take the
        slots first) and when candidates were dropped (a full pending list, a forced cut)."""
        probs, n = self.check_feed(probs, sizes)
        if not probs.is_cuda:
            probs = probs.to(_device("KeywordStream", ".feed"))
        probs = probs.float()
        if probs.stride(2) != 1:
            probs = probs.contiguous()
        return self._call("KeywordStream.feed", probs, n, is_log, False, probs.device, frame_seconds)

    def finish(self, frame_seconds=None):
        """Ends the stream: everything still pending is picked as search() would on the frames consumed, and returned as final records
        per utterance.  A later feed() raises ValueError."""
        if self.closed:
            raise ValueError("KeywordStream.finish: the stream is closed already")
        dev = self._state.device if self._state is not None else _device("KeywordStream", ".finish")
        records = self._call("KeywordStream.finish", None, [0] * self.batch, False, True, dev, frame_seconds)
        self.closed, self._state = True, None
        return records


CONF_MAX_UNIT_LABELS = 63


def confidence_units(text, spans, n_frames, unit="word", margin=0):
    """Pure host half of CTCConfidence.score: a hypothesis `text` (one character per label) and the aligner's (start, end) span of
    every label (end exclusive) -> [(text, lo, hi, start, end)], the units ds2_ctc_conf_f32 scores: the labels [lo, hi) in the frames
    [start, end).  unit="word": the runs of characters between spaces (leading, trailing and doubled spaces make no word), from the
    first label's start to the last label's end; unit="char": every label, the spaces among them.  The window is the span widened by
    `margin` frames on each side and clipped to [0, n_frames]."""
    if unit not in ("word", "char"):
        raise ValueError(f"unit must be 'word' or 'char', got {unit!r}")
    if isinstance(margin, bool) or int(margin) != margin or int(margin) < 0:
        raise ValueError(f"margin must be an integer >= 0, got {margin!r}")
    if len(spans) != len(text):
        raise ValueError(f"confidence_units: {len(spans)} spans for {len(text)} characters")
    margin, n_frames = int(margin), int(n_frames)
    if unit == "char":
        ranges = [(i, i + 1) for i in range(len(text))]
    else:
        ranges, first = [], None
        for i, ch in enumerate(text + " "):
            if ch == " ":
                if first is not None:
                    ranges.append((first, i))
                first = None
            elif first is None:
                first = i
    return [(text[lo:hi], lo, hi, max(int(spans[lo][0]) - margin, 0), min(int(spans[hi - 1][1]) + margin, n_frames)) for lo, hi in ranges]


class CTCConfidence(Decoder):
    """HOW SURE a transcript is of each of its words or characters.  `score` aligns the texts (CTCAligner.align), turns every word or
    character into a unit (its labels, and its span as a frame window) and runs one library call (`ds2_ctc_conf_f32`, contract in
    include/ds2hip.h; restated by tests/ctc_conf_oracle.py): the two lattices of the loss and one short masked backward sweep per unit.
    A unit's confidence is a true conditional probability in [0, 1]: that the whole utterance spells the text, given that the audio
    outside the unit's window spells the rest of the text.  It is exact and needs no calibration set.  The reference has nothing like it.
    NOT MEASURED: how the number calibrates on real recordings (whether the words at 0.9 are right nine times in ten), and which
    `margin` serves them: no margin was tuned, the default 0 takes the aligner's span as it is.  A widened window takes frames from
    its neighbours, which lowers what the frames outside can account for; one that reaches the first or last frame while labels of
    the text remain outside it has no possible context (NaN).  A unit of more than 63 labels is not scored (NaN)."""

    def __init__(self, labels, blank_index=0):
        if blank_index != 0:
            raise ValueError("CTCConfidence: the kernels take class 0 as the blank (blank_index must be 0)")
        super().__init__(labels, blank_index)

    def score(self, probs, sizes, texts, is_log=False, unit="word", margin=0):
        """probs (B,T,C) as decode() takes them (probabilities, or log-probabilities with is_log=True), sizes (B) valid frames or None,
        texts: B strings over the labels.  CTCAligner.align on the same posteriors gives the spans; the units, offsets and lengths go
        up in one pinned upload; one library call; one device-to-host copy.  Returns per utterance {"nll": -log p(text), "units":
        [(text, start, end, confidence)]} (frames, end exclusive: the unit's window; confidence = exp(logconf), NaN for a unit that was
        not scored); an utterance whose alignment is infeasible has "units": [].  Host tensors are uploaded first: there is no CPU
        implementation."""
        from .. import ops
        confidence_units("", [], 0, unit, margin)          # the options, before any work
        probs = torch.as_tensor(probs)
        if probs.dim() != 3:
            raise ValueError(f"CTCConfidence.score: probs must be (B,T,C), got {tuple(probs.shape)}")
        B, T = int(probs.shape[0]), int(probs.shape[1])
        if len(texts) != B or not all(isinstance(t, str) for t in texts):
            raise ValueError(f"CTCConfidence.score: texts must be {B} strings")
        if not probs.is_cuda:
            probs = probs.to(_device("CTCConfidence", ".score"))
        probs = probs.float()
        records = CTCAligner(self.labels).align(probs, sizes, texts, is_log=is_log)
        sizes_h = [T] * B if sizes is None else [int(v) for v in torch.as_tensor(sizes).reshape(-1).tolist()]
        frames = [min(max(n, 0), T) for n in sizes_h]
        targets = encode_transcripts(texts, self.labels)
        units = [confidence_units(texts[b], [(t[1], t[2]) for t in r["tokens"]], frames[b], unit, margin) if r["tokens"] else []
                 for b, r in enumerate(records)]
        lens = [len(t) for t in targets]
        W = max([len(u) for u in units] + [1])
        n_tok, max_u = sum(lens), max(lens, default=0)
        grid = np.zeros((4, B, W), np.int64)
        for b, us in enumerate(units):
            for w, (_, lo, hi, s, e) in enumerate(us):
                grid[:, b, w] = lo, hi, s, e
        # one int32 image: hyp_off (int64, as int32 pairs), hyp_lens, in_lens, n_units, unit_lo / unit_hi / win_start / win_end, labels
        off = np.cumsum([0] + lens[:-1]).astype(np.int64) if B else np.zeros(0, np.int64)
        flat = np.concatenate([off.view(np.int32), lens, frames, [len(u) for u in units], grid.reshape(-1), [i for t in targets for i in t], [0]])   # (a last 0: the label array is never empty)
        d = ops._upload_i32(probs.device, (flat,))[0]
        logits = (probs if is_log else torch.log(probs)).transpose(0, 1).contiguous()
        g0 = 5 * B
        arr = d[g0:g0 + 4 * B * W].view(4, B, W)
        nll, logconf = ops.ctc_confidence(logits, d[g0 + 4 * B * W:], d[:2 * B].view(torch.int64), d[2 * B:3 * B], d[3 * B:4 * B], max_u,
                                          d[4 * B:5 * B], arr[0], arr[1], arr[2], arr[3])
        out = torch.cat((nll, logconf.reshape(-1))).cpu().numpy().astype(np.float64)
        conf = np.exp(out[B:].reshape(B, W))
        return [{"nll": float(out[b]), "units": [(u[0], u[3], u[4], float(conf[b, w])) for w, u in enumerate(us)]} for b, us in enumerate(units)]


def plan_segment_batches(lengths, batch_size):
    """Host half of DeepSpeech.transcribe_long: the segments, given by their lengths, ordered longest first (ties by index) and cut into
    batches of at most batch_size -> a list of index lists.  A batch's t_max is its first segment's length, so a batch pads only up to
    its own longest segment and the decoder's (S, K, t_max) outputs stay bounded."""
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or int(batch_size) < 1:
        raise ValueError(f"plan_segment_batches: batch_size must be a positive integer, got {batch_size!r}")
    lengths = [int(n) for n in lengths]
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    return [order[i:i + int(batch_size)] for i in range(0, len(order), int(batch_size))]


def words_from_offsets(text, offsets, shift=0):
    """A decoded string and its per-character offsets -> [(word, start, end)]: a word is the run of characters between spaces (leading,
    trailing and doubled spaces make no word), start = its first character's offset + shift, end = its last character's offset +
    shift + 1.  The offsets of decode() are the frames where a label was FIRST EMITTED, not spans: a word's end is one past the frame
    where its last character appeared, not where that character's sound ended.  CTCAligner.align() gives spans."""
    offsets = [int(o) for o in (offsets.tolist() if hasattr(offsets, "tolist") else offsets)]
    if len(offsets) != len(text):
        raise ValueError(f"words_from_offsets: {len(offsets)} offsets for {len(text)} characters")
    words, first = [], None
    for i, ch in enumerate(text + " "):
        if ch == " ":
            if first is not None:
                words.append((text[first:i], offsets[first] + shift, offsets[i - 1] + shift + 1))
            first = None
        elif first is None:
            first = i
    return words


def assemble_transcript(texts, offsets, seg_start, seg_end, seg_flags, order, scores=None, frame_seconds=None):
    """Pure host half of DeepSpeech.transcribe_long.  texts / offsets (/ scores): one decoded string, its per-character offsets (frames
    inside the segment) and optionally its score per segment, IN DECODE ORDER; order[i] is the index of the i-th decoded segment in the
    time-ordered arrays seg_start / seg_end / seg_flags (the flattened plan_segment_batches).  Returns {"text": the stripped non-empty
    segment texts joined by single spaces, "segments": [{"start", "end" (global frames, end exclusive), "text" (the decoder's raw
    string), "words": [(word, start, end)] (words_from_offsets, global frames), "forced": flags (1 = starts at a forced cut, 2 = ends at
    one), "score" with scores}]} in time order; with frame_seconds every segment gains "start_s" / "end_s" and every word tuple
    (start_s, end_s)."""
    n = len(seg_start)
    order = [int(i) for i in order]
    if sorted(order) != list(range(n)) or len(texts) != n or len(offsets) != n or (scores is not None and len(scores) != n):
        raise ValueError(f"assemble_transcript: {len(texts)} texts / {len(offsets)} offsets / an order of {len(order)} for {n} segments")
    segments = [None] * n
    for i, k in enumerate(order):
        s, e = int(seg_start[k]), int(seg_end[k])
        rec = {"start": s, "end": e, "text": texts[i], "words": words_from_offsets(texts[i], offsets[i], s), "forced": int(seg_flags[k])}
        if frame_seconds is not None:
            rec["start_s"], rec["end_s"] = s * frame_seconds, e * frame_seconds
            rec["words"] = [w + (w[1] * frame_seconds, w[2] * frame_seconds) for w in rec["words"]]
        if scores is not None:
            rec["score"] = float(scores[i])
        segments[k] = rec
    return {"text": " ".join(t for t in (r["text"].strip() for r in segments) if t), "segments": segments}


def check_segment_options(who, threshold, min_gap, pad, max_len, decode_batch):
    """The argument checks of transcribe_posteriors / DeepSpeech.transcribe_long: ValueError naming the option."""
    from ..ops import _is_int
    if not _is_int(decode_batch, 1):
        raise ValueError(f"{who}: decode_batch must be a positive integer, got {decode_batch!r}")
    if not (0.0 < float(threshold) <= 1.0):              # (NaN fails too)
        raise ValueError(f"{who}: threshold must lie in (0, 1], got {threshold!r}")
    for name, v, lo in (("min_gap", min_gap, 1), ("pad", pad, 0), ("max_len", max_len, 2)):
        if not _is_int(v, lo):
            raise ValueError(f"{who}: {name} must be an integer >= {lo}, got {v!r}")


def transcribe_posteriors(probs, decoder, threshold=0.9, min_gap=25, pad=5, max_len=1000, decode_batch=64, frame_seconds=None):
    """The device half of DeepSpeech.transcribe_long on posteriors you already have: probs (T, C) fp32 probabilities of ONE recording
    (uploaded first if on the host; there is no CPU implementation).  ops.ctc_segment with the decoder's blank, one device-to-host copy
    of the segment list, plan_segment_batches, per batch one ops.ctc_segment_gather and one decoder.decode, assemble_transcript (see
    there for the record; "score" per segment with a BeamCTCDecoder, its best beam's).  The options and what is not measured about
    their defaults: DeepSpeech.transcribe_long."""
    from .. import ops
    check_segment_options("transcribe_posteriors", threshold, min_gap, pad, max_len, decode_batch)
    probs = torch.as_tensor(probs)
    if probs.dim() != 2:
        raise ValueError(f"transcribe_posteriors: probs must be (T, C), got {tuple(probs.shape)}")
    if not probs.is_cuda:
        probs = probs.to(_device("transcribe_posteriors", ""))
    probs = probs.float()
    if probs.stride(1) != 1:
        probs = probs.contiguous()
    probs = probs[None]
    start, end, flags, n_segs = ops.ctc_segment(probs, None, decoder.blank_index, threshold, min_gap, pad, max_len)
    seg = torch.cat((n_segs, start[0], end[0], flags[0])).cpu().numpy()
    n, m = int(seg[0]), start.size(1)
    start_h, end_h, flags_h = seg[1:1 + n], seg[1 + m:1 + m + n], seg[1 + 2 * m:1 + 2 * m + n]
    batches = plan_segment_batches(end_h - start_h, decode_batch)
    beam = isinstance(decoder, BeamCTCDecoder)
    texts, offsets, scores = [], [], [] if beam else None
    for idx in batches:
        host = torch.zeros((3, len(idx)), dtype=torch.int32)          # one int32 image: utterance indices (all 0), starts, lengths
        host[1], host[2] = torch.from_numpy(start_h[idx]), torch.from_numpy(end_h[idx] - start_h[idx])
        d = host.to(probs.device)
        packed, sizes = ops.ctc_segment_gather(probs, d[0], d[1], d[2], int(host[2, 0]))
        strings, offs = decoder.decode(packed, sizes)
        texts += [s[0] for s in strings]
        offsets += [o[0] for o in offs]
        if beam:
            scores += decoder.last_scores[:, 0].tolist()
    return assemble_transcript(texts, offsets, start_h, end_h, flags_h, [i for idx in batches for i in idx], scores, frame_seconds)


def _device(who="GreedyDecoder", what=".decode"):
    from .._lib import DS2LibraryError
    if not torch.cuda.is_available():
        raise DS2LibraryError(f"{who}{what} needs a GPU (no CPU fallback exists)")
    return torch.device("cuda", torch.cuda.current_device())
