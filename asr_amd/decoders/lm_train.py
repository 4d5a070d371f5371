"""Estimate the n-gram language models the decoders read: interpolated modified Kneser-Ney from sentences, written as an ARPA file
(contract: include/ds2hip.h, ds2_ngram_*; kernels: csrc/ngram_train.h).  This module tokenises, numbers the tokens and writes the file;
the counting and the estimation run on the GPU (ops.ngram_estimate) or, with device="cpu", in the library's host twin.  Everything
downstream (lm.NgramLM, the packed tables, the searches, the rescorer, the tuner) reads the file.  Byte parity with KenLM's lmplz is
not pinned (the tool was not at hand to compare with); pruning, count thresholds and the interpolation of several models are not offered."""
from __future__ import annotations

import gzip

import numpy as np

from .lm import SPECIAL

SPACE_TOKEN = "▁"   # how a character model spells the space: an ARPA line is split on whitespace, so " " cannot be a token
MODES = ("word", "char")


def max_order(n_vocab):
    """the largest order (at most 6) at which n-grams over n_vocab ids, <unk>, <s> and </s> included, fit the kernels' 64-bit key"""
    from .. import ops
    return ops.ngram_max_order(n_vocab)


def tokenize(sentences, mode="word", labels=None, unknown="drop"):
    """sentences (strings) -> (vocab in file order, flat int32 ids, int64 offsets, n_empty).  Word mode splits on whitespace.  Character
    mode takes every character, whitespace as SPACE_TOKEN; with `labels` (the characters a model emits) a character outside them is
    dropped, as the loaders' parse_transcript does, or raises with unknown="error".  Ids: 0 <unk>, 1 <s>, 2 </s>, then the tokens by
    code point."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if unknown not in ("drop", "error"):
        raise ValueError(f"unknown must be 'drop' or 'error', got {unknown!r}")
    if isinstance(sentences, str):
        raise ValueError("sentences must be an iterable of strings, not one string")
    keep = None
    if mode == "char" and labels is not None:
        chars = list(labels)                                           # (a {char: index} dictionary lists its characters)
        if SPACE_TOKEN in chars:
            raise ValueError(f"the labels hold {SPACE_TOKEN!r} (U+2581) as a label of its own: it is how a character model spells the space")
        keep = {SPACE_TOKEN if c.isspace() else c for c in chars if len(c) == 1}
    rows = []
    for s in sentences:
        if not isinstance(s, str):
            raise ValueError(f"sentences must be strings, got {type(s).__name__}")
        if mode == "word":
            toks = s.split()
        else:
            toks = [SPACE_TOKEN if c.isspace() else c for c in s]
            if keep is not None:
                if unknown == "error" and any(c not in keep for c in toks):
                    raise ValueError(f"a character of {s!r} is outside the labels")
                toks = [c for c in toks if c in keep]
        rows.append(toks)
    tokens = sorted(set().union(*rows)) if rows else []
    clash = [t for t in tokens if t in SPECIAL]
    if clash:
        raise ValueError(f"the text holds the reserved token {clash[0]!r}")
    vocab = ["<unk>", "<s>", "</s>"] + tokens
    ids = {t: i for i, t in enumerate(vocab)}
    lengths = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    flat = np.fromiter((ids[t] for r in rows for t in r), dtype=np.int32, count=int(lengths.sum()))
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return vocab, flat, offsets, int((lengths == 0).sum())


class NgramEstimate:
    """An estimated model.  order, mode; vocab in file order (a token's id is its position: <unk>, <s>, </s>, then the tokens by code
    point); ngrams[n-1] = (ids (count, n) int32, count, adjusted, log10_prob, log10_backoff) over the counted n-grams in file order
    (log10_backoff NaN where the file lists none); unk_log10 the listed log10 p(<unk>); discounts (order, 3), count_of_counts (order, 4),
    fallback_orders (the orders whose closed-form discounts did not exist and that took discount_fallback); n_tokens, n_sentences,
    n_empty (sentences without tokens, skipped)."""

    def __init__(self, raw, mode, vocab, n_tokens, n_sentences, n_empty):
        self.order, self.mode, self.vocab = raw["order"], mode, vocab
        b, mask = raw["bits"], np.uint64((1 << raw["bits"]) - 1)
        self.ngrams = []
        for n, (keys, count, adjusted, lp, lb) in enumerate(raw["orders"], 1):
            ids = np.stack([((keys >> np.uint64(b * (n - 1 - j))) & mask).astype(np.int32) for j in range(n)], axis=1) if len(keys) \
                else np.zeros((0, n), np.int32)
            self.ngrams.append((ids, count, adjusted, lp, lb))
        self.unk_log10 = raw["unk_log10"]
        self.discounts, self.count_of_counts, self.fallback_orders = raw["discounts"], raw["count_of_counts"], raw["fallback_orders"]
        self.n_tokens, self.n_sentences, self.n_empty = n_tokens, n_sentences, n_empty

    def write_arpa(self, path):
        """The model as an ARPA file (gzip when the path ends in .gz): <unk>, <s>, </s> and the tokens by code point, higher orders in
        the order of their tokens' positions in that list; log10 values with 8 decimals, so that reading them as fp32 is the only
        rounding a reader adds."""
        lines = ["", "\\data\\"] + [f"ngram {n}={len(sec[0]) + (n == 1)}" for n, sec in enumerate(self.ngrams, 1)] + [""]
        vocab = self.vocab
        for n, (ids, _, _, lp, lb) in enumerate(self.ngrams, 1):
            lines.append(f"\\{n}-grams:")
            if n == 1:
                lines.append(f"{self.unk_log10:.8f}\t<unk>")
            for row, p, b in zip(ids.tolist(), lp.tolist(), lb.tolist()):
                text = " ".join([vocab[i] for i in row])
                lines.append(f"{p:.8f}\t{text}" if b != b else f"{p:.8f}\t{text}\t{b:.8f}")
            lines.append("")
        lines.append("\\end\\")
        data = ("\n".join(lines) + "\n").encode("utf-8")
        if str(path).endswith(".gz"):
            with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:   # (no timestamp: equal models, equal bytes)
                g.write(data)
        else:
            with open(path, "wb") as f:
                f.write(data)
        return path


def estimate_ngram(sentences, order=3, mode="word", labels=None, unknown="drop", discount_fallback=(0.5, 1.0, 1.5), device=None):
    """An interpolated modified-Kneser-Ney model of `order` (1..6) from sentences -> NgramEstimate.  mode, labels, unknown: see tokenize.
    device: a GPU ("cuda", "cuda:0", a torch.device) runs the HIP kernels; "cpu" the library's host twin, which computes the same model;
    None takes the GPU when there is one.  An order whose n-grams do not fit the kernels' 64-bit key is refused (max_order)."""
    import torch
    from .. import ops
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 6:
        raise ValueError(f"order must be an integer in [1, 6], got {order!r}")
    vocab, flat, offsets, n_empty = tokenize(sentences, mode, labels, unknown)
    if flat.size == 0:
        raise ValueError("the sentences hold no token")
    top = max_order(len(vocab))
    if order > top:
        raise ValueError(f"order {order} over a vocabulary of {len(vocab)} does not fit the 64-bit n-gram key: at most order {top}")
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if dev.type == "cpu":
        raw = ops.ngram_estimate_host(flat, offsets, len(vocab), order, discount_fallback)
    else:
        raw = ops.ngram_estimate(torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), len(vocab), order, discount_fallback)
    return NgramEstimate(raw, mode, vocab, int(flat.size), len(offsets) - 1, n_empty)


def manifest_sentences(manifest):
    """the `text` column of a manifest CSV (the layout data.write_manifest writes) as a list of strings"""
    import pandas as pd
    df = pd.read_csv(manifest)
    if "text" not in df.columns:
        raise ValueError(f"{manifest}: no `text` column")
    return ["" if t != t else str(t) for t in df["text"].tolist()]
