"""Estimate, prune and evaluate the n-gram language models the decoders read: interpolated modified Kneser-Ney from sentences, written as
an ARPA file (contract: include/ds2hip.h, ds2_ngram_*; kernels: csrc/ngram_train.h, csrc/ngram_prune.h).  This module tokenises, numbers
the tokens and writes the file; the counting, the estimation, the pruning and the scoring of held-out text run on the GPU (ops.ngram_*)
or, with device="cpu", in the library's host twins.  Everything downstream (lm.NgramLM, the packed tables, the searches, the rescorer,
the tuner) reads the file.
Pruning (NgramEstimate.prune, estimate_ngram(prune=, min_count=), prune_arpa): a count cut marks the n-grams of order n >= 2 whose raw
count is below min_count[n-1]; an entropy cut marks those whose removal, each judged alone, raises the model's perplexity by less than
the threshold (Stolcke 1998, every quantity from the model being pruned).  A marked n-gram that is the context of a kept one is kept;
kept probabilities stay bit for bit; the backoffs of every context that still has a child are recomputed bottom up so that every
distribution sums to 1; 1-grams are never removed; an order left empty is dropped.  NgramEstimate.perplexity scores held-out
sentences as SRILM's ppl counts them (</s> counted, <s> not).
Byte parity with KenLM's lmplz is not pinned, and neither is parity of the pruning rule with SRILM's -prune or lmplz's --prune (the
tools were not at hand to compare with); the interpolation of several models is not offered."""
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
    n_empty (sentences without tokens, skipped).  A pruned model (prune, prune_arpa) lists the kept n-grams only, and its order is the
    highest order that kept any; one read from a file (prune_arpa) has None for its counts, discounts and corpus figures, and None for
    unk_log10 when the file lists no <unk>."""

    def __init__(self, raw, mode, vocab, n_tokens, n_sentences, n_empty, model=None):
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
        self._raw, self._models = raw, {} if model is None else {str(model["keys"][0].device): model}

    def model(self, device=None):
        """the model as ops.ngram_eval / ngram_prune take it, on `device` (None: the GPU when there is one), uploaded once"""
        from .. import ops
        dev = _device(device)
        if str(dev) not in self._models:
            self._models[str(dev)] = ops.ngram_model(self._raw, dev)
        return self._models[str(dev)]

    def tokens(self, sentences):
        """sentences (strings, split as the model's mode splits them, or sequences of tokens) -> (flat int32 ids, int64 offsets); a token
        outside the vocabulary is <unk> (0)"""
        if isinstance(sentences, str):
            raise ValueError("sentences must be an iterable of strings, not one string")
        ids = {t: i for i, t in enumerate(self.vocab)}
        rows = []
        for s in sentences:
            if isinstance(s, str):
                s = s.split() if self.mode == "word" else [SPACE_TOKEN if c.isspace() else c for c in s]
            rows.append([0 if t in ("<s>", "</s>") else ids.get(t, 0) for t in s])
        lengths = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
        flat = np.fromiter((i for r in rows for i in r), dtype=np.int32, count=int(lengths.sum()))
        offsets = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        return flat, offsets

    def perplexity(self, sentences, device=None):
        """Score held-out sentences (ops.ngram_eval: one lane per token and per </s>) -> {"log10_prob", "n_tokens", "n_sentences", "n_oov",
        "perplexity", "hits"}.  A token outside the model's vocabulary is scored as <unk> and counted in n_oov; hits[n-1] is how many
        positions an n-gram of order n answered.  perplexity = 10 ** (-log10_prob / (n_tokens + n_sentences)), as SRILM's ppl: </s> is
        counted, <s> is not, and an empty sentence is its </s>.  In a model without <unk> such a token has no probability: it is
        counted in n_oov and left out of both the sum and the divisor."""
        import torch
        from .. import ops
        flat, offsets = self.tokens(sentences)
        if len(offsets) < 2:
            raise ValueError("perplexity: no sentence")
        model = self.model(device)
        dev = model["keys"][0].device
        tok = torch.from_numpy(flat).to(dev)
        lp, order = ops.ngram_eval(model, tok, torch.from_numpy(offsets).to(dev))
        scored = order > 0
        total = float(torch.sum(torch.where(scored, lp, torch.zeros_like(lp))))
        hits = torch.bincount(order.clamp(min=0).long(), minlength=self.order + 1).tolist()
        n_tokens, n_sentences = int(flat.size), len(offsets) - 1
        n_scored = n_tokens + n_sentences - hits[0]
        return {"log10_prob": total, "n_tokens": n_tokens, "n_sentences": n_sentences, "n_oov": int((tok == 0).sum()),
                "perplexity": 10.0 ** (-total / n_scored) if n_scored else float("nan"), "hits": hits[1:self.order + 1]}

    def prune(self, threshold=None, min_count=None, device=None):
        """-> a new NgramEstimate without the n-grams of order >= 2 that the count cut (min_count: one integer >= 1 per order,
        non-decreasing, the first ignored; an n-gram whose raw count is below its order's is marked) and then the entropy cut
        (threshold > 0, Stolcke 1998) mark: the module docstring has the rule, ops.ngram_prune the launches.  With neither, or when
        nothing is marked, the same arrays come back."""
        from .. import ops
        if threshold is None and min_count is None:
            return self
        model = self.model(device)
        new = ops.ngram_prune(model, threshold, min_count)
        if new is model:
            return self
        return NgramEstimate(ops.ngram_model_download(new), self.mode, self.vocab, self.n_tokens, self.n_sentences, self.n_empty, model=new)

    def write_arpa(self, path):
        """The model as an ARPA file (gzip when the path ends in .gz): <unk>, <s>, </s> and the tokens by code point, higher orders in
        the order of their tokens' positions in that list; log10 values with 8 decimals, so that reading them as fp32 is the only
        rounding a reader adds."""
        unk = self.unk_log10 is not None
        lines = ["", "\\data\\"] + [f"ngram {n}={len(sec[0]) + (n == 1 and unk)}" for n, sec in enumerate(self.ngrams, 1)] + [""]
        vocab = self.vocab
        for n, (ids, _, _, lp, lb) in enumerate(self.ngrams, 1):
            lines.append(f"\\{n}-grams:")
            if n == 1 and unk:
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


def estimate_ngram(sentences, order=3, mode="word", labels=None, unknown="drop", discount_fallback=(0.5, 1.0, 1.5), device=None, prune=None,
                   min_count=None):
    """An interpolated modified-Kneser-Ney model of `order` (1..6) from sentences -> NgramEstimate.  mode, labels, unknown: see tokenize.
    device: a GPU ("cuda", "cuda:0", a torch.device) runs the HIP kernels; "cpu" the library's host twin, which computes the same model;
    None takes the GPU when there is one.  An order whose n-grams do not fit the kernels' 64-bit key is refused (max_order).
    prune (an entropy threshold) and min_count (count cuts per order): NgramEstimate.prune applied to the estimate."""
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
    dev = _device(device)
    sizes = (int(flat.size), len(offsets) - 1, n_empty)
    if dev.type == "cpu":
        raw = ops.ngram_estimate_host(flat, offsets, len(vocab), order, discount_fallback)
    elif prune is None and min_count is None:
        raw = ops.ngram_estimate(torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), len(vocab), order, discount_fallback)
    else:                                                                # the sorted arrays stay on the device until they are pruned
        st = ops.ngram_count(torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev), len(vocab), order, discount_fallback)
        full = ops.ngram_collect_model(ops.ngram_solve(st))
        kept = ops.ngram_prune(full, prune, min_count)
        return NgramEstimate(ops.ngram_model_download(kept), mode, vocab, *sizes, model=kept)
    return NgramEstimate(raw, mode, vocab, *sizes).prune(prune, min_count, device=dev)


def _device(device):
    """the torch.device of a `device=` argument; None takes the GPU when there is one; "cuda" is named by its index, so that a model
    kept on cuda:0 is found again under every spelling"""
    import torch
    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev


def prune_arpa(src, dst, threshold, device=None):
    """Prune an ARPA file from elsewhere by entropy (NgramEstimate.prune(threshold)) and write the result to dst -> the pruned
    NgramEstimate (without counts).  The tokens are renumbered as the estimator numbers them (<unk>, <s>, </s>, then by code point); a
    file without <unk> simply lists none.  Refused: a model whose order times the bits of one token id exceeds the 64-bit key, an n-gram
    with a token that is no 1-gram, and an n-gram whose context is not listed (the closure could not keep what is not there).  A
    backoff the file lists for <unk> is not kept."""
    from .lm import read_arpa
    if threshold is None:
        raise ValueError("prune_arpa: threshold must be a positive number, got None")
    order, ngrams = read_arpa(src)
    tokens = sorted({toks[0] for toks, _, _ in ngrams[0]} - set(SPECIAL))
    vocab = ["<unk>", "<s>", "</s>"] + tokens
    ids = {t: i for i, t in enumerate(vocab)}
    bits = (len(vocab) - 1).bit_length()
    if order * bits > 64:
        raise ValueError(f"{src}: order {order} over a vocabulary of {len(vocab)} needs {order * bits} bits: it does not fit the 64-bit n-gram key")
    per_order, unk = [], None
    for n, sec in enumerate(ngrams, 1):
        try:
            rows = np.array([[ids[t] for t in toks] for toks, _, _ in sec], dtype=np.uint64).reshape(-1, n)
        except KeyError as e:
            raise ValueError(f"{src}: a {n}-gram has the token {e.args[0]!r}, which is not a 1-gram") from None
        keys = np.zeros(len(rows), np.uint64)
        for j in range(n):
            keys |= rows[:, j] << np.uint64(bits * (n - 1 - j))
        lp = np.array([p for _, p, _ in sec], np.float64)
        lb = np.array([b if b != 0.0 else np.nan for _, _, b in sec], np.float64)      # (read_arpa gives 0 where none is listed: alpha = 1)
        srt = np.argsort(keys, kind="stable")
        keys, lp, lb = keys[srt], lp[srt], lb[srt]
        if len(keys) > 1 and not (keys[1:] > keys[:-1]).all():
            raise ValueError(f"{src}: a {n}-gram is listed twice")
        if n >= 2 and not np.isin(keys >> np.uint64(bits), listed).all():
            raise ValueError(f"{src}: a {n}-gram's context is not listed among the {n - 1}-grams")
        listed = keys
        if n == 1 and len(keys) and keys[0] == 0:
            unk, keys, lp, lb = float(lp[0]), keys[1:], lp[1:], lb[1:]
        per_order.append((keys, None, None, lp, lb))
    raw = {"order": order, "n_vocab": len(vocab), "bits": bits, "orders": per_order, "unk_log10": unk, "discounts": None,
           "count_of_counts": None, "fallback_orders": None}
    mode = "char" if all(len(t) == 1 for t in tokens) else "word"
    est = NgramEstimate(raw, mode, vocab, None, None, None).prune(threshold, device=device)
    est.write_arpa(dst)
    return est


def manifest_sentences(manifest):
    """the `text` column of a manifest CSV (the layout data.write_manifest writes) as a list of strings"""
    import pandas as pd
    df = pd.read_csv(manifest)
    if "text" not in df.columns:
        raise ValueError(f"{manifest}: no `text` column")
    return ["" if t != t else str(t) for t in df["text"].tolist()]
