"""Small ARPA files for the language-model tests: a writer and a seeded random model."""
from __future__ import annotations

import gzip

import numpy as np


def write_arpa(path, sections, gz=False, counts=None):
    """sections[k] = list of (tokens tuple, log10 prob, log10 backoff or None) for the (k+1)-grams"""
    counts = counts or [len(s) for s in sections]
    lines = ["", "\\data\\"] + [f"ngram {k + 1}={c}" for k, c in enumerate(counts)] + [""]
    for k, sec in enumerate(sections):
        lines.append(f"\\{k + 1}-grams:")
        for toks, p, b in sec:
            lines.append(f"{p:.6f}\t{' '.join(toks)}" + ("" if b is None else f"\t{b:.6f}"))
        lines.append("")
    lines.append("\\end\\")
    text = "\n".join(lines) + "\n"
    if gz:
        with gzip.open(path, "wt", encoding="utf-8") as f:
            f.write(text)
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
    return path


def random_arpa(path, vocab, order, n_per_order, seed, gz=False):
    """a seeded random model over `vocab` (plus <s>, </s>): every 1-gram, then up to n_per_order random k-grams per higher order,
    which may start with <s>; backoffs on every order below the top, some missing"""
    rng = np.random.default_rng(seed)
    toks = list(vocab)
    uni = [(("<s>",), -99.0, float(rng.uniform(-1, 0))), (("</s>",), float(rng.uniform(-2, -0.5)), None)]
    uni += [((w,), float(rng.uniform(-3, -0.3)), (float(rng.uniform(-1, 0)) if order > 1 and rng.random() < 0.8 else None)) for w in toks]
    sections = [uni]
    for k in range(2, order + 1):
        seen, sec = set(), []
        for _ in range(n_per_order):
            g = tuple(toks[i] for i in rng.integers(0, len(toks), size=k))
            if rng.random() < 0.3:
                g = ("<s>",) + g[1:]
            if g in seen:
                continue
            seen.add(g)
            b = float(rng.uniform(-1, 0)) if k < order and rng.random() < 0.8 else None
            sec.append((g, float(rng.uniform(-3, -0.1)), b))
        sections.append(sec)
    return write_arpa(path, sections, gz=gz)
