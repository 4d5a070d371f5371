"""N-gram language models in the ARPA text format (plain or .gz) for BeamCTCDecoder's shallow fusion (contract: include/ds2hip.h,
ds2_ctc_beam_decode_lm_f32).  The file is parsed here; hashing and packing into the tables the kernel reads happen in the library
(csrc/ctc_lm.h, ds2_ctc_lm_pack), so the host and the device cannot disagree on them.  KenLM's binary format is not read."""
from __future__ import annotations

import ctypes
import gzip
import re

import numpy as np

MAX_ORDER = 6
SPECIAL = ("<s>", "</s>", "<unk>")
MODE_CHAR, MODE_WORD = 1, 2
_KENLM_MAGIC = b"mmap lm http://kheafield.com/code"
_BINARY_SUFFIXES = (".binary", ".klm")


class ArpaError(ValueError):
    pass


def _reject_binary(path):
    if str(path).endswith(_BINARY_SUFFIXES):
        raise NotImplementedError(f"{path}: KenLM binary language models are not supported; pass the ARPA file (plain or .gz)")


def read_arpa(path):
    """-> (order, ngrams): ngrams[n-1] is a list of (tokens tuple, log10 prob, log10 backoff) in file order."""
    _reject_binary(path)
    with open(path, "rb") as f:
        head = f.read(len(_KENLM_MAGIC))
    if head.startswith(_KENLM_MAGIC):
        raise NotImplementedError(f"{path}: a KenLM binary language model; pass the ARPA file (plain or .gz) instead")
    opener = gzip.open if head[:2] == b"\x1f\x8b" else open
    with opener(path, "rt", encoding="utf-8") as f:
        lines = [ln.strip() for ln in f]
    i = 0
    while i < len(lines) and lines[i] != "\\data\\":
        i += 1
    if i == len(lines):
        raise ArpaError(f"{path}: no \\data\\ section")
    counts = {}
    i += 1
    while i < len(lines) and lines[i]:
        m = re.fullmatch(r"ngram\s+(\d+)\s*=\s*(\d+)", lines[i])
        if not m:
            raise ArpaError(f"{path}:{i + 1}: bad count line {lines[i]!r}")
        counts[int(m.group(1))] = int(m.group(2))
        i += 1
    if not counts or sorted(counts) != list(range(1, len(counts) + 1)):
        raise ArpaError(f"{path}: the \\data\\ counts must list orders 1..N, got {sorted(counts)}")
    order = len(counts)
    if order > MAX_ORDER:
        raise ArpaError(f"{path}: order {order} models are not supported (at most {MAX_ORDER})")
    ngrams = [[] for _ in range(order)]
    n = None
    ended = False
    for j in range(i, len(lines)):
        ln = lines[j]
        if not ln:
            continue
        m = re.fullmatch(r"\\(\d+)-grams:", ln)
        if m:
            n = int(m.group(1))
            if not 1 <= n <= order:
                raise ArpaError(f"{path}:{j + 1}: section {ln} beyond the declared order {order}")
            continue
        if ln == "\\end\\":
            ended = True
            break
        if n is None:
            raise ArpaError(f"{path}:{j + 1}: n-gram line outside an \\N-grams: section")
        parts = ln.split()
        if len(parts) not in (n + 1, n + 2):
            raise ArpaError(f"{path}:{j + 1}: expected {n} tokens, a log10 prob and an optional backoff, got {ln!r}")
        try:
            prob = float(parts[0])
            bow = float(parts[n + 1]) if len(parts) == n + 2 else 0.0
        except ValueError:
            raise ArpaError(f"{path}:{j + 1}: bad number in {ln!r}") from None
        ngrams[n - 1].append((tuple(parts[1:n + 1]), prob, bow))
    if not ended:
        raise ArpaError(f"{path}: no \\end\\ marker")
    for k in range(order):
        if len(ngrams[k]) != counts[k + 1]:
            raise ArpaError(f"{path}: \\data\\ declares {counts[k + 1]} {k + 1}-grams, the file lists {len(ngrams[k])}")
    return order, ngrams


def detect_mode(vocab):
    """character mode when every entry other than <s>, </s>, <unk> is exactly one Unicode character, word mode otherwise"""
    return MODE_CHAR if all(len(w) == 1 for w in vocab if w not in SPECIAL) else MODE_WORD


class NgramLM:
    """A parsed ARPA model bound to a decoder's labels: token ids (the 1-grams' positions in the file), the mode, the word-mode
    dictionary trie over label ids, and the packed tables (`packed`, host bytes) that ds2_ctc_beam_decode_lm_f32 reads."""

    def __init__(self, path, int_to_char, blank, space):
        self.path = path
        self.order, ngrams = read_arpa(path)
        self.vocab = {}
        for toks, _, _ in ngrams[0]:
            if toks[0] in self.vocab:
                raise ArpaError(f"{path}: 1-gram {toks[0]!r} is listed twice")
            self.vocab[toks[0]] = len(self.vocab)
        self.mode = detect_mode(self.vocab)
        C = max(int_to_char) + 1
        self.C, self.blank, self.space = C, blank, space
        if self.mode == MODE_WORD and space is None:
            raise ValueError(f"{path}: a word-level language model needs a space label, and the labels have none")
        rows, n_of, prob, bow = [], [], [], []
        for k, sec in enumerate(ngrams):
            for toks, p, b in sec:
                ids = [self.vocab.get(t, -1) for t in toks]
                if min(ids) < 0:
                    raise ArpaError(f"{path}: {k + 1}-gram {' '.join(toks)!r} has a token that is not a 1-gram")
                rows.append(ids + [-1] * (self.order - k - 1))
                n_of.append(k + 1)
                prob.append(p)
                bow.append(b)
        self.n_ngrams = len(rows)
        # label -> token (character mode), the dictionary trie (word mode)
        self.label_tok = np.full(C, -1, dtype=np.int32)
        char_label = {}
        for i, ch in sorted(int_to_char.items()):
            if i in (blank, space):
                continue
            if self.mode == MODE_CHAR:
                self.label_tok[i] = self.vocab.get(ch, -1)
            char_label.setdefault(ch, i)
        if self.mode == MODE_CHAR and space is not None and 0 <= space < C:
            # no file can list " " (lines are split on whitespace): a character model spells the space as U+2581 (lm_train.SPACE_TOKEN)
            self.label_tok[space] = self.vocab.get(" ", self.vocab.get("▁", -1))
        edges, node_word = {}, [-1]
        self.dictionary = set()
        if self.mode == MODE_WORD:
            for w, tid in self.vocab.items():
                if w in SPECIAL or any(ch not in char_label for ch in w):
                    continue
                self.dictionary.add(w)
                node = 0
                for ch in w:
                    key = (node, char_label[ch])
                    if key not in edges:
                        edges[key] = len(node_word)
                        node_word.append(-1)
                    node = edges[key]
                node_word[node] = tid
        self.n_nodes = len(node_word)
        e = np.array([(a, b, c) for (a, b), c in edges.items()], dtype=np.int32).reshape(-1, 3)
        from .. import _lib
        lib = _lib.load()
        nbytes = lib.ds2_ctc_lm_packed_bytes(self.order, self.n_ngrams, len(e), self.n_nodes, C)
        if nbytes == 0:
            raise ArpaError(f"{path}: the model does not fit the packed tables ({self.n_ngrams} n-grams)")
        buf = np.zeros(nbytes, dtype=np.uint8)
        tok = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, self.order))
        n_of, prob, bow = (np.ascontiguousarray(np.array(x, dtype=t)) for x, t in ((n_of, np.int32), (prob, np.float32), (bow, np.float32)))
        ec = [np.ascontiguousarray(e[:, j]) for j in range(3)]
        nw = np.ascontiguousarray(np.array(node_word, dtype=np.int32))
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        _lib.check(lib.ds2_ctc_lm_pack(self.order, self.n_ngrams, ptr(tok), ptr(n_of), ptr(prob), ptr(bow), len(e), ptr(ec[0]),
                                       ptr(ec[1]), ptr(ec[2]), self.n_nodes, ptr(nw), C, ptr(self.label_tok),
                                       self.vocab.get("<s>", -1), self.mode, ptr(buf), nbytes), "ds2_ctc_lm_pack")
        self.packed = buf
        self._dev = {}

    @property
    def mode_name(self):
        return "char" if self.mode == MODE_CHAR else "word"

    def in_dictionary(self, word):
        return word in self.dictionary

    def score(self, context, word):
        """lm(word | context), log10, by the library's host scorer: context is the last order-1 tokens (strings, oldest first;
        padded on the left with <s> when shorter); a token outside the vocabulary scores -1000."""
        from .. import _lib
        m = self.order - 1
        ctx = (["<s>"] * m + list(context))[len(context):] if m > 0 else []
        h = np.array([self.vocab.get(t, -1) for t in ctx], dtype=np.int32)
        out = ctypes.c_float()
        _lib.check(_lib.load().ds2_ctc_lm_score(self.packed.ctypes.data_as(ctypes.c_void_p), h.ctypes.data_as(ctypes.c_void_p), len(h),
                                                self.vocab.get(word, -1), ctypes.byref(out)), "ds2_ctc_lm_score")
        return out.value

    def device_tables(self, device):
        """the packed tables on `device`, uploaded once and cached"""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.packed).to(device)
        return self._dev[key]
