"""Hotword phrases for BeamCTCDecoder (contract: include/ds2hip.h, ds2_ctc_beam_decode_hot_f32): the phrases are encoded through the
decoder's labels, checked, and built into the trie with Aho-Corasick failure links and the potentials phi the kernel reads.  Hashing
and packing happen in the library (csrc/ctc_hot.h, ds2_ctc_hot_pack), so the host and the device cannot disagree on them."""
from __future__ import annotations

import ctypes
import math
from collections import deque

import numpy as np

MAX_PHRASE_LABELS = 64


class Hotwords:
    """phrases: an iterable of `str`, `(str, weight)`, a sequence of label ids, or `(ids, weight)`.  labels: {char: id} or a sequence of
    characters; a space in a string is encoded through the space label (`space_index`, by default the label whose character is " ").
    `weight` (per label, natural log, finite, >= 0) is that of every phrase given without one.
    Raises ValueError for an empty phrase, a character outside the labels (named), the blank or an id outside the classes in a phrase,
    a negative or non-finite weight, two phrases equal after encoding, or a phrase that is a proper prefix of another (both named).
    Attributes: `phrases` (tuples of ids), `weights`, the automaton arrays `edges` {(node, label): child}, `fail`, `phi` (fp32),
    `terminal`, `depth`, and `packed` (the host bytes ds2_ctc_beam_decode_hot_f32 reads)."""

    def __init__(self, phrases, labels, blank_index=0, weight=1.0, space_index=None):
        char_to_int = dict(labels) if isinstance(labels, dict) else {c: i for i, c in enumerate(labels)}
        self.C = max(char_to_int.values()) + 1
        self.blank = int(blank_index)
        if space_index is not None:
            char_to_int[" "] = int(space_index)
        self.space = char_to_int.get(" ")
        default = self._weight(weight, "the default")
        self.phrases, self.weights, self.names = [], [], []
        if isinstance(phrases, str):
            phrases = [phrases]
        for n, item in enumerate(phrases):
            w = default
            if isinstance(item, tuple) and len(item) == 2 and not isinstance(item[0], (int, np.integer)) and isinstance(
                    item[1], (int, float, np.integer, np.floating)):
                item, w = item[0], self._weight(item[1], f"phrase {n} ({item[0]!r})")
            name = repr(item if isinstance(item, str) else [int(i) for i in item])
            if isinstance(item, str):
                ids = []
                for ch in item:
                    if ch not in char_to_int:
                        raise ValueError(f"hotword {name}: character {ch!r} is not in the labels")
                    ids.append(int(char_to_int[ch]))
            else:
                ids = [int(i) for i in (item.tolist() if hasattr(item, "tolist") else item)]
            if not ids:
                raise ValueError(f"hotword {n} is empty")
            if len(ids) > MAX_PHRASE_LABELS:
                raise ValueError(f"hotword {name} has {len(ids)} labels, at most {MAX_PHRASE_LABELS} are supported")
            if self.blank in ids:
                raise ValueError(f"hotword {name} contains the blank label {self.blank}")
            if min(ids) < 0 or max(ids) >= self.C:
                raise ValueError(f"hotword {name} has a label id outside 0..{self.C - 1}")
            self.phrases.append(tuple(ids))
            self.weights.append(w)
            self.names.append(name)
        if not self.phrases:
            raise ValueError("a hotword set needs at least one phrase")
        seen = {}
        for n, p in enumerate(self.phrases):
            if p in seen:
                raise ValueError(f"hotwords {self.names[seen[p]]} and {self.names[n]} are equal after encoding")
            seen[p] = n
        for n, p in enumerate(self.phrases):
            for k in range(1, len(p)):
                if p[:k] in seen:
                    raise ValueError(f"hotword {self.names[seen[p[:k]]]} is a proper prefix of {self.names[n]}: the shorter one would "
                                     f"always be credited first; drop one of the two")
        self._build()
        self._pack()
        self._dev = {}

    @staticmethod
    def _weight(w, what):
        w = float(w)
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"hotword weight of {what} must be finite and >= 0, got {w}")
        return w

    def _build(self):
        edges, depth, wmax, terminal = {}, [0], [0.0], [0]
        for p, w in zip(self.phrases, self.weights):
            node = 0
            for c in p:
                nxt = edges.get((node, c))
                if nxt is None:
                    nxt = edges[(node, c)] = len(depth)
                    depth.append(depth[node] + 1)
                    wmax.append(0.0)
                    terminal.append(0)
                node = nxt
                wmax[node] = max(wmax[node], w)
            terminal[node] = 1
        children = {}
        for (a, c), b in edges.items():
            children.setdefault(a, []).append((c, b))
        fail = [0] * len(depth)
        queue = deque(b for _, b in children.get(0, []))
        while queue:                                   # breadth first: a node's link is known before its children's
            a = queue.popleft()
            for c, b in children.get(a, []):
                f = fail[a]
                while f and (f, c) not in edges:
                    f = fail[f]
                fail[b] = edges.get((f, c), 0)
                queue.append(b)
        self.edges, self.depth, self.fail, self.terminal = edges, depth, fail, terminal
        self.phi = (np.array(depth, np.float64) * np.array(wmax, np.float64)).astype(np.float32)
        self.n_nodes = len(depth)

    def _pack(self):
        from .. import _lib
        lib = _lib.load()
        e = np.array([(a, c, b) for (a, c), b in self.edges.items()], dtype=np.int32).reshape(-1, 3)
        nbytes = lib.ds2_ctc_hot_packed_bytes(self.n_nodes, len(e))
        if nbytes == 0:
            raise ValueError(f"the hotwords do not fit the packed automaton ({self.n_nodes} trie nodes)")
        buf = np.zeros(nbytes, dtype=np.uint8)
        ec = [np.ascontiguousarray(e[:, j]) for j in range(3)]
        fail, term = np.array(self.fail, np.int32), np.array(self.terminal, np.int32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        _lib.check(lib.ds2_ctc_hot_pack(self.n_nodes, len(e), ptr(ec[0]), ptr(ec[1]), ptr(ec[2]), ptr(fail), ptr(self.phi), ptr(term),
                                        self.C, ptr(buf), nbytes), "ds2_ctc_hot_pack")
        self.packed = buf

    def step(self, node, label):
        """one step of the automaton by the library's host function (the device's code) -> (next state, fp32 term)"""
        from .. import _lib
        nxt, term = ctypes.c_int(), ctypes.c_float()
        _lib.check(_lib.load().ds2_ctc_hot_step(self.packed.ctypes.data_as(ctypes.c_void_p), int(node), int(label), ctypes.byref(nxt),
                                                ctypes.byref(term)), "ds2_ctc_hot_step")
        return nxt.value, term.value

    def device_tables(self, device):
        """the packed automaton on `device`, uploaded once and cached"""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.packed).to(device)
        return self._dev[key]
