// Packed n-gram language model of the CTC beam search's LM arm (include/ds2hip.h, ds2_ctc_lm_*), shared by the host packer,
// the host scorer and the kernel, so that the two sides hash and look up alike.  One contiguous blob:
//   LmHeader (64 B) | n-gram table: ncap LmEntry | trie table: tcap TrieEntry | node -> word token id: nnodes int32 |
//   label -> token id: C int32
// The n-gram table is open addressing (linear probing, load <= 1/2) keyed by (order n, tokens of the n-gram, oldest first),
// holding log10 prob and log10 backoff (0 when the file has none).  The trie table holds the dictionary's prefix tree over label
// ids (word mode), keyed by (parent node, label) -> child node; node 0 is the root.  Token ids are the 1-grams' positions in the
// file; -1 is "not in the vocabulary".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace ds2lm {

typedef unsigned long long u64;
constexpr int MAX_ORDER = 6;
constexpr int MAGIC = 0x314D4C44;   // "DLM1"
constexpr float OOV = -1000.f;       // log10 score of any n-gram with a token outside the vocabulary
constexpr int MODE_CHAR = 1, MODE_WORD = 2;

struct LmHeader {
  int magic, order, ncap, tcap, nnodes, C, bos, mode;
  int pad[8];
};
struct LmEntry {   // n == 0: empty slot
  int n;
  int tok[MAX_ORDER];
  float prob, bow;
};
struct TrieEntry {   // node < 0: empty slot
  int node, label, child;
};

struct LmView {
  const LmHeader* h;
  const LmEntry* ng;
  const TrieEntry* trie;
  const int* word_of;
  const int* label_tok;
};

__host__ __device__ inline size_t lm_bytes(int ncap, int tcap, int nnodes, int C) {
  return sizeof(LmHeader) + (size_t)ncap * sizeof(LmEntry) + (size_t)tcap * sizeof(TrieEntry) + 4 * ((size_t)nnodes + (size_t)C);
}

__host__ __device__ inline LmView lm_view(const void* blob) {
  LmView v;
  const char* p = (const char*)blob;
  v.h = (const LmHeader*)p;
  v.ng = (const LmEntry*)(p + sizeof(LmHeader));
  v.trie = (const TrieEntry*)(v.ng + v.h->ncap);
  v.word_of = (const int*)(v.trie + v.h->tcap);
  v.label_tok = v.word_of + v.h->nnodes;
  return v;
}

__host__ __device__ inline u64 lm_mix(u64 z) {   // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// hash of the n-gram tok[0..n-1]
__host__ __device__ inline u64 ngram_hash(int n, const int* tok) {
  u64 h = lm_mix((u64)(unsigned)n);
  for (int i = 0; i < n; ++i) h = lm_mix(h ^ (u64)(unsigned)tok[i]);
  return h;
}

// the entry of the n-gram (tok[0..n-1]), or null when it is not listed
__host__ __device__ inline const LmEntry* ngram_find(const LmView& v, int n, const int* tok) {
  const int mask = v.h->ncap - 1;
  int pos = (int)(ngram_hash(n, tok) & (u64)mask);
  for (;;) {   // load <= 1/2: an empty slot is always reached
    const LmEntry* e = v.ng + pos;
    if (e->n == 0) return nullptr;
    if (e->n == n) {
      bool eq = true;
      for (int i = 0; i < n; ++i) eq = eq && e->tok[i] == tok[i];
      if (eq) return e;
    }
    pos = (pos + 1) & mask;
  }
}

__host__ __device__ inline u64 trie_hash(int node, int label) {
  return lm_mix(((u64)(unsigned)node << 32) | (unsigned)label);
}

// the child of `node` along `label`, or -1
__host__ __device__ inline int trie_child(const LmView& v, int node, int label) {
  const int mask = v.h->tcap - 1;
  int pos = (int)(trie_hash(node, label) & (u64)mask);
  for (;;) {
    const TrieEntry e = v.trie[pos];
    if (e.node < 0) return -1;
    if (e.node == node && e.label == label) return e.child;
    pos = (pos + 1) & mask;
  }
}

// backoff of every suffix of the context h[0..m-1]: bow[k] = log10 backoff of (h[k..m-1]), 0 when unlisted or out of vocabulary
__host__ __device__ inline void context_backoffs(const LmView& v, const int* h, int m, float* bow) {
  for (int k = 0; k < m; ++k) {
    bool oov = false;
    for (int i = k; i < m; ++i) oov = oov || h[i] < 0;
    const LmEntry* e = oov ? nullptr : ngram_find(v, m - k, h + k);
    bow[k] = e ? e->bow : 0.f;
  }
}

// lm(w | h), log10, for the context h[0..m-1] (m = order - 1, oldest first) with its suffix backoffs `bow` (context_backoffs):
// the longest listed (h[k..], w) plus the backoffs of the longer contexts; OOV when w or a context token is out of vocabulary.
// At most `order` n-gram probes.
__host__ __device__ inline float cond_score(const LmView& v, const int* h, const float* bow, int m, int w) {
  if (w < 0) return OOV;
  for (int i = 0; i < m; ++i)
    if (h[i] < 0) return OOV;
  int tok[MAX_ORDER];
  for (int i = 0; i < m; ++i) tok[i] = h[i];
  tok[m] = w;
  float acc = 0.f;
  for (int k = 0; k <= m; ++k) {
    const LmEntry* e = ngram_find(v, m + 1 - k, tok + k);
    if (e) return acc + e->prob;
    if (k < m) acc += bow[k];
  }
  return OOV;   // w has no 1-gram: not in the vocabulary
}

}  // namespace ds2lm
