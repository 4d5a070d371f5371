// Packed hotword automaton of the CTC beam search's hotword arm (include/ds2hip.h, ds2_ctc_hot_*), shared by the host packer, the
// host stepping function and the kernel, so that the two sides hash, probe and walk alike.  One contiguous blob:
//   HotHeader (64 B) | edge table: tcap TrieEntry | fail: nnodes int32 | phi: nnodes fp32 | terminal: nnodes int32
// The edge table is the open-addressing (node, label) -> child table of ctc_lm.h (trie_hash, linear probing, load <= 1/2) over the
// trie of the phrases; node 0 is the root.  fail[n] is the Aho-Corasick failure link (the longest proper suffix of path(n) that is a
// trie node; fail[0] = 0), phi[n] = depth(n) * max(weight of the phrases through n), terminal[n] != 0 where a phrase ends.
// The packer admits a blob only when every failure link points to a strictly shallower node, so the walk of hot_step ends within
// depth(n) <= MAX_DEPTH steps whatever the table holds.
#pragma once
#include "ctc_lm.h"

namespace ds2hot {

constexpr int MAGIC = 0x31544844;      // "DHT1"
constexpr int MAX_DEPTH = 64;          // labels per phrase
constexpr int MAX_NODES = 1 << 20;     // trie nodes, the root included (1000 phrases of 64 labels need at most 64001)

struct HotHeader {
  int magic, nnodes, tcap, C, nterminal, depth;
  int pad[10];
};

struct HotView {
  const HotHeader* h;
  const ds2lm::TrieEntry* trie;
  const int* fail;
  const float* phi;
  const int* terminal;
};

__host__ __device__ inline size_t hot_bytes(int tcap, int nnodes) {
  return sizeof(HotHeader) + (size_t)tcap * sizeof(ds2lm::TrieEntry) + 12 * (size_t)nnodes;
}

__host__ __device__ inline HotView hot_view(const void* blob) {
  HotView v;
  const char* p = (const char*)blob;
  v.h = (const HotHeader*)p;
  v.trie = (const ds2lm::TrieEntry*)(p + sizeof(HotHeader));
  v.fail = (const int*)(v.trie + v.h->tcap);
  v.phi = (const float*)(v.fail + v.h->nnodes);
  v.terminal = (const int*)(v.phi + v.h->nnodes);
  return v;
}

// the child of `node` along `label`, or -1 (the probing of ds2lm::trie_child)
__host__ __device__ inline int hot_child(const HotView& v, int node, int label) {
  const int mask = v.h->tcap - 1;
  int pos = (int)(ds2lm::trie_hash(node, label) & (ds2lm::u64)mask);
  for (;;) {   // load <= 1/2: an empty slot is always reached
    const ds2lm::TrieEntry e = v.trie[pos];
    if (e.node < 0) return -1;
    if (e.node == node && e.label == label) return e.child;
    pos = (pos + 1) & mask;
  }
}

// One step of the contract from state `node` on `label`: n' = the longest suffix of path(node) + label that is a trie node (the
// root when there is none), term = phi(n') - phi(node) in fp32, next = the root when n' ends a phrase (its len * w stays banked in
// the terms so far), n' otherwise.
__host__ __device__ inline void hot_step(const HotView& v, int node, int label, int& next, float& term) {
  int n = node, ch = hot_child(v, n, label);
  while (ch < 0 && n != 0) {   // every link goes to a strictly shallower node: at most depth(node) rounds
    n = v.fail[n];
    ch = hot_child(v, n, label);
  }
  const int np = ch < 0 ? 0 : ch;
  term = v.phi[np] - v.phi[node];
  next = v.terminal[np] ? 0 : np;
}

}  // namespace ds2hot
