// N-gram language-model estimation (contract in include/ds2hip.h, ds2_ngram_*; restated in fp64 by tests/ngram_train_oracle.py):
// interpolated modified Kneser-Ney from token ids, the producer of the ARPA files that ctc_lm.h packs and the searches read.
//
// An n-gram is ONE 64-bit key: its tokens in b bits each (b the bit width of n_vocab - 1), oldest token highest, so that the unsigned
// order of the keys of one order is the lexicographic order of the token ids.  Token 0 (<unk>) never occurs in the input, so every
// key is >= 1 and 0 marks an empty slot.  Order n has its own open-addressing table (linear probing, a power of two of slots):
//   keys  slots x u64
//   vals  slots x NgVals: raw count c, distinct left extensions lext, adjusted count adj, and the sums of the entry AS A CONTEXT of
//         order n + 1: S = sum_w a(h w), n1 / n2 / n3 = |{w : a(h w) = 1 / = 2 / >= 3}|
//   prob  slots x (log10 p, log10 backoff or NaN = none), fp64
// and `glob` (NG_GLOB u64 words) holds the flags, the empty context's sums (order 1), the number of distinct 1-grams and the
// count-of-counts t_k of every order.  Everything that is accumulated is an integer, so no result depends on arrival order; which
// slot a key lands in does, and the caller sorts the distinct entries by key before it looks at them.
//
//   ngram_count_kernel    one lane per token position: finds its sentence in `offsets` (binary search), frames it with <s> / </s>
//                         itself, and inserts the n-grams that END at its token for n = 1..N: a 64-bit compare-and-swap claims the
//                         slot, an integer atomic adds the occurrence.  The first token's lane also inserts <s>, the last token's the
//                         n-grams ending in </s>.  A token outside [3, n_vocab) or offsets that do not enclose the position set a flag.
//   ngram_adjust_kernel   one launch per order, N down to 1, one lane per slot: the adjusted count of the entry (its lext is complete
//                         because order n + 1 ran before), +1 on the lext of its suffix, + (a, tallies) on its context's entry, both in
//                         table n - 1, and the count-of-counts by ballot and popcount, one atomic per wave and class.
//   ngram_prob_kernel     one launch per order, 1 up to N, one lane per slot, fp64: p = (a - D) / S(h) + gamma(h) * p_lower(suffix),
//                         the suffix's p read from table n - 1 (the launch before), and the entry's own backoff gamma_{n+1}(entry).
//   ngram_log_kernel      p -> log10 p in place, one launch per order once every order has read the p below it (rounding a logarithm
//                         and raising it again between the orders would cost the fp64 agreement with the host twin).
// Every probe loop runs at most `slots` steps: an insert that finds no room sets NG_OVERFLOW, a lookup that finds no entry sets
// NG_MISSING, and neither spins.  The host sizes the tables so that neither happens; both are reported as errors, not retried.
// Scattered single-lane atomics are the slow shape on this chip (cdna guide, guideline 12) and cannot be avoided for distinct keys;
// merging the duplicates of a wave before the atomic is not done here and its worth is unmeasured.
//
// ds2_ngram_estimate_host is the same estimator in plain C++ over std::unordered_map, through the SAME formula routines
// (ng_discounts, ng_gamma, ng_prob ...), for device="cpu" and for the CPU suite.
#pragma once
#ifndef DS2_NGRAM_TRAIN_TU
#error "ngram_train.h defines the ds2_ngram_* entry points: it is compiled once, as part of decode.hip"
#endif
#include "common.h"
#include <math.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace ds2ng {

typedef unsigned long long u64;
constexpr int MAX_ORDER = 6;
constexpr int UNK = 0, BOS = 1, EOS = 2, FIRST_TOKEN = 3;
constexpr long long MAX_SLOTS = 1ll << 30;
// glob words
constexpr int NG_OVERFLOW = 0, NG_S1 = 1, NG_N1 = 2 /* .. 4 */, NG_BAD_INPUT = 5, NG_MISSING = 6, NG_DISTINCT1 = 7, NG_COC = 8, NG_GLOB = 32;

struct NgVals {
  unsigned c, lext, adj, S, n1, n2, n3, pad;
};
struct NgTable {
  u64* keys;
  NgVals* vals;
  double* prob;   // 2 per slot
  long long slots;
};
struct NgTables {
  NgTable t[MAX_ORDER];
};
struct NgDiscounts {
  double D[MAX_ORDER][4];   // D[n-1][k], D[.][0] = 0
};

__host__ __device__ inline int ng_bits(int n_vocab) {   // bit width of n_vocab - 1
  int b = 0;
  for (unsigned v = (unsigned)(n_vocab - 1); v; v >>= 1) ++b;
  return b;
}
__host__ __device__ inline u64 ng_hash(u64 z) {   // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline u64 ng_suffix(u64 key, int n, int b) { return key & ((1ull << (b * (n - 1))) - 1ull); }   // n >= 2
__host__ __device__ inline u64 ng_context(u64 key, int b) { return key >> b; }
__host__ __device__ inline int ng_first(u64 key, int n, int b) { return (int)(key >> (b * (n - 1))); }
__host__ __device__ inline int ng_last(u64 key, int b) { return (int)(key & ((1ull << b) - 1ull)); }

// a_n(g) from the raw count and the number of distinct left extensions
__host__ __device__ inline unsigned ng_adjusted(u64 key, int n, int N, int b, unsigned c, unsigned lext) {
  if (n == 1 && key == (u64)BOS) return 0u;
  if (n == N || (n >= 2 && ng_first(key, n, b) == BOS)) return c;
  return lext;
}
// gamma(h) of the order whose discounts are D, from the context's sums
__host__ __device__ inline double ng_gamma(const double* D, u64 S, u64 n1, u64 n2, u64 n3) {
  return ((D[1] * (double)n1 + D[2] * (double)n2) + D[3] * (double)n3) / (double)S;
}
// p(w | h) = (a - D_min(a,3)) / S(h) + gamma(h) * lower, lower = p_{n-1}(w | h[1:]); order 1 passes gamma / |V| as gamma with lower = 1
__host__ __device__ inline double ng_prob(const double* D, unsigned a, u64 S, double gamma, double lower) {
  return ((double)a - D[a < 3u ? a : 3u]) / (double)S + gamma * lower;
}
__host__ __device__ inline double ng_log10(double x) { return x > 0.0 ? log10(x) : -99.0; }

// The discounts of one order from its count-of-counts t[0..3] = t_1..t_4; returns 1 when the order falls back
inline int ng_discounts(const long long* t, const double* fallback, double* D) {
  D[0] = 0.0;
  bool ok = t[0] > 0 && t[1] > 0 && t[2] > 0 && t[3] > 0;
  if (ok) {
    const double Y = (double)t[0] / ((double)t[0] + 2.0 * (double)t[1]);
    for (int k = 1; k <= 3; ++k) {
      D[k] = (double)k - (double)(k + 1) * Y * (double)t[k] / (double)t[k - 1];
      ok = ok && D[k] >= 0.0 && D[k] <= (double)k;
    }
  }
  if (!ok)
    for (int k = 1; k <= 3; ++k) D[k] = fallback[k - 1];
  return ok ? 0 : 1;
}

namespace {

constexpr int NG_BLOCK = 256;

__device__ __forceinline__ u64 ng_load_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of `key`, claimed if it is new; -1 when `slots` probes found neither the key nor room (the table is full)
__device__ inline long long ng_insert(u64* keys, long long slots, u64 key) {
  long long i = (long long)(ng_hash(key) & (u64)(slots - 1));
  for (long long probe = 0; probe < slots; ++probe) {
    u64 k = ng_load_key(keys + i);
    if (k == 0ull) k = atomicCAS(keys + i, 0ull, key);   // the old value: 0 = claimed here, `key` = claimed by another lane just now
    if (k == 0ull || k == key) return i;
    i = (i + 1) & (slots - 1);
  }
  return -1;
}
// the slot of `key`, -1 when it is not in the table (an empty slot ends the chain; at most `slots` probes)
__device__ inline long long ng_find(const u64* keys, long long slots, u64 key) {
  long long i = (long long)(ng_hash(key) & (u64)(slots - 1));
  for (long long probe = 0; probe < slots; ++probe) {
    const u64 k = keys[i];
    if (k == key) return i;
    if (k == 0ull) return -1;
    i = (i + 1) & (slots - 1);
  }
  return -1;
}

__device__ __forceinline__ void ng_flag(u64* glob, int which) { atomicOr(glob + which, 1ull); }

__device__ inline void ng_count_one(const NgTable& t, u64 key, u64* glob) {
  const long long i = ng_insert(t.keys, t.slots, key);
  if (i < 0) ng_flag(glob, NG_OVERFLOW);
  else atomicAdd(&t.vals[i].c, 1u);
}

__global__ __launch_bounds__(NG_BLOCK) void ngram_count_kernel(const int* __restrict__ tokens, long long n_tokens,
                                                               const long long* __restrict__ off, long long n_sent, int n_vocab, int N,
                                                               int b, NgTables tabs, u64* __restrict__ glob) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i >= n_tokens) return;
  // the sentence of position i: the largest s in [0, n_sent) with off[s] <= i (empty sentences share their offset with the next one)
  long long lo = 0, hi = n_sent - 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  const long long start = off[lo], end = off[lo + 1];
  if (start < 0 || start > i || end <= i || end > n_tokens) {   // offsets that are not ascending from 0 to n_tokens
    ng_flag(glob, NG_BAD_INPUT);
    return;
  }
  const long long j = i - start;   // the token is framed position j + 1; position 0 is <s>
  // the window of the last N framed positions, newest first; a token outside the vocabulary ends it (and is reported)
  int w[MAX_ORDER];
  int have = 0;
  for (int k = 0; k < N && k <= j + 1; ++k) {
    const int tok = k == j + 1 ? BOS : tokens[i - k];
    if (k <= j && (tok < FIRST_TOKEN || tok >= n_vocab)) {
      ng_flag(glob, NG_BAD_INPUT);
      if (k == 0) return;
      break;
    }
    w[k] = tok;
    have = k + 1;
  }
  u64 key = 0;
  for (int n = 1; n <= have; ++n) {
    key |= (u64)w[n - 1] << (b * (n - 1));
    ng_count_one(tabs.t[n - 1], key, glob);
  }
  if (j == 0) ng_count_one(tabs.t[0], (u64)BOS, glob);
  if (i == end - 1) {   // the n-grams ending in </s>: </s> and the last n - 1 framed positions
    key = (u64)EOS;
    ng_count_one(tabs.t[0], key, glob);
    for (int n = 2; n <= N && n - 2 < have; ++n) {
      key |= (u64)w[n - 2] << (b * (n - 1));
      ng_count_one(tabs.t[n - 1], key, glob);
    }
  }
}

__device__ __forceinline__ u64 ng_wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NG_BLOCK) void ngram_adjust_kernel(NgTable t, NgTable lower, int n, int N, int b, u64* __restrict__ glob) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const u64 key = i < t.slots ? t.keys[i] : 0ull;
  const bool live = key != 0ull;
  unsigned a = 0;
  if (live) {
    const NgVals v = t.vals[i];
    a = ng_adjusted(key, n, N, b, v.c, v.lext);
    t.vals[i].adj = a;
    if (n >= 2) {
      const long long s = ng_find(lower.keys, lower.slots, ng_suffix(key, n, b));
      const long long h = ng_find(lower.keys, lower.slots, ng_context(key, b));
      if (s < 0 || h < 0) ng_flag(glob, NG_MISSING);
      else {
        atomicAdd(&lower.vals[s].lext, 1u);
        if (a > 0u) {
          atomicAdd(&lower.vals[h].S, a);
          atomicAdd(a == 1u ? &lower.vals[h].n1 : a == 2u ? &lower.vals[h].n2 : &lower.vals[h].n3, 1u);
        }
      }
    }
  }
  // per wave: the count-of-counts, and at order 1 the empty context's sums and the number of distinct 1-grams
  for (unsigned k = 1; k <= 4u; ++k) {
    const unsigned long long m = __ballot(live && a == k);
    if (lane == 0 && m) atomicAdd(glob + NG_COC + 4 * (n - 1) + (k - 1), (u64)__popcll(m));
  }
  if (n == 1) {
    const u64 sum = ng_wave_sum(live ? (u64)a : 0ull);
    const unsigned long long m1 = __ballot(live && a == 1u), m2 = __ballot(live && a == 2u), m3 = __ballot(live && a >= 3u),
                             ml = __ballot(live);
    if (lane == 0 && ml) {
      atomicAdd(glob + NG_DISTINCT1, (u64)__popcll(ml));
      if (sum) atomicAdd(glob + NG_S1, sum);
      if (m1) atomicAdd(glob + NG_N1, (u64)__popcll(m1));
      if (m2) atomicAdd(glob + NG_N1 + 1, (u64)__popcll(m2));
      if (m3) atomicAdd(glob + NG_N1 + 2, (u64)__popcll(m3));
    }
  }
}

__global__ __launch_bounds__(NG_BLOCK) void ngram_prob_kernel(NgTable t, NgTable lower, int n, int N, int b, NgDiscounts disc,
                                                              u64* __restrict__ glob) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i >= t.slots) return;
  const u64 key = t.keys[i];
  if (key == 0ull) return;
  const NgVals v = t.vals[i];
  const double* D = disc.D[n - 1];
  double p;
  if (n == 1) {
    const u64 S = glob[NG_S1];
    p = ng_prob(D, v.adj, S, ng_gamma(D, S, glob[NG_N1], glob[NG_N1 + 1], glob[NG_N1 + 2]) / (double)glob[NG_DISTINCT1], 1.0);
  } else {
    const long long s = ng_find(lower.keys, lower.slots, ng_suffix(key, n, b));
    const long long h = ng_find(lower.keys, lower.slots, ng_context(key, b));
    if (s < 0 || h < 0) {
      ng_flag(glob, NG_MISSING);
      return;
    }
    const NgVals c = lower.vals[h];
    // prob[2s] still holds p itself: the launches of ngram_log_kernel turn it into log10 p after every order has read its lower one
    p = ng_prob(D, v.adj, c.S, ng_gamma(D, c.S, c.n1, c.n2, c.n3), lower.prob[2 * s]);
  }
  t.prob[2 * i] = p;
  double bow = NAN;
  if (n < N && ng_last(key, b) != EOS && v.S > 0u) bow = ng_log10(ng_gamma(disc.D[n], v.S, v.n1, v.n2, v.n3));
  t.prob[2 * i + 1] = bow;
}

// p -> log10 p in place, after every order has read its lower order's p; <s> is listed with -99
__global__ __launch_bounds__(NG_BLOCK) void ngram_log_kernel(NgTable t, int n) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i >= t.slots) return;
  const u64 key = t.keys[i];
  if (key == 0ull) return;
  t.prob[2 * i] = (n == 1 && key == (u64)BOS) ? -99.0 : ng_log10(t.prob[2 * i]);
}

int ng_args_check(const char* who, int n_vocab, int order) {
  DS2_REQUIRE(order >= 1 && order <= MAX_ORDER, "%s: the order must be in [1, %d], got %d", who, MAX_ORDER, order);
  DS2_REQUIRE(n_vocab >= FIRST_TOKEN, "%s: n_vocab = %d leaves no room for <unk>, <s> and </s> (ids 0, 1, 2)", who, n_vocab);
  const int b = ng_bits(n_vocab);
  DS2_REQUIRE(order * b <= 64, "%s: an n-gram of order %d over %d ids needs %d bits per token and %d in all; the 64-bit key admits order %d at most",
              who, order, n_vocab, b, order * b, 64 / b);
  return 0;
}

int ng_tables(const char* who, int order, const long long* slots, void* const* keys, void* const* vals, void* const* prob, bool want_prob,
              NgTables* out) {
  DS2_REQUIRE(slots && keys && vals && (prob || !want_prob), "%s: null pointer", who);
  for (int n = 0; n < order; ++n) {
    DS2_REQUIRE(slots[n] >= 2 && slots[n] <= MAX_SLOTS && (slots[n] & (slots[n] - 1)) == 0,
                "%s: the table of order %d must have a power of two of slots in [2, 2^30], got %lld", who, n + 1, slots[n]);
    DS2_REQUIRE(keys[n] && vals[n] && (!want_prob || prob[n]), "%s: null table of order %d", who, n + 1);
    out->t[n] = NgTable{(u64*)keys[n], (NgVals*)vals[n], want_prob ? (double*)prob[n] : nullptr, slots[n]};
  }
  return 0;
}

inline dim3 ng_grid(long long n) { return dim3((unsigned)((n + NG_BLOCK - 1) / NG_BLOCK)); }

}  // namespace
}  // namespace ds2ng

extern "C" int ds2_ngram_max_order(int n_vocab) { return n_vocab < ds2ng::FIRST_TOKEN ? 0 : std::min(ds2ng::MAX_ORDER, 64 / ds2ng::ng_bits(n_vocab)); }
extern "C" int ds2_ngram_glob_words(void) { return ds2ng::NG_GLOB; }

extern "C" int ds2_ngram_count(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                               const long long* slots, void* const* keys, void* const* vals, void* glob, void* stream) {
  using namespace ds2ng;
  if (ng_args_check("ds2_ngram_count", n_vocab, order)) return 1;
  DS2_REQUIRE(n_tokens >= 1 && n_sent >= 1 && n_tokens + 2 * n_sent < 0x7fffffffll,
              "ds2_ngram_count: needs at least one token and fewer than 2^31 framed positions (n_tokens=%lld n_sent=%lld)", n_tokens, n_sent);
  DS2_REQUIRE(tokens && offsets && glob, "ds2_ngram_count: null pointer");
  NgTables tabs;
  if (ng_tables("ds2_ngram_count", order, slots, keys, vals, nullptr, false, &tabs)) return 1;
  hipStream_t s = (hipStream_t)stream;
  DS2_HIP(hipMemsetAsync(glob, 0, sizeof(u64) * NG_GLOB, s));
  for (int n = 0; n < order; ++n) {
    DS2_HIP(hipMemsetAsync(tabs.t[n].keys, 0, sizeof(u64) * (size_t)tabs.t[n].slots, s));
    DS2_HIP(hipMemsetAsync(tabs.t[n].vals, 0, sizeof(NgVals) * (size_t)tabs.t[n].slots, s));
  }
  hipLaunchKernelGGL(ngram_count_kernel, ng_grid(n_tokens), dim3(NG_BLOCK), 0, s, tokens, n_tokens, offsets, n_sent, n_vocab, order,
                     ng_bits(n_vocab), tabs, (u64*)glob);
  DS2_LAUNCH_CHECK("ngram_count_kernel");
  return 0;
}

extern "C" int ds2_ngram_adjust(int n_vocab, int order, const long long* slots, void* const* keys, void* const* vals, void* glob,
                                void* stream) {
  using namespace ds2ng;
  if (ng_args_check("ds2_ngram_adjust", n_vocab, order)) return 1;
  DS2_REQUIRE(glob, "ds2_ngram_adjust: null pointer");
  NgTables tabs;
  if (ng_tables("ds2_ngram_adjust", order, slots, keys, vals, nullptr, false, &tabs)) return 1;
  for (int n = order; n >= 1; --n) {
    hipLaunchKernelGGL(ngram_adjust_kernel, ng_grid(tabs.t[n - 1].slots), dim3(NG_BLOCK), 0, (hipStream_t)stream, tabs.t[n - 1],
                       tabs.t[n >= 2 ? n - 2 : 0], n, order, ng_bits(n_vocab), (u64*)glob);
    DS2_LAUNCH_CHECK("ngram_adjust_kernel");
  }
  return 0;
}

// Host: from a copy of glob, the discounts (order x 4, D[.][0] = 0), which orders fell back, and log10 p(<unk>) = log10(gamma_1 / |V|)
extern "C" int ds2_ngram_discounts(int order, const unsigned long long* glob_host, const double* fallback, double* D, int* fell_back,
                                   long long* coc, double* unk_log10) {
  using namespace ds2ng;
  DS2_REQUIRE(order >= 1 && order <= MAX_ORDER && glob_host && fallback && D && fell_back && coc && unk_log10,
              "ds2_ngram_discounts: bad arguments (order %d)", order);
  for (int k = 0; k < 3; ++k)
    DS2_REQUIRE(fallback[k] >= 0.0 && fallback[k] <= (double)(k + 1), "ds2_ngram_discounts: discount_fallback[%d] = %g is outside [0, %d]", k,
                fallback[k], k + 1);
  DS2_REQUIRE(!glob_host[NG_OVERFLOW], "ds2_ngram: internal error: a counting table overflowed (too few slots)");
  DS2_REQUIRE(!glob_host[NG_BAD_INPUT], "ds2_ngram: a token id outside [3, n_vocab), or offsets that do not ascend from 0 to n_tokens");
  DS2_REQUIRE(!glob_host[NG_MISSING], "ds2_ngram: internal error: a context or suffix of a counted n-gram is in no table");
  DS2_REQUIRE(glob_host[NG_S1] > 0 && glob_host[NG_DISTINCT1] >= 2, "ds2_ngram: internal error: no 1-gram was counted");
  for (int n = 0; n < order; ++n) {
    for (int k = 0; k < 4; ++k) coc[4 * n + k] = (long long)glob_host[NG_COC + 4 * n + k];
    fell_back[n] = ng_discounts(coc + 4 * n, fallback, D + 4 * n);
  }
  *unk_log10 = ng_log10(ng_gamma(D, glob_host[NG_S1], glob_host[NG_N1], glob_host[NG_N1 + 1], glob_host[NG_N1 + 2]) /
                        (double)glob_host[NG_DISTINCT1]);
  return 0;
}

extern "C" int ds2_ngram_probs(int n_vocab, int order, const long long* slots, void* const* keys, void* const* vals, void* const* prob,
                               void* glob, const double* D, void* stream) {
  using namespace ds2ng;
  if (ng_args_check("ds2_ngram_probs", n_vocab, order)) return 1;
  DS2_REQUIRE(glob && D, "ds2_ngram_probs: null pointer");
  NgTables tabs;
  if (ng_tables("ds2_ngram_probs", order, slots, keys, vals, prob, true, &tabs)) return 1;
  NgDiscounts disc;
  for (int n = 0; n < MAX_ORDER; ++n)
    for (int k = 0; k < 4; ++k) disc.D[n][k] = n < order ? D[4 * n + k] : 0.0;
  hipStream_t s = (hipStream_t)stream;
  for (int n = 1; n <= order; ++n) {
    hipLaunchKernelGGL(ngram_prob_kernel, ng_grid(tabs.t[n - 1].slots), dim3(NG_BLOCK), 0, s, tabs.t[n - 1], tabs.t[n >= 2 ? n - 2 : 0], n,
                       order, ng_bits(n_vocab), disc, (u64*)glob);
    DS2_LAUNCH_CHECK("ngram_prob_kernel");
  }
  for (int n = 1; n <= order; ++n) {
    hipLaunchKernelGGL(ngram_log_kernel, ng_grid(tabs.t[n - 1].slots), dim3(NG_BLOCK), 0, s, tabs.t[n - 1], n);
    DS2_LAUNCH_CHECK("ngram_log_kernel");
  }
  return 0;
}

// The host twin: everything above from host arrays, serially.  Outputs per order n (cap[n-1] rows each, n_distinct[n-1] filled, sorted by
// key): keys, count, adjusted, log10 p, log10 backoff (NaN = none); coc (order x 4), D (order x 4), fell_back (order), unk_log10.
extern "C" int ds2_ngram_estimate_host(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab,
                                       int order, const double* fallback, const long long* cap, unsigned long long* const* keys_out,
                                       unsigned* const* count_out, unsigned* const* adjusted_out, double* const* lp_out,
                                       double* const* bow_out, long long* n_distinct, long long* coc, double* D, int* fell_back,
                                       double* unk_log10) {
  using namespace ds2ng;
  if (ng_args_check("ds2_ngram_estimate_host", n_vocab, order)) return 1;
  DS2_REQUIRE(n_tokens >= 1 && n_sent >= 1 && n_tokens + 2 * n_sent < 0x7fffffffll,
              "ds2_ngram_estimate_host: needs at least one token and fewer than 2^31 framed positions (n_tokens=%lld n_sent=%lld)", n_tokens,
              n_sent);
  DS2_REQUIRE(tokens && offsets && fallback && cap && keys_out && count_out && adjusted_out && lp_out && bow_out && n_distinct && coc && D &&
                  fell_back && unk_log10,
              "ds2_ngram_estimate_host: null pointer");
  const int N = order, b = ng_bits(n_vocab);
  struct Entry {
    NgVals v;
    double p, bow;
  };
  std::vector<std::unordered_map<u64, Entry>> tab(N);
  u64 glob[NG_GLOB] = {0};
  DS2_REQUIRE(offsets[0] == 0 && offsets[n_sent] == n_tokens, "ds2_ngram_estimate_host: offsets must run from 0 to n_tokens");
  std::vector<int> framed;
  for (long long s = 0; s < n_sent; ++s) {
    const long long lo = offsets[s], hi = offsets[s + 1];
    DS2_REQUIRE(lo <= hi && hi <= n_tokens, "ds2_ngram_estimate_host: offsets must ascend (sentence %lld)", s);
    if (lo == hi) continue;
    framed.assign(1, BOS);
    for (long long i = lo; i < hi; ++i) {
      DS2_REQUIRE(tokens[i] >= FIRST_TOKEN && tokens[i] < n_vocab, "ds2_ngram_estimate_host: token %lld is %d, outside [3, %d)", i, tokens[i],
                  n_vocab);
      framed.push_back(tokens[i]);
    }
    framed.push_back(EOS);
    for (size_t e = 0; e < framed.size(); ++e) {
      u64 key = 0;
      for (int n = 1; n <= N && (size_t)n <= e + 1; ++n) {
        key |= (u64)framed[e - (n - 1)] << (b * (n - 1));
        ++tab[n - 1][key].v.c;   // (a new Entry is value-initialised: all zero)
      }
    }
  }
  for (int n = N; n >= 1; --n)
    for (auto& kv : tab[n - 1]) {
      NgVals& v = kv.second.v;
      const unsigned a = v.adj = ng_adjusted(kv.first, n, N, b, v.c, v.lext);
      if (a >= 1u && a <= 4u) ++glob[NG_COC + 4 * (n - 1) + (a - 1)];
      if (n >= 2) {
        ++tab[n - 2].at(ng_suffix(kv.first, n, b)).v.lext;
        NgVals& h = tab[n - 2].at(ng_context(kv.first, b)).v;
        h.S += a;
        if (a > 0u) ++(a == 1u ? h.n1 : a == 2u ? h.n2 : h.n3);
      } else {
        ++glob[NG_DISTINCT1];
        glob[NG_S1] += a;
        if (a > 0u) ++glob[NG_N1 + (a < 3u ? a : 3u) - 1];
      }
    }
  if (ds2_ngram_discounts(N, glob, fallback, D, fell_back, coc, unk_log10)) return 1;
  for (int n = 1; n <= N; ++n) {
    const double* Dn = D + 4 * (n - 1);
    for (auto& kv : tab[n - 1]) {
      Entry& e = kv.second;
      if (n == 1) {
        const u64 S = glob[NG_S1];
        e.p = ng_prob(Dn, e.v.adj, S, ng_gamma(Dn, S, glob[NG_N1], glob[NG_N1 + 1], glob[NG_N1 + 2]) / (double)glob[NG_DISTINCT1], 1.0);
      } else {
        const NgVals& c = tab[n - 2].at(ng_context(kv.first, b)).v;
        e.p = ng_prob(Dn, e.v.adj, c.S, ng_gamma(Dn, c.S, c.n1, c.n2, c.n3), tab[n - 2].at(ng_suffix(kv.first, n, b)).p);
      }
      e.bow = NAN;
      if (n < N && ng_last(kv.first, b) != EOS && e.v.S > 0u) e.bow = ng_log10(ng_gamma(D + 4 * n, e.v.S, e.v.n1, e.v.n2, e.v.n3));
    }
  }
  std::vector<u64> order_keys;
  for (int n = 1; n <= N; ++n) {
    const auto& m = tab[n - 1];
    DS2_REQUIRE((long long)m.size() <= cap[n - 1], "ds2_ngram_estimate_host: %zu distinct %d-grams, room for %lld", m.size(), n, cap[n - 1]);
    DS2_REQUIRE(keys_out[n - 1] && count_out[n - 1] && adjusted_out[n - 1] && lp_out[n - 1] && bow_out[n - 1],
                "ds2_ngram_estimate_host: null output of order %d", n);
    order_keys.clear();
    for (const auto& kv : m) order_keys.push_back(kv.first);
    std::sort(order_keys.begin(), order_keys.end());
    n_distinct[n - 1] = (long long)order_keys.size();
    for (size_t r = 0; r < order_keys.size(); ++r) {
      const Entry& e = m.at(order_keys[r]);
      keys_out[n - 1][r] = order_keys[r];
      count_out[n - 1][r] = e.v.c;
      adjusted_out[n - 1][r] = e.v.adj;
      lp_out[n - 1][r] = (n == 1 && order_keys[r] == (u64)BOS) ? -99.0 : ng_log10(e.p);
      bow_out[n - 1][r] = e.bow;
    }
  }
  return 0;
}
