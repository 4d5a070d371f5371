// N-gram model evaluation and pruning (contract in include/ds2hip.h, ds2_ngram_eval / ds2_ngram_prune_*; restated in fp64 by
// tests/ngram_prune_oracle.py).  Everything works on the estimator's representation (ngram_train.h): per order n the listed n-grams as
// 64-bit keys in ascending order, with log10 p and log10 backoff (NaN = none) beside them.  A lookup is a binary search, bounded by
// log2 of the array; nothing here probes, spins or adds with an atomic.
//
//   pr_logp               log10 p_M(w | h): the listed (m+1)-gram, else backoff(h) + the same one token shorter; OOV at m = 0.
//   ngram_eval_kernel     one lane per scored position of the framed sentences (every token and every </s>): log10 p and the order hit.
//   ngram_prune_sums_kernel / _cross_kernel
//                         for the n-grams of one order, per context h (their keys without the last token): sum p and sum q over the
//                         children of h, q = p_M(w | h[1:]).  The children are contiguous.  A lane per n-gram computes (p, q); a
//                         segmented scan over the wave adds them in lane order; a segment that lies within one wave is finished there, a
//                         segment that crosses waves leaves one partial per wave, and the second launch adds those partials with one
//                         wave per crossing segment (strided, then a fixed butterfly).  The order of every addition is a function of
//                         the keys alone, so equal arrays give equal bits.
//   ngram_prune_entropy_kernel   one launch, a lane per n-gram of every order >= 2: P(h), alpha' and the relative perplexity change
//                         exp(dH) - 1 of removing that n-gram alone (Stolcke 1998); marks it when the change is below the threshold.
//   ngram_prune_closure_kernel   one launch per order, top down: a kept n-gram clears the mark of its context.
//   ngram_prune_backoff_kernel   one launch per order, bottom up: backoff(h) = (1 - sum p) / (1 - sum q) over the kept children.
// The host twins (ds2_*_host, also what device="cpu" runs) loop over the same per-entry routines (pr_logp, pr_value, pr_backoff ...).
#pragma once
#ifndef DS2_NGRAM_TRAIN_TU
#error "ngram_prune.h defines the ds2_ngram_eval / ds2_ngram_prune_* entry points: it is compiled once, after ngram_train.h, as part of decode.hip"
#endif
#include "common.h"
#include <math.h>

namespace ds2ng {

struct PrModel {
  const u64* keys[MAX_ORDER];
  const double* lp[MAX_ORDER];
  const double* lb[MAX_ORDER];
  long long cnt[MAX_ORDER];
  int N, b;
};
// what the pruning launches read and write beside the model; index n - 1 belongs to the n-grams of order n
struct PrWork {
  const double* q[MAX_ORDER];     // cnt[n-1]: p_M(w | h[1:]) of each n-gram
  const double* sp[MAX_ORDER];    // cnt[n-2]: per context row of order n - 1, the sum of p over its children of order n (NaN: no child)
  const double* sq[MAX_ORDER];    // cnt[n-2]: the sum of q over the same children
  double* val[MAX_ORDER];         // cnt[n-1]: exp(dH) - 1
  unsigned char* mark[MAX_ORDER]; // cnt[n-1]: 1 = marked for removal
};

// the first row of the ascending keys with keys[row] >= key (cnt when there is none); at most log2(cnt) + 1 steps
__host__ __device__ inline long long pr_lower(const u64* keys, long long cnt, u64 key) {
  long long lo = 0, hi = cnt;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// the row of `key`, -1 when it is not listed
__host__ __device__ inline long long pr_find(const u64* keys, long long cnt, u64 key) {
  const long long r = pr_lower(keys, cnt, key);
  return (r < cnt && keys[r] == key) ? r : -1;
}
// the newest k tokens of a key, k <= N - 1 (so k * b < 64: no shift here is by 64)
__host__ __device__ inline u64 pr_low(u64 key, int k, int b) { return k > 0 ? key & ((1ull << (k * b)) - 1ull) : 0ull; }
__host__ __device__ inline double pr_pow10(double x) { return pow(10.0, x); }

// log10 p_M(w | h), h the key of m <= N - 1 tokens: the backoffs on the way down are added first, the listed log10 p last.
// *order: the order of the n-gram that was listed, 0 when w is not even a 1-gram (OOV: NaN is returned)
__host__ __device__ inline double pr_logp(const PrModel& M, u64 h, int m, int w, int* order) {
  double acc = 0.0;
  for (int k = m; k >= 0; --k) {
    const u64 ctx = pr_low(h, k, M.b);
    const long long r = pr_find(M.keys[k], M.cnt[k], (ctx << M.b) | (u64)w);
    if (r >= 0) {
      *order = k + 1;
      return acc + M.lp[k][r];
    }
    if (k == 0) break;
    const long long hr = pr_find(M.keys[k - 1], M.cnt[k - 1], ctx);
    if (hr >= 0) {
      const double bo = M.lb[k - 1][hr];
      if (bo == bo) acc += bo;
    }
  }
  *order = 0;
  return NAN;
}

// log10 P(h) = sum_i log10 p_M(h_i | h_1 .. h_{i-1}), h of m >= 1 tokens; a leading <s> is scored as p_M(</s>)
__host__ __device__ inline double pr_log_history(const PrModel& M, u64 h, int m) {
  const u64 mask = (1ull << M.b) - 1ull;
  double acc = 0.0;
  for (int i = 1; i <= m; ++i) {
    const u64 pre = h >> (M.b * (m - i + 1));   // h_1 .. h_{i-1}: a shift by at most b * m <= 64 - b
    int w = (int)((h >> (M.b * (m - i))) & mask), ord;
    if (i == 1 && w == BOS) w = EOS;
    acc += pr_logp(M, pre, i - 1, w, &ord);
  }
  return acc;
}

// exp(dH) - 1 of removing h w alone: p, q as above, sp / sq the sums over h's children, alpha h's backoff, Ph = P(h)
__host__ __device__ inline double pr_value(double p, double q, double sp, double sq, double alpha, double Ph) {
  const double num = 1.0 - sp, den = 1.0 - sq;
  const double la = log((num + p) / (den + q));
  const double dH = -Ph * (p * ((log(q) + la) - log(p)) + num * (la - log(alpha)));
  return expm1(dH);
}
__host__ __device__ inline double pr_backoff(double sp, double sq) { return ng_log10((1.0 - sp) / (1.0 - sq)); }

// (p, q) of row r of order n >= 2
__host__ __device__ inline void pr_pq(const PrModel& M, int n, long long r, double* p, double* q) {
  const u64 key = M.keys[n - 1][r];
  int ord;
  *p = pr_pow10(M.lp[n - 1][r]);
  *q = pr_pow10(pr_logp(M, pr_low(key >> M.b, n - 2, M.b), n - 2, ng_last(key, M.b), &ord));
}

// the value of row r of order n >= 2 and whether it is marked; an n-gram whose context is not listed is never marked (value NaN)
__host__ __device__ inline void pr_entropy_one(const PrModel& M, const PrWork& W, int n, long long r, double theta) {
  const u64 key = M.keys[n - 1][r], h = key >> M.b;
  const long long hr = pr_find(M.keys[n - 2], M.cnt[n - 2], h);
  double v = NAN;
  if (hr >= 0) {
    const double bo = M.lb[n - 2][hr];
    v = pr_value(pr_pow10(M.lp[n - 1][r]), W.q[n - 1][r], W.sp[n - 1][hr], W.sq[n - 1][hr], bo == bo ? pr_pow10(bo) : 1.0,
                 pr_pow10(pr_log_history(M, h, n - 1)));
  }
  W.val[n - 1][r] = v;
  W.mark[n - 1][r] = v < theta ? 1 : 0;
}

// the scored position i of the framed sentences: sentence s owns positions off[s] + s .. off[s+1] + s (its tokens, then </s>)
__host__ __device__ inline void pr_eval_one(const PrModel& M, const int* tokens, long long n_tokens, const long long* off, long long n_sent,
                                            int n_vocab, long long i, double* out_lp, int* out_order) {
  long long lo = 0, hi = n_sent - 1;   // the largest s with off[s] + s <= i (strictly ascending, empty sentences included)
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (off[mid] + mid <= i) lo = mid;
    else hi = mid - 1;
  }
  const long long start = off[lo], end = off[lo + 1], j = i - start - lo;
  out_lp[i] = NAN;
  out_order[i] = -1;
  if (start < 0 || end < start || end > n_tokens || j < 0 || j > end - start) return;   // offsets that do not ascend from 0 to n_tokens
  out_order[i] = 0;
  const int tok = j < end - start ? tokens[start + j] : EOS;
  if (tok < 0 || tok >= n_vocab) return;
  u64 h = 0;
  int m = 0;
  for (int k = 1; k < M.N && k <= j + 1; ++k) {   // the context, newest token lowest; an id outside the vocabulary ends it
    const int t = k == j + 1 ? BOS : tokens[start + j - k];
    if (t < 0 || t >= n_vocab) break;
    h |= (u64)t << (M.b * (k - 1));
    m = k;
  }
  int ord;
  out_lp[i] = pr_logp(M, h, m, tok, &ord);
  out_order[i] = ord;
}

namespace {

__global__ __launch_bounds__(NG_BLOCK) void ngram_eval_kernel(PrModel M, const int* __restrict__ tokens, long long n_tokens,
                                                              const long long* __restrict__ off, long long n_sent, int n_vocab,
                                                              double* __restrict__ out_lp, int* __restrict__ out_order) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i < n_tokens + n_sent) pr_eval_one(M, tokens, n_tokens, off, n_sent, n_vocab, i, out_lp, out_order);
}

// part: 4 doubles per wave of this launch: (sum p, sum q) of the segment that came in from the wave before, and of the segment that
// starts in this wave and goes on into the next
__global__ __launch_bounds__(NG_BLOCK) void ngram_prune_sums_kernel(PrModel M, int n, double* __restrict__ q_out, double* __restrict__ sp,
                                                                    double* __restrict__ sq, double* __restrict__ part) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const long long cnt = M.cnt[n - 1];
  const u64* keys = M.keys[n - 1];
  const bool live = i < cnt;
  const u64 ctx = live ? keys[i] >> M.b : 0ull;
  double p = 0.0, q = 0.0;
  if (live) {
    pr_pq(M, n, i, &p, &q);
    if (q_out) q_out[i] = q;
  }
  const bool head = live && (i == 0 || (keys[i - 1] >> M.b) != ctx);         // the context's first child
  const bool tail = live && (i == cnt - 1 || (keys[i + 1] >> M.b) != ctx);   // and its last
  // inclusive segmented scan in lane order; `th`: the segment this lane belongs to starts in this wave
  int f = (head || lane == 0 || !live) ? 1 : 0, th = head ? 1 : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double p2 = __shfl_up(p, d, 64), q2 = __shfl_up(q, d, 64);
    const int f2 = __shfl_up(f, d, 64), th2 = __shfl_up(th, d, 64);
    if (lane >= d && !f) {
      p = p2 + p;
      q = q2 + q;
      f = f2;
      th = th2;
    }
  }
  if (!live || !(tail || lane == 63)) return;   // the last lane of each segment within the wave goes on
  const long long wave = i >> 6;
  if (th && tail) {
    const long long r = pr_find(M.keys[n - 2], M.cnt[n - 2], ctx);
    if (r >= 0) {
      sp[r] = p;
      sq[r] = q;
    }
  } else {
    const int slot = th ? 2 : 0;
    part[4 * wave + slot] = p;
    part[4 * wave + slot + 1] = q;
  }
}

// one wave per wave w0 of the launch above: when a segment starts in w0 and goes on, add its partials
__global__ __launch_bounds__(NG_BLOCK) void ngram_prune_sums_cross_kernel(PrModel M, int n, double* __restrict__ sp, double* __restrict__ sq,
                                                                          const double* __restrict__ part) {
  const long long w0 = ((long long)blockIdx.x * NG_BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const long long cnt = M.cnt[n - 1];
  const u64* keys = M.keys[n - 1];
  if (w0 * 64 >= cnt) return;
  const long long e = (w0 * 64 + 63 < cnt ? w0 * 64 + 63 : cnt - 1);   // the wave's last row
  if (e + 1 >= cnt) return;
  const u64 ctx = keys[e] >> M.b;
  if ((keys[e + 1] >> M.b) != ctx) return;
  if (pr_lower(keys, cnt, ctx << M.b) < w0 * 64) return;                // it started in an earlier wave: that wave's job
  // the row after the segment: the first whose context is larger (ctx + 1 may not fit the key, so search on the context itself)
  long long lo = e + 1, hi = cnt;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if ((keys[mid] >> M.b) <= ctx) lo = mid + 1;
    else hi = mid;
  }
  const long long w1 = (lo - 1) >> 6;
  double p = 0.0, q = 0.0;
  for (long long k = w0 + 1 + lane; k <= w1; k += 64) {
    p += part[4 * k];
    q += part[4 * k + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    p += __shfl_xor(p, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (lane != 0) return;
  const long long r = pr_find(M.keys[n - 2], M.cnt[n - 2], ctx);
  if (r >= 0) {
    sp[r] = part[4 * w0 + 2] + p;
    sq[r] = part[4 * w0 + 3] + q;
  }
}

__global__ __launch_bounds__(NG_BLOCK) void ngram_prune_entropy_kernel(PrModel M, PrWork W, double theta) {
  long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  for (int n = 2; n <= M.N; ++n) {
    if (i < M.cnt[n - 1]) {
      pr_entropy_one(M, W, n, i, theta);
      return;
    }
    i -= M.cnt[n - 1];
  }
}

// a kept n-gram of order n keeps its context (order n - 1) as well; every lane that writes, writes 0
__global__ __launch_bounds__(NG_BLOCK) void ngram_prune_closure_kernel(PrModel M, int n, const unsigned char* __restrict__ mark,
                                                                       unsigned char* __restrict__ mark_ctx) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i >= M.cnt[n - 1] || mark[i]) return;
  const long long r = pr_find(M.keys[n - 2], M.cnt[n - 2], M.keys[n - 1][i] >> M.b);
  if (r >= 0) mark_ctx[r] = 0;
}

__global__ __launch_bounds__(NG_BLOCK) void ngram_prune_backoff_kernel(long long cnt, const double* __restrict__ sp,
                                                                       const double* __restrict__ sq, double* __restrict__ lb) {
  const long long i = (long long)blockIdx.x * NG_BLOCK + threadIdx.x;
  if (i >= cnt) return;
  const double a = sp[i];
  lb[i] = a == a ? pr_backoff(a, sq[i]) : NAN;
}

int pr_model(const char* who, int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, PrModel* M) {
  DS2_REQUIRE(order >= 1 && order <= MAX_ORDER, "%s: the order must be in [1, %d], got %d", who, MAX_ORDER, order);
  DS2_REQUIRE(n_vocab >= FIRST_TOKEN, "%s: n_vocab = %d leaves no room for <unk>, <s> and </s> (ids 0, 1, 2)", who, n_vocab);
  const int b = ng_bits(n_vocab);
  DS2_REQUIRE(order * b <= 64, "%s: an n-gram of order %d over %d ids needs %d bits; the 64-bit key admits order %d at most", who, order, n_vocab,
              order * b, 64 / b);
  DS2_REQUIRE(cnt && keys && lp && lb, "%s: null pointer", who);
  *M = PrModel{};
  M->N = order;
  M->b = b;
  for (int n = 0; n < order; ++n) {
    DS2_REQUIRE(cnt[n] >= 0 && cnt[n] < 0x7fffffffll * NG_BLOCK, "%s: %lld %d-grams", who, cnt[n], n + 1);
    DS2_REQUIRE(cnt[n] == 0 || (keys[n] && lp[n] && lb[n]), "%s: null array of order %d", who, n + 1);
    M->keys[n] = (const u64*)keys[n];
    M->lp[n] = (const double*)lp[n];
    M->lb[n] = (const double*)lb[n];
    M->cnt[n] = cnt[n];
  }
  return 0;
}

int pr_eval_args(const char* who, const void* tokens, long long n_tokens, const void* offsets, long long n_sent, const void* out_lp,
                 const void* out_order) {
  DS2_REQUIRE(n_tokens >= 0 && n_sent >= 1 && n_tokens + n_sent < 0x7fffffffll,
              "%s: needs at least one sentence and fewer than 2^31 scored positions (n_tokens=%lld n_sent=%lld)", who, n_tokens, n_sent);
  DS2_REQUIRE((tokens || n_tokens == 0) && offsets && out_lp && out_order, "%s: null pointer", who);
  return 0;
}

int pr_sums_args(const char* who, const PrModel& M, int n, const void* sp, const void* sq, const void* scratch, long long scratch_doubles,
                 bool device) {
  DS2_REQUIRE(n >= 2 && n <= M.N, "%s: the children's order must be in [2, %d], got %d", who, M.N, n);
  DS2_REQUIRE(M.cnt[n - 2] == 0 || (sp && sq), "%s: null pointer", who);
  DS2_REQUIRE(!device || M.cnt[n - 1] == 0 || (scratch && scratch_doubles >= 4 * ((M.cnt[n - 1] + 63) / 64)),
              "%s: the scratch must hold 4 doubles per 64 n-grams of order %d", who, n);
  return 0;
}

int pr_work(const char* who, const PrModel& M, void* const* q, void* const* sp, void* const* sq, void* const* val, void* const* mark,
            double theta, PrWork* W) {
  DS2_REQUIRE(theta > 0.0, "%s: the threshold must be positive, got %g", who, theta);
  DS2_REQUIRE(q && sp && sq && val && mark, "%s: null pointer", who);
  *W = PrWork{};
  for (int n = 1; n < M.N; ++n) {
    DS2_REQUIRE(M.cnt[n] == 0 || (q[n] && sp[n] && sq[n] && val[n] && mark[n]), "%s: null array of order %d", who, n + 1);
    W->q[n] = (const double*)q[n];
    W->sp[n] = (const double*)sp[n];
    W->sq[n] = (const double*)sq[n];
    W->val[n] = (double*)val[n];
    W->mark[n] = (unsigned char*)mark[n];
  }
  return 0;
}

}  // namespace
}  // namespace ds2ng

extern "C" int ds2_ngram_eval(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                              const long long* cnt, void* const* keys, void* const* lp, void* const* lb, double* out_lp, int* out_order,
                              void* stream) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_eval", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_eval_args("ds2_ngram_eval", tokens, n_tokens, offsets, n_sent, out_lp, out_order)) return 1;
  hipLaunchKernelGGL(ngram_eval_kernel, ng_grid(n_tokens + n_sent), dim3(NG_BLOCK), 0, (hipStream_t)stream, M, tokens, n_tokens, offsets, n_sent,
                     n_vocab, out_lp, out_order);
  DS2_LAUNCH_CHECK("ngram_eval_kernel");
  return 0;
}

extern "C" int ds2_ngram_eval_host(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                                   const long long* cnt, void* const* keys, void* const* lp, void* const* lb, double* out_lp,
                                   int* out_order) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_eval_host", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_eval_args("ds2_ngram_eval_host", tokens, n_tokens, offsets, n_sent, out_lp, out_order)) return 1;
  for (long long i = 0; i < n_tokens + n_sent; ++i) pr_eval_one(M, tokens, n_tokens, offsets, n_sent, n_vocab, i, out_lp, out_order);
  return 0;
}

// Sums over the children of order n, per context row of order n - 1: sp, sq (NaN where a context has no child); q_out (may be null): q
// of every child.  scratch: 4 doubles per 64 children.
extern "C" int ds2_ngram_prune_sums(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, int n,
                                    double* q_out, double* sp, double* sq, double* scratch, long long scratch_doubles, void* stream) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_prune_sums", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_sums_args("ds2_ngram_prune_sums", M, n, sp, sq, scratch, scratch_doubles, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (M.cnt[n - 2] > 0) {
    DS2_HIP(hipMemsetAsync(sp, 0xFF, sizeof(double) * (size_t)M.cnt[n - 2], s));   // all bits set is a NaN: "no child"
    DS2_HIP(hipMemsetAsync(sq, 0xFF, sizeof(double) * (size_t)M.cnt[n - 2], s));
  }
  if (M.cnt[n - 1] == 0) return 0;
  hipLaunchKernelGGL(ngram_prune_sums_kernel, ng_grid(M.cnt[n - 1]), dim3(NG_BLOCK), 0, s, M, n, q_out, sp, sq, scratch);
  DS2_LAUNCH_CHECK("ngram_prune_sums_kernel");
  hipLaunchKernelGGL(ngram_prune_sums_cross_kernel, ng_grid(((M.cnt[n - 1] + 63) / 64) * 64), dim3(NG_BLOCK), 0, s, M, n, sp, sq,
                     (const double*)scratch);
  DS2_LAUNCH_CHECK("ngram_prune_sums_cross_kernel");
  return 0;
}

extern "C" int ds2_ngram_prune_sums_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb,
                                         int n, double* q_out, double* sp, double* sq) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_prune_sums_host", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_sums_args("ds2_ngram_prune_sums_host", M, n, sp, sq, nullptr, 0, false)) return 1;
  for (long long r = 0; r < M.cnt[n - 2]; ++r) sp[r] = sq[r] = NAN;
  const u64* k = M.keys[n - 1];
  for (long long i = 0; i < M.cnt[n - 1];) {   // one context's children at a time, in row order
    const u64 ctx = k[i] >> M.b;
    double a = 0.0, c = 0.0;
    for (; i < M.cnt[n - 1] && (k[i] >> M.b) == ctx; ++i) {
      double p, q;
      pr_pq(M, n, i, &p, &q);
      if (q_out) q_out[i] = q;
      a += p;
      c += q;
    }
    const long long r = pr_find(M.keys[n - 2], M.cnt[n - 2], ctx);
    if (r >= 0) {
      sp[r] = a;
      sq[r] = c;
    }
  }
  return 0;
}

// One launch over the n-grams of every order >= 2: val (exp(dH) - 1) and mark (val < theta).  q, sp, sq, val, mark: `order` pointers,
// entry n - 1 for the n-grams of order n (entry 0 unused); sp / sq of entry n - 1 have the rows of order n - 1.
extern "C" int ds2_ngram_prune_entropy(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb,
                                       void* const* q, void* const* sp, void* const* sq, double theta, void* const* val, void* const* mark,
                                       void* stream) {
  using namespace ds2ng;
  PrModel M;
  PrWork W;
  if (pr_model("ds2_ngram_prune_entropy", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_work("ds2_ngram_prune_entropy", M, q, sp, sq, val, mark, theta, &W)) return 1;
  long long total = 0;
  for (int n = 2; n <= M.N; ++n) total += M.cnt[n - 1];
  if (total == 0) return 0;
  DS2_REQUIRE(total < 0x7fffffffll * NG_BLOCK, "ds2_ngram_prune_entropy: %lld n-grams exceed one launch", total);
  hipLaunchKernelGGL(ngram_prune_entropy_kernel, ng_grid(total), dim3(NG_BLOCK), 0, (hipStream_t)stream, M, W, theta);
  DS2_LAUNCH_CHECK("ngram_prune_entropy_kernel");
  return 0;
}

extern "C" int ds2_ngram_prune_entropy_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp,
                                            void* const* lb, void* const* q, void* const* sp, void* const* sq, double theta,
                                            void* const* val, void* const* mark) {
  using namespace ds2ng;
  PrModel M;
  PrWork W;
  if (pr_model("ds2_ngram_prune_entropy_host", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  if (pr_work("ds2_ngram_prune_entropy_host", M, q, sp, sq, val, mark, theta, &W)) return 1;
  for (int n = 2; n <= M.N; ++n)
    for (long long r = 0; r < M.cnt[n - 1]; ++r) pr_entropy_one(M, W, n, r, theta);
  return 0;
}

// Closure, one call per order n = N down to 3: an n-gram of order n that is kept (mark 0) clears the mark of its context
extern "C" int ds2_ngram_prune_closure(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb,
                                       int n, const unsigned char* mark, unsigned char* mark_ctx, void* stream) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_prune_closure", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  DS2_REQUIRE(n >= 2 && n <= M.N, "ds2_ngram_prune_closure: the order must be in [2, %d], got %d", M.N, n);
  if (M.cnt[n - 1] == 0 || M.cnt[n - 2] == 0) return 0;
  DS2_REQUIRE(mark && mark_ctx, "ds2_ngram_prune_closure: null pointer");
  hipLaunchKernelGGL(ngram_prune_closure_kernel, ng_grid(M.cnt[n - 1]), dim3(NG_BLOCK), 0, (hipStream_t)stream, M, n, mark, mark_ctx);
  DS2_LAUNCH_CHECK("ngram_prune_closure_kernel");
  return 0;
}

extern "C" int ds2_ngram_prune_closure_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp,
                                            void* const* lb, int n, const unsigned char* mark, unsigned char* mark_ctx) {
  using namespace ds2ng;
  PrModel M;
  if (pr_model("ds2_ngram_prune_closure_host", n_vocab, order, cnt, keys, lp, lb, &M)) return 1;
  DS2_REQUIRE(n >= 2 && n <= M.N, "ds2_ngram_prune_closure_host: the order must be in [2, %d], got %d", M.N, n);
  if (M.cnt[n - 1] == 0 || M.cnt[n - 2] == 0) return 0;
  DS2_REQUIRE(mark && mark_ctx, "ds2_ngram_prune_closure_host: null pointer");
  for (long long i = 0; i < M.cnt[n - 1]; ++i) {
    if (mark[i]) continue;
    const long long r = pr_find(M.keys[n - 2], M.cnt[n - 2], M.keys[n - 1][i] >> M.b);
    if (r >= 0) mark_ctx[r] = 0;
  }
  return 0;
}

// New backoffs of `cnt` context rows from the sums over their kept children: log10((1 - sp) / (1 - sq)), NaN where sp is NaN
extern "C" int ds2_ngram_prune_backoff(long long cnt, const double* sp, const double* sq, double* lb, void* stream) {
  using namespace ds2ng;
  DS2_REQUIRE(cnt >= 0 && cnt < 0x7fffffffll * NG_BLOCK, "ds2_ngram_prune_backoff: %lld rows", cnt);
  if (cnt == 0) return 0;
  DS2_REQUIRE(sp && sq && lb, "ds2_ngram_prune_backoff: null pointer");
  hipLaunchKernelGGL(ngram_prune_backoff_kernel, ng_grid(cnt), dim3(NG_BLOCK), 0, (hipStream_t)stream, cnt, sp, sq, lb);
  DS2_LAUNCH_CHECK("ngram_prune_backoff_kernel");
  return 0;
}

extern "C" int ds2_ngram_prune_backoff_host(long long cnt, const double* sp, const double* sq, double* lb) {
  using namespace ds2ng;
  DS2_REQUIRE(cnt >= 0, "ds2_ngram_prune_backoff_host: %lld rows", cnt);
  if (cnt == 0) return 0;
  DS2_REQUIRE(sp && sq && lb, "ds2_ngram_prune_backoff_host: null pointer");
  for (long long i = 0; i < cnt; ++i) lb[i] = sp[i] == sp[i] ? pr_backoff(sp[i], sq[i]) : NAN;
  return 0;
}
