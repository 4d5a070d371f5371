// N-best rescoring (contracts in include/ds2hip.h): the n-gram LM term of FINISHED label sequences as a number of its own
// (ds2_lm_score_seqs, ds2_lm_score_seq_host), and the sweep of an (alpha, beta) grid over per-hypothesis features (ds2_nbest_sweep).
// The beam search fuses the same LM term into pnb (ctc_beam.h), where alpha and beta cannot be varied without decoding again; here
// the packed model of ctc_lm.h is read through the same ngram_find / trie_child / context_backoffs / cond_score, unchanged.
//
// lm_score_kernel, one wavefront per sequence, 64 labels at a time, NO LDS and NO workspace:
//   1. a ballot over every label of the sequence finds a label outside [0, C) or equal to the blank before anything is read through
//      one (label_tok[label], the trie hash); such a sequence, or one whose length or range is out of bounds, gets NaN, -1, -1;
//   2. lanes stride the labels; a ballot marks the token starts (character mode: every label; word mode: a non-space label at index 0
//      or behind a space).  The lane at a start computes its token id: label_tok[label], or the walk of its word through trie_child,
//      which may run past the block of 64 and is bounded by the sequence's length;
//   3. the context of a start lane is the tokens of the previous order-1 start lanes: the highest set bits of the start ballot below
//      the lane, fetched by ds_bpermute (__shfl); where the block has too few, the tokens carried over from earlier blocks (lane j of
//      one VGPR holds the j-th most recent), and <s> before those.  The issue's sketch compacted the token ids into LDS or a
//      workspace row first; the ballot already orders the tokens, so nothing needs to be stored: no LDS, no per-sequence row, and no
//      length beyond which another path is taken;
//   4. every start lane runs context_backoffs and cond_score (at most 2 * order - 1 probes, independent across lanes);
//   5. the scores are added in token order: a wave-uniform loop over the set bits of the start ballot, v_readlane + one fp32 add each,
//      OOV scores counted instead of added.  The sum is therefore the sequential fp32 sum, bit for bit the host twin's.
// The order (a template parameter: contexts live in registers, indexed statically) and the mode select the instance.
// Cost: one dependent chain of hash probes per token (a trie walk of the word's length, then the n-gram probes), tokens of a block in
// parallel; HBM/L2 latency-bound table lookups, no arithmetic to speak of.
//
// nbest_sweep_kernel: one wavefront per (utterance, grid point), lanes stride the K slots, a (score, slot) butterfly picks the slot,
// lane r adds err[n, pick, r] into a register; a wave takes NS_UPW utterances of one grid point and ends with one 64-bit integer
// atomic per error kind, so the totals are exact and order-free.  Nothing of size N * K * Ga * Gb is stored.
#pragma once
#ifndef DS2_LM_SCORE_TU
#error "lm_score.h defines the ds2_lm_score_* and ds2_nbest_sweep entry points: it is compiled once, as part of decode.hip"
#endif
#include "common.h"
#include "ctc_lm.h"
#include <math.h>

namespace ds2lm {

__host__ __device__ inline bool seq_label_ok(int l, int C, int blank) { return l >= 0 && l < C && l != blank; }

// does a token start at label i?  (the labels are already known to be admissible)
__host__ __device__ inline bool seq_token_start(int mode, int space, const int* lab, int i) {
  return mode == MODE_CHAR || (lab[i] != space && (i == 0 || lab[i - 1] == space));
}

// the id of the token that starts at label i: the label's own token, or word_of[] of the trie node its word spells (-1: no such word)
__host__ __device__ inline int seq_token_at(const LmView& v, int mode, int space, const int* lab, int len, int i) {
  if (mode == MODE_CHAR) return v.label_tok[lab[i]];
  int node = 0;
  for (int j = i; j < len && lab[j] != space; ++j) {
    node = trie_child(v, node, lab[j]);
    if (node < 0) return -1;
  }
  return v.word_of[node];
}

// lm(w | h), h the M previous tokens, oldest first
template <int M>
__host__ __device__ inline float seq_token_score(const LmView& v, const int* h, int w) {
  float bow[MAX_ORDER];
  context_backoffs(v, h, M, bow);
  return cond_score(v, h, bow, M, w);
}

// One sequence, serially: the host twin of lm_score_kernel (same token and score routines, the same order of additions)
template <int M>
inline void seq_score_serial(const LmView& v, int mode, int space, int C, int blank, const int* lab, int len, int max_len, float* lm_sum,
                             int* n_tok, int* n_oov) {
  bool bad = len < 0 || len > max_len;
  for (int i = 0; !bad && i < len; ++i) bad = !seq_label_ok(lab[i], C, blank);
  if (bad) {
    *lm_sum = NAN;
    *n_tok = *n_oov = -1;
    return;
  }
  int h[MAX_ORDER];
  for (int k = 0; k < M; ++k) h[k] = v.h->bos;
  float sum = 0.f;
  int nt = 0, no = 0;
  for (int i = 0; i < len; ++i) {
    if (!seq_token_start(mode, space, lab, i)) continue;
    const int w = seq_token_at(v, mode, space, lab, len, i);
    const float s = seq_token_score<M>(v, h, w);
    ++nt;
    if (s == OOV) ++no;
    else sum = sum + s;
    for (int k = 0; k + 1 < M; ++k) h[k] = h[k + 1];
    if (M > 0) h[M - 1] = w;
  }
  *lm_sum = sum;
  *n_tok = nt;
  *n_oov = no;
}

}  // namespace ds2lm

namespace {

constexpr int LS_WAVES = 4;    // sequences per workgroup
constexpr int NS_WAVES = 4;    // waves per workgroup of the sweep
constexpr int NS_UPW = 8;      // utterances per wave of the sweep: one atomic per error kind and NS_UPW utterances
constexpr int NS_MAX_R = 64;   // error kinds: one lane each

__device__ __forceinline__ int ls_top_bit(unsigned long long m) { return 63 - __clzll((long long)m); }   // m != 0

template <int M>
__global__ __launch_bounds__(64 * LS_WAVES) void lm_score_kernel(const int* __restrict__ labels, long long n_labels,
                                                                  const long long* __restrict__ off, const int* __restrict__ lens, int P,
                                                                  int max_len, const void* __restrict__ blob, int mode, int space, int C,
                                                                  int blank, float* __restrict__ lm_sum, int* __restrict__ n_tok,
                                                                  int* __restrict__ n_oov) {
  using namespace ds2lm;
  const int p = blockIdx.x * LS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= P) return;
  const int lane = threadIdx.x & 63;
  const long long o = off[p];
  const int len = lens[p];
  bool bad = len < 0 || len > max_len || o < 0 || o > n_labels - len;
  const int* lab = labels + (bad ? 0 : o);
  // 1. every label, before anything is read through one
  for (int base = 0; !bad && base < len; base += 64) {
    const int i = base + lane;
    bad = __ballot(i < len && !seq_label_ok(lab[i], C, blank)) != 0ull;
  }
  if (bad) {
    if (lane == 0) {
      lm_sum[p] = NAN;
      n_tok[p] = -1;
      n_oov[p] = -1;
    }
    return;
  }
  const LmView v = lm_view(blob);
  int cw = v.h->bos;   // lane j: the j-th most recent token of the blocks so far
  float sum = 0.f;
  int nt = 0, no = 0;
  for (int base = 0; base < len; base += 64) {
    const int i = base + lane;
    const bool start = i < len && seq_token_start(mode, space, lab, i);
    const unsigned long long mk = __ballot(start);
    if (mk == 0ull) continue;
    const int w = start ? seq_token_at(v, mode, space, lab, len, i) : -1;
    const int cnt = __popcll(mk);
    // 3. the context: the previous M tokens (h oldest first), from this block's start lanes and then from the carry
    int h[MAX_ORDER];
    {
      unsigned long long below = mk & ((1ull << lane) - 1ull);
      const int mine = __popcll(below);
#pragma unroll
      for (int k = 0; k < M; ++k) {
        const int src = below ? ls_top_bit(below) : 0;
        const int from_block = __shfl(w, src, 64);
        const int from_carry = __shfl(cw, max(k - mine, 0), 64);
        h[M - 1 - k] = below ? from_block : from_carry;
        if (below) below &= ~(1ull << src);
      }
    }
    const float s = start ? seq_token_score<M>(v, h, w) : 0.f;
    const unsigned long long oovm = __ballot(start && s == OOV);
    nt += cnt;
    no += __popcll(oovm);
    // 5. in token order
    for (unsigned long long add = mk & ~oovm; add; add &= add - 1ull)
      sum = sum + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), __builtin_ctzll(add)));
    // the carry of the next block: lane j takes this block's j-th last token, or the old carry's (j - cnt)-th
    if (M > 0) {
      const int j = min(lane, MAX_ORDER);
      unsigned long long t = mk;
#pragma unroll
      for (int q = 0; q < MAX_ORDER - 1; ++q)
        if (q < j && t) t &= ~(1ull << ls_top_bit(t));
      const int from_block = __shfl(w, t ? ls_top_bit(t) : 0, 64);
      const int from_carry = __shfl(cw, max(j - cnt, 0), 64);
      cw = j < cnt ? from_block : from_carry;
    }
  }
  if (lane == 0) {
    lm_sum[p] = sum;
    n_tok[p] = nt;
    n_oov[p] = no;
  }
}

__global__ __launch_bounds__(64 * NS_WAVES) void nbest_sweep_kernel(const float* __restrict__ ac, const float* __restrict__ lm_sum,
                                                                     const int* __restrict__ n_tok, const int* __restrict__ n_oov,
                                                                     const int* __restrict__ err, int N, int K, int R, float oov_score,
                                                                     const float* __restrict__ alphas, const float* __restrict__ betas,
                                                                     int Gb, int* __restrict__ pick,
                                                                     unsigned long long* __restrict__ total) {
  const int g = blockIdx.x;   // grid point, row-major (alpha, beta)
  const float alpha = alphas[g / Gb], beta = betas[g % Gb];
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.y * NS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * NS_UPW;
  long long acc = 0;   // lane r: sum of err[n, pick, r] over this wave's utterances
  for (int n = n0; n < min(n0 + NS_UPW, N); ++n) {
    const long long row = (long long)n * K;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
      const float lm = __fadd_rn(lm_sum[row + k], __fmul_rn(oov_score, (float)n_oov[row + k]));
      float s = __fadd_rn(__fadd_rn(ac[row + k], __fmul_rn(alpha, lm)), __fmul_rn(beta, (float)n_tok[row + k]));
      s = s == s ? s : -INFINITY;
      if (s > best || arg == 0x7fffffff) {   // k ascends within a lane: strictly greater keeps the lowest slot
        best = s;
        arg = k;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(arg, o, 64);
      if (ov > best || (ov == best && oa < arg)) {
        best = ov;
        arg = oa;
      }
    }
    if (pick && lane == 0) pick[(long long)g * N + n] = arg;
    if (lane < R) acc += err[(row + arg) * R + lane];
  }
  if (lane < R && acc != 0) atomicAdd(total + (long long)g * R + lane, (unsigned long long)acc);
}

// the sizes a packed language model claims, against the bytes it was given and the arguments of the call
int lm_header_check(const char* who, const void* packed, size_t bytes, int lm_order, int lm_mode, int C) {
  using namespace ds2lm;
  DS2_REQUIRE(packed && bytes >= sizeof(LmHeader), "%s: no packed language model (%zu bytes)", who, bytes);
  const LmHeader* h = (const LmHeader*)packed;
  DS2_REQUIRE(h->magic == MAGIC, "%s: not a packed language model", who);
  DS2_REQUIRE(h->order >= 1 && h->order <= MAX_ORDER && (h->mode == MODE_CHAR || h->mode == MODE_WORD) && h->ncap >= 2 &&
                  (h->ncap & (h->ncap - 1)) == 0 && h->tcap >= 1 && (h->tcap & (h->tcap - 1)) == 0 && h->nnodes >= 1 && h->C >= 1 &&
                  h->bos >= -1 && bytes >= lm_bytes(h->ncap, h->tcap, h->nnodes, h->C),
              "%s: bad language model (order %d, mode %d, tables of %d and %d, %d nodes, %d classes, %zu bytes)", who, h->order, h->mode,
              h->ncap, h->tcap, h->nnodes, h->C, bytes);
  DS2_REQUIRE(h->order == lm_order && h->mode == lm_mode, "%s: the language model was packed with order %d, mode %d, the call says %d, %d",
              who, h->order, h->mode, lm_order, lm_mode);
  DS2_REQUIRE(h->C == C, "%s: the language model was packed for %d classes, the call has %d", who, h->C, C);
  return 0;
}

int lm_score_args_check(const char* who, int lm_mode, int space, int C, int blank) {
  DS2_REQUIRE(C >= 2 && blank >= 0 && blank < C, "%s: bad dims (C=%d blank=%d)", who, C, blank);
  DS2_REQUIRE(lm_mode == ds2lm::MODE_CHAR || (space >= 0 && space < C && space != blank),
              "%s: word mode needs a space label other than the blank (got %d)", who, space);
  return 0;
}

}  // namespace

extern "C" int ds2_lm_score_seqs(const int* labels, long long n_labels, const long long* off, const int* len, int P, int max_len,
                                 const void* lm_dev, const void* lm_host, size_t lm_bytes, int lm_order, int lm_mode, int space, int C,
                                 int blank, float* lm_sum, int* n_tok, int* n_oov, void* stream) {
  DS2_REQUIRE(P >= 0 && n_labels >= 0 && max_len >= 0 && max_len <= 0x7fffffff - 64,   // (label indices advance in steps of 64)
              "ds2_lm_score_seqs: bad dims (P=%d n_labels=%lld max_len=%d)", P, n_labels, max_len);
  if (lm_header_check("ds2_lm_score_seqs", lm_host, lm_bytes, lm_order, lm_mode, C)) return 1;
  if (lm_score_args_check("ds2_lm_score_seqs", lm_mode, space, C, blank)) return 1;
  if (P == 0) return 0;
  DS2_REQUIRE(lm_dev && off && len && lm_sum && n_tok && n_oov && (labels || n_labels == 0), "ds2_lm_score_seqs: null pointer");
  const dim3 grid((unsigned)(((long long)P + LS_WAVES - 1) / LS_WAVES)), block(64 * LS_WAVES);
  hipStream_t s = (hipStream_t)stream;
  const int sp = lm_mode == ds2lm::MODE_WORD ? space : -1;
#define DS2_LS_LAUNCH(M)                                                                                                              \
  case M + 1:                                                                                                                         \
    hipLaunchKernelGGL(lm_score_kernel<M>, grid, block, 0, s, labels, n_labels, off, len, P, max_len, lm_dev, lm_mode, sp, C, blank, \
                       lm_sum, n_tok, n_oov);                                                                                         \
    break;
  switch (lm_order) {
    DS2_LS_LAUNCH(0) DS2_LS_LAUNCH(1) DS2_LS_LAUNCH(2) DS2_LS_LAUNCH(3) DS2_LS_LAUNCH(4) DS2_LS_LAUNCH(5)
  }
#undef DS2_LS_LAUNCH
  DS2_LAUNCH_CHECK("lm_score_kernel");
  return 0;
}

extern "C" int ds2_lm_score_seq_host(const void* packed, size_t packed_bytes, const int* labels, int len, int max_len, int space, int C,
                                     int blank, float* lm_sum, int* n_tok, int* n_oov) {
  using namespace ds2lm;
  DS2_REQUIRE(lm_sum && n_tok && n_oov && (labels || len <= 0), "ds2_lm_score_seq_host: null pointer");
  DS2_REQUIRE(max_len >= 0, "ds2_lm_score_seq_host: max_len must be >= 0, got %d", max_len);
  const LmHeader* h = (const LmHeader*)packed;
  if (lm_header_check("ds2_lm_score_seq_host", packed, packed_bytes, packed && packed_bytes >= sizeof(LmHeader) ? h->order : 0,
                      packed && packed_bytes >= sizeof(LmHeader) ? h->mode : 0, C))
    return 1;
  if (lm_score_args_check("ds2_lm_score_seq_host", h->mode, space, C, blank)) return 1;
  const LmView v = lm_view(packed);
  const int sp = h->mode == MODE_WORD ? space : -1;
  switch (h->order) {
    case 1: seq_score_serial<0>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
    case 2: seq_score_serial<1>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
    case 3: seq_score_serial<2>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
    case 4: seq_score_serial<3>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
    case 5: seq_score_serial<4>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
    default: seq_score_serial<5>(v, h->mode, sp, C, blank, labels, len, max_len, lm_sum, n_tok, n_oov); break;
  }
  return 0;
}

extern "C" int ds2_nbest_sweep(const float* ac, const float* lm_sum, const int* n_tok, const int* n_oov, const int* err, int N, int K,
                               int R, float oov_score, const float* alphas, int Ga, const float* betas, int Gb, int* pick,
                               long long* total, void* stream) {
  DS2_REQUIRE(N >= 0 && K >= 1 && R >= 1 && R <= NS_MAX_R && Ga >= 1 && Gb >= 1, "ds2_nbest_sweep: bad dims (N=%d K=%d R=%d grid %d x %d; R <= %d)",
              N, K, R, Ga, Gb, NS_MAX_R);
  DS2_REQUIRE((long long)Ga * Gb <= 0x7fffffffll && (long long)N * K <= 0x7fffffffll / R, "ds2_nbest_sweep: grid or N * K * R too large");
  DS2_REQUIRE(oov_score == oov_score, "ds2_nbest_sweep: oov_score is NaN");
  DS2_REQUIRE(alphas && betas && total && (N == 0 || (ac && lm_sum && n_tok && n_oov && err)), "ds2_nbest_sweep: null pointer");
  hipStream_t s = (hipStream_t)stream;
  DS2_HIP(hipMemsetAsync(total, 0, sizeof(long long) * (size_t)Ga * Gb * R, s));
  if (N == 0) return 0;
  const int per_block = NS_WAVES * NS_UPW;
  const unsigned gy = (unsigned)((N + per_block - 1) / per_block);
  DS2_REQUIRE(gy <= 65535u, "ds2_nbest_sweep: N = %d exceeds the %d utterances of one call", N, 65535 * per_block);
  hipLaunchKernelGGL(nbest_sweep_kernel, dim3((unsigned)(Ga * Gb), gy), dim3(64 * NS_WAVES), 0, s, ac, lm_sum, n_tok, n_oov, err, N, K, R,
                     oov_score, alphas, betas, Gb, pick, (unsigned long long*)total);
  DS2_LAUNCH_CHECK("nbest_sweep_kernel");
  return 0;
}
