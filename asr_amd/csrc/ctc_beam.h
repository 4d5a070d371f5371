// CTC prefix beam search without a language model, one workgroup per utterance, the whole time loop in one launch.
// Replaces BeamCTCDecoder.decode (asr_deepspeech/decoders/beam_decoder.py), which hands the batch to the external
// `ctcdecode` C++ package.  The contract (include/ds2hip.h, tests/ctc_beam_oracle.py) in short: per frame the classes are
// sorted by probability (ties -> lower index) and pruned (cutoff_top_n, then cutoff_prob on the running sum); every beam l
// with last label e and every kept class c with log-prob lp contributes, under logaddexp:
//   c == blank: pb'(l) += total(l) + lp;   c == e: pnb'(l) += pnb(l) + lp, pnb'(l+c) += pb(l) + lp;
//   otherwise:  pnb'(l+c) += total(l) + lp
// and the K prefixes with the highest total = logaddexp(pb, pnb) survive (ties: shorter first, then smaller label sequence).
// The kernel is ctc_beam_kernel<PROF, Arm>; its last argument, the arm, says which search it is.  ctc_beam_kernel<PROF, NoArm> is the
// search above (ds2_ctc_beam_decode_f32): the arm is empty and the kernel compiles without the code of the others.
// ctc_beam_kernel<PROF, LmArgs> is the language-model arm (ds2_ctc_beam_decode_lm_f32): the LM terms of ctc_lm.h ride in pnb of
// each extension, every beam is extended by every kept class (no staircase) and, in word mode, the survivors are re-scored and
// re-sorted after the last frame.
// ctc_beam_kernel<PROF, HotArgs> is the hotword arm (ds2_ctc_beam_decode_hot_f32) on the same full grid: one more int of
// state per beam (the node of the automaton of ctc_hot.h), the term phi(n') - phi(n) added to the LM term of every extension, and
// the end-of-utterance re-score (-phi(state)) and re-sort always run.  Its LM blob may be null (hot-only): no LM table is read.
// ctc_beam_kernel<PROF, Streamed<Arm>> are the streaming instances of the three (ds2_ctc_beam_stream_feed_f32, ctc_beam_stream.h):
// the beams come from and go back to a state blob in global memory, and the frames of one call continue those of the calls before.
// Host side, every entry is beam_check -> beam_plan (sizes, LDS carve, the arm's arguments: BeamPlan) -> beam_dispatch, which picks the
// instance and launches it through the one launch site, beam_launch.
//
// Per frame, inside the workgroup (256 threads, all state in LDS):
//  1. class keys (prob bits, index) of the frame's row, block bitonic sort, running-sum cutoff by wave 0, the threshold key
//     of the last kept class (class x is kept  <=>  key(x) <= threshold) and the first K+1 kept non-blank classes;
//  2. the old beams go into an LDS hash table (64-bit rolling prefix hash + length);
//  3. candidates, in fixed slots:
//       - "stay" l for every old beam: the blank and repeat terms, plus the extension term from its parent l[:-1] when
//         the parent is a beam too (the only way two contributions can meet: a prefix has exactly one parent);
//       - the repeat extension l+e (score pb(l) + lp(e)) of every old beam;
//       - the extensions l_i + c_r (score total(l_i) + lp(c_r)) for beam rank i and non-blank class rank r with
//         (i+1)*r <= K.  A cell outside that staircase has at least (i+1)(r+1) - 1 - (i+1) >= K distinct prefixes ahead of
//         it (every cell up and to the left, less one repeat cell per row): it can never be among the K survivors;
//     an extension that is already a beam is merged into that beam's stay candidate instead (hash lookup);
//  4. block bitonic sort of the candidates by (total desc, length asc, label sequence asc); the label-sequence comparison
//     walks the two back-pointer chains and only runs on exact (total, length) ties;
//  5. the first K finite candidates become the new beams; a new prefix gets a node (parent, label, frame t).
// Candidate count <= 2K + sum_{j=1..K} (K/j + 1) = 2234 at K = 256 (4096 sort slots).
//
// Hash collisions: two prefixes are merged only when their 64-bit hashes AND lengths are equal.  The hash is
// h(l+c) = mix64(h(l) ^ (c+1)*k) with mix64 the splitmix64 finaliser (a bijection): two children of the SAME parent never
// collide; children of different parents collide when h(l1) ^ (c1+1)k == h(l2) ^ (c2+1)k, which for well-mixed parent hashes
// has probability 2^-64 per pair.  A lookup probes the table of at most K stored hashes, and at most T*(2K + K(K+1)) lookups
// are made per utterance: ~T*K^3 = 8.4e9 pairs at T = 501, K = 256, so a false merge has probability ~5e-10 per utterance.
//
// Cost of the tie rule: the label-sequence comparison of step 4 runs only for two candidates with bit-equal fp32 totals and
// equal lengths, and walks both back-pointer chains until they meet at a common node: at most t dependent global loads per
// side at frame t.  Worst case (every candidate of every frame tied, e.g. uniform frames): every comparison of the bitonic
// network walks, log2(P)(log2(P)+1)/2 stages of P/2 comparisons per frame, i.e. O(T^2 * P log^2 P) loads per utterance.
// Inputs with no exact ties never walk.  DS2_EXPERIMENTAL=1 DS2_BEAM_PROFILE=1 prints the per-frame time of each step and
// the number and length of the walks to stderr (one synchronising launch).
//
// Node storage (device workspace): parent / label / frame int32 per node, node id = t*K + slot, at most T*K per
// utterance: 12*B*T*K bytes.  The output chain walk runs once, after the last frame.
#pragma once
#ifndef DS2_CTC_BEAM_TU
#error "ctc_beam.h defines the ds2_ctc_beam_* entry points: it is compiled once, as part of decode.hip"
#endif
#include "common.h"
#include "ctc_lm.h"
#include "ctc_hot.h"
#include <stdio.h>
#include <string.h>

namespace {

typedef unsigned long long u64;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_K = 256;        // one new-beam slot per thread at selection; candidate slot ids fit 12 bits
constexpr int BEAM_MAX_C = 16384;      // the per-frame class sort lives in LDS (8 B per class, padded to a power of two)
constexpr int BEAM_MAX_T = (1 << 20) - 1;  // prefix length field of the candidate key
constexpr unsigned NEG_INF_HI = 0xFF800000u;   // high word of the key of any candidate whose total is -inf

__host__ __device__ inline int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
__host__ __device__ inline int max_candidates(int K) {
  int n = 2 * K;
  for (int j = 1; j <= K; ++j) n += K / j + 1;
  return n;
}

// LDS carve (all offsets multiples of 16): header | 2 beam buffers | kept non-blank list | row starts | hash table | union of
// the class sort keys and the candidate arrays
struct Layout {
  int K, PC, PK, HT;
  size_t beams, nb, rows, tab, uni, total;
  __host__ __device__ Layout(int K_, int PC_, int PK_, int HT_) : K(K_), PC(PC_), PK(PK_), HT(HT_) {
    // buffer_bytes(K), written out: calling it here reorders the address arithmetic at the head of every kernel instance, and with it
    // their register allocation (profiles/beam_plan_resources.txt)
    const size_t bb = align_up(6 * 4 * (size_t)K, 16) + 2 * 8 * (size_t)K;
    beams = 64;
    nb = beams + 2 * bb;
    rows = nb + 2 * align_up(4 * (size_t)(K + 1), 16);
    tab = rows + align_up(4 * (size_t)(K + 1), 16);
    uni = tab + align_up(4 * (size_t)HT, 16);
    const size_t cls = 8 * (size_t)PC, cand = 8 * (size_t)PK + 4 * 4 * (size_t)PK;
    total = uni + (cls > cand ? cls : cand);
  }
  __host__ __device__ static size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
  // one beam buffer, in LDS and in a stream's state blob: pb pnb tot node len last | h ph
  __host__ __device__ static size_t buffer_bytes(int K) { return align_up(6 * 4 * (size_t)K, 16) + 2 * 8 * (size_t)K; }
};

struct Beams {
  float *pb, *pnb, *tot;
  int *node, *len, *last;
  u64 *h, *ph;
};

__device__ inline Beams beams_at(char* smem, const Layout& L, int which) {
  char* p = smem + L.beams + which * Layout::buffer_bytes(L.K);
  Beams s;
  s.pb = (float*)p;
  s.pnb = s.pb + L.K;
  s.tot = s.pnb + L.K;
  s.node = (int*)(s.tot + L.K);
  s.len = s.node + L.K;
  s.last = s.len + L.K;
  s.h = (u64*)(p + Layout::align_up(6 * 4 * (size_t)L.K, 16));
  s.ph = s.h + L.K;
  return s;
}

struct Header {
  int nb, nkept, bpos, ncells, blank_kept, pad0, pad1, pad2;
  u64 thr;
  float lp_blank;
};

__device__ inline float lae(float a, float b) {   // log(exp a + exp b), -inf absorbing
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (m == -INFINITY || m == INFINITY) return m;
  return m + log1pf(expf(n - m));
}
__device__ inline float sane_prob(float p) { return p >= 0.f ? p : 0.f; }   // NaN (a poisoned forward) and negatives count as 0
__device__ inline u64 class_key(float p, int c) {   // ascending = probability descending, then class index ascending
  return ((u64)(~__float_as_uint(sane_prob(p))) << 32) | (unsigned)c;
}
__device__ inline float key_prob(u64 k) { return __uint_as_float(~(unsigned)(k >> 32)); }
__device__ inline u64 cand_key(float s, int len, int slot) {   // ascending = total descending, then length ascending, then slot
  if (s != s) s = -INFINITY;
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((u64)(~u) << 32) | ((u64)len << 12) | (unsigned)slot;
}
__device__ inline u64 dummy_key(int slot) { return ((u64)NEG_INF_HI << 32) | ((u64)BEAM_MAX_T << 12) | (unsigned)slot; }

__device__ inline u64 mix64(u64 z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ inline u64 hash_ext(u64 h, int c) { return mix64(h ^ ((u64)(unsigned)(c + 1) * 0xD6E8FEB86659FD93ull)); }

__device__ inline int tab_lookup(const int* tab, int HT, const Beams& o, u64 h, int len) {
  int pos = (int)(h & (u64)(HT - 1));
  for (;;) {   // load factor <= 1/2: an empty slot is always reached
    const int v = tab[pos];
    if (v < 0) return -1;
    if (o.h[v] == h && o.len[v] == len) return v;
    pos = (pos + 1) & (HT - 1);
  }
}

__device__ inline float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
__device__ inline int wave_incl_scan_i(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// ascending block bitonic sort of n (a power of two) keys; the caller has synchronised before, this ends synchronised
template <class Less>
__device__ void block_sort(u64* k, int n, Less less) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += BEAM_THREADS) {
        const int i = 2 * stride * (t / stride) + (t & (stride - 1)), j = i + stride;
        const u64 a = k[i], b = k[j];
        const bool swap = (i & size) == 0 ? less(b, a) : less(a, b);
        if (swap) {
          k[i] = b;
          k[j] = a;
        }
      }
      __syncthreads();
    }
  }
}

struct ClassLess {
  __device__ bool operator()(u64 a, u64 b) const { return a < b; }
};

// order of two candidates with equal (total, length): the smaller label sequence first.  A candidate is (chain x, label y)
// with x the node of its first len-1 labels: stay l -> (parent(node l), label(node l)), extension l_i + c -> (node l_i, c).
struct CandLess {
  const Beams o;
  const int* c_src;
  const int* c_cls;
  const int* n_parent;
  const int* n_label;
  int* walks;   // profiling: [number of chain walks, chain steps], or null
  __device__ void split(int idx, int& x, int& y) const {
    const int src = c_src[idx], cls = c_cls[idx];
    if (cls >= 0) {
      x = o.node[src];
      y = cls;
    } else {
      const int nd = o.node[src];
      x = nd >= 0 ? n_parent[nd] : -1;
      y = nd >= 0 ? n_label[nd] : -1;
    }
  }
  __device__ bool operator()(u64 a, u64 b) const {
    if ((a >> 12) != (b >> 12) || (unsigned)(a >> 32) == NEG_INF_HI) return a < b;
    int xa, ya, xb, yb;
    split((int)(a & 0xFFF), xa, ya);
    split((int)(b & 0xFFF), xb, yb);
    int d = 0;   // equal lengths: both chains reach the root together; the last difference seen is the earliest position
    if (walks) atomicAdd(&walks[0], 1);
    while (xa != xb && xa >= 0 && xb >= 0) {
      if (walks) atomicAdd(&walks[1], 1);
      const int la = n_label[xa], lb = n_label[xb];
      if (la != lb) d = la < lb ? -1 : 1;
      xa = n_parent[xa];
      xb = n_parent[xb];
    }
    if (d == 0) d = ya < yb ? -1 : (ya > yb ? 1 : 0);
    return d != 0 ? d < 0 : a < b;
  }
};

// PROF: thread 0 stamps the 100 MHz wall clock after each step's closing barrier and writes, per utterance, the ticks of
// [prune classes, generate candidates, sort candidates, select], the chain walks and their steps, and the frame count.
//
// Arms: the kernel's one trailing argument says which instance it is.  An arm type (NoArm, LmArgs, HotArgs, Streamed<> of one of them)
// states LM, HOT and STREAM and hands out the LmArgs, the hotword blob and the StreamArgs the kernel reads; what an arm does not have is
// empty and, under the kernel's `if constexpr`, never read.
// A streaming instance (ctc_beam_stream.h) resumes the search from a state blob in global memory, consumes this call's frames, writes the
// state back and, when asked, reads the beams out.  Every difference from the one-call kernel sits under `if constexpr (STREAM)`: an
// instance whose arm is not Streamed<> compiles to the code it was.
struct StreamArgs {
  char* state;        // B blobs of `stride` bytes: StreamHeader | beam buffer | LmBeams (LM, hotwords) | hotword states
  size_t stride;
  int cap, n_out, W;  // node storage for `cap` rows of K nodes per utterance (a row per frame until a commit compacts them,
                      // ctc_beam_commit.h); read-out of n_out slots in rows of W (n_out == 0: none)
  int* stable_len;    // (B)
  int* frames;        // (B)
};
// LM arm (LM = true): shallow fusion with the packed n-gram model of ctc_lm.h.  Per-beam LM state sits in LDS after the no-LM
// layout (LmBeams, one per beam buffer) and the kept non-blank class list is sized for every kept class (the full grid).
struct LmArgs {
  static constexpr bool LM = true, HOT = false, STREAM = false;
  const void* blob;
  float alpha, beta;
  int m, mode, space, nbl;   // context length (order - 1), ds2lm::MODE_*, space label (word mode), non-blank list capacity
  __device__ LmArgs lm_args() const { return *this; }
  __device__ const void* hot_blob() const { return nullptr; }
  __device__ StreamArgs stream_args() const { return StreamArgs{}; }
};
// the plain kernel: no extra argument is read, and its code is that of the kernel without the LM arm
struct NoArm {
  static constexpr bool LM = false, HOT = false, STREAM = false;
  __device__ LmArgs lm_args() const { return LmArgs{}; }
  __device__ const void* hot_blob() const { return nullptr; }
  __device__ StreamArgs stream_args() const { return StreamArgs{}; }
};

constexpr int LM_CTX = ds2lm::MAX_ORDER - 1;

struct LmBeams {
  int* ctx;     // K x LM_CTX: the last m tokens, oldest first (<s>-padded)
  float* bow;   // K x LM_CTX: log10 backoff of every suffix of ctx (ds2lm::context_backoffs)
  int* node;    // trie node of the partial word (word mode)
  float* lmb;   // the LM bonus added when the beam's last label was appended
};

__host__ __device__ inline size_t lm_beams_bytes(int K) { return (size_t)(2 * LM_CTX + 2) * 4 * K; }
__host__ __device__ inline size_t lm_layout_total(const Layout& L, int nbl) {
  return Layout::align_up(L.total, 16) + 2 * lm_beams_bytes(L.K) + 8 * (size_t)nbl;
}

__device__ inline LmBeams lm_beams_at(char* smem, const Layout& L, int which) {
  char* p = smem + Layout::align_up(L.total, 16) + which * lm_beams_bytes(L.K);
  LmBeams s;
  s.ctx = (int*)p;
  s.bow = (float*)(s.ctx + LM_CTX * L.K);
  s.node = (int*)(s.bow + LM_CTX * L.K);
  s.lmb = (float*)(s.node + L.K);
  return s;
}

// the LM term of the extension l -> l+c for a beam in state (ctx, bow, node) with length len and last label `last`;
// -inf when word mode's dictionary rules out the extension
__device__ inline float lm_bonus(const ds2lm::LmView& v, const LmArgs& a, const int* ctx, const float* bow, int node, int len, int last,
                                 int c) {
  if (a.mode == ds2lm::MODE_CHAR) return a.alpha * ds2lm::cond_score(v, ctx, bow, a.m, v.label_tok[c]) + a.beta;
  if (c != a.space) return ds2lm::trie_child(v, node, c) >= 0 ? 0.f : -INFINITY;
  const int w = v.word_of[node];   // the root (empty partial) is no word: no leading or double space
  if (len == 0 || last == a.space || w < 0) return -INFINITY;
  return a.alpha * ds2lm::cond_score(v, ctx, bow, a.m, w) + a.beta;
}

// the child state of l+c from the parent's state (src) into slot j of dst
__device__ inline void lm_child(const ds2lm::LmView& v, const LmArgs& a, const LmBeams& o, int src, int c, float bonus,
                                const LmBeams& d, int j) {
  int tok = -2;
  if (a.mode == ds2lm::MODE_CHAR) tok = v.label_tok[c];
  else if (c == a.space) tok = v.word_of[o.node[src]];
  if (tok != -2) {   // a new token enters the context
    for (int i = 0; i + 1 < a.m; ++i) d.ctx[j * LM_CTX + i] = o.ctx[src * LM_CTX + i + 1];
    if (a.m > 0) d.ctx[j * LM_CTX + a.m - 1] = tok;
    ds2lm::context_backoffs(v, d.ctx + j * LM_CTX, a.m, d.bow + j * LM_CTX);
    d.node[j] = 0;
  } else {
    for (int i = 0; i < a.m; ++i) {
      d.ctx[j * LM_CTX + i] = o.ctx[src * LM_CTX + i];
      d.bow[j * LM_CTX + i] = o.bow[src * LM_CTX + i];
    }
    d.node[j] = ds2lm::trie_child(v, o.node[src], c);
  }
  d.lmb[j] = bonus;
}

__device__ inline void lm_copy(const LmArgs& a, const LmBeams& o, int src, const LmBeams& d, int j) {
  for (int i = 0; i < a.m; ++i) {
    d.ctx[j * LM_CTX + i] = o.ctx[src * LM_CTX + i];
    d.bow[j * LM_CTX + i] = o.bow[src * LM_CTX + i];
  }
  d.node[j] = o.node[src];
  d.lmb[j] = o.lmb[src];
}

// Hotword arm: the LM arm's arguments (lm.blob null: hot-only, the LM term is 0 and no LM table is read) and the packed automaton.
// Per-beam state: the automaton node of the prefix, one int per beam and beam buffer, after the LM arm's LDS.
struct HotArgs {
  static constexpr bool LM = true, HOT = true, STREAM = false;
  LmArgs lm;
  const void* hot;
  __device__ LmArgs lm_args() const { return lm; }
  __device__ const void* hot_blob() const { return hot; }
  __device__ StreamArgs stream_args() const { return StreamArgs{}; }
};
// the streaming instance of an arm: the arm's own arguments and constants, and the stream's
template <class Arm>
struct Streamed : Arm {
  static constexpr bool STREAM = true;
  StreamArgs st;
  __device__ StreamArgs stream_args() const { return st; }
};

__host__ __device__ inline size_t hot_state_bytes(int K) { return Layout::align_up(4 * (size_t)K, 16); }
__host__ __device__ inline size_t hot_layout_total(const Layout& L, int nbl) {
  return Layout::align_up(lm_layout_total(L, nbl), 16) + 2 * hot_state_bytes(L.K);
}

// LM term + hotword term of the extension of beam k (hotword state hs) by class c; -inf stays -inf
__device__ inline float hot_bonus(const ds2lm::LmView& v, const LmArgs& a, const LmBeams& mo, int k, int len, int last, int c,
                                  const ds2hot::HotView& hv, int hs) {
  const float b = a.blob ? lm_bonus(v, a, mo.ctx + k * LM_CTX, mo.bow + k * LM_CTX, mo.node[k], len, last, c) : 0.f;
  int nx;
  float term;
  ds2hot::hot_step(hv, hs, c, nx, term);
  return b + term;
}

// 64 bytes; all zero = a freshly opened stream.  The last four fields belong to the commit kernel (ctc_beam_commit.h) and stay zero in a
// stream that never commits: the frame t0 + t writes row row_base + t0 + t - frame_base of the node storage (rows below row_base hold
// the compacted live tree), and the first committed_len (label, offset) pairs of every beam have left the storage for the host
// (the last of them at frame commit_frame), so a read-out starts at pair committed_len.
struct StreamHeader {
  int opened, t0, nb, stable_len, stable_node, row_base, frame_base, committed_len, commit_frame, pad[7];
};
static_assert(sizeof(StreamHeader) == 64, "the state blob's header is 64 bytes");
// defined in ctc_beam_stream.h
__device__ inline void stream_load(const StreamArgs& st, int b, const Layout& L, char* smem, Header* hd, bool lm, const LmBeams& l0, int* h0);
__device__ inline void stream_save(const StreamArgs& st, int b, const Layout& L, char* smem, const Header* hd, int cur, int frames, bool lm,
                                   const LmBeams& l0, const LmBeams& l1, const int* hf);
__device__ inline void stream_stable(const StreamArgs& st, int b, Header* hd, const Beams& f, int nb, const int* n_parent);

template <bool PROF, class Arm>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_kernel(const float* __restrict__ probs, long long ld_b, long long ld_t, int T,
                                                               int C, const int* __restrict__ sizes, int blank, int K, int top_n,
                                                               float cutoff_prob, int PC, int PK, int HT, int* __restrict__ labels,
                                                               int* __restrict__ offsets, int* __restrict__ lens, float* __restrict__ scores,
                                                               int* __restrict__ nodes, u64* __restrict__ prof, Arm arm) {
  constexpr bool LM = Arm::LM, HOT = Arm::HOT, STREAM = Arm::STREAM;
  [[maybe_unused]] const StreamArgs st = arm.stream_args();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const LmArgs lm = arm.lm_args();
  const Layout L(K, PC, PK, HT);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  Header* hd = (Header*)smem;
  const Beams b0 = beams_at(smem, L, 0), b1 = beams_at(smem, L, 1);
  float* nb_lp = (float*)(smem + L.nb);
  int* nb_cls = (int*)(smem + L.nb + Layout::align_up(4 * (size_t)(K + 1), 16));
  int* rowstart = (int*)(smem + L.rows);
  int* tab = (int*)(smem + L.tab);
  u64* ck = (u64*)(smem + L.uni);   // class keys (phase 1) ...
  u64* keys = (u64*)(smem + L.uni);  // ... then candidate keys and data (phases 3-5)
  int* c_src = (int*)(keys + PK);
  int* c_cls = c_src + PK;
  float* c_pb = (float*)(c_cls + PK);
  float* c_pnb = c_pb + PK;
  long long TK = (long long)T * K;
  if constexpr (STREAM) TK = (long long)st.cap * K;   // node ids row * K + slot do not depend on the capacity
  int* n_parent = nodes + (long long)b * 3 * TK;
  int* n_label = n_parent + TK;
  int* n_frame = n_label + TK;
  int n = sizes ? min(max(sizes[b], 0), T) : T;
  [[maybe_unused]] int t0 = 0;        // frames consumed by earlier calls
  [[maybe_unused]] bool fresh = true;  // no earlier call: the beams start from the empty prefix
  [[maybe_unused]] int row_shift = 0;  // frame t0 + t writes node row t0 + t + row_shift: 0 in a stream that never committed
  if constexpr (STREAM) {
    const StreamHeader* sh = (const StreamHeader*)(st.state + (size_t)b * st.stride);
    fresh = sh->opened == 0;
    t0 = fresh ? 0 : sh->t0;
    row_shift = fresh ? 0 : sh->row_base - sh->frame_base;
    n = max(min(n, st.cap - (t0 + row_shift)), 0);   // (the entry has checked the host's bound; a wrong bound must not write past the nodes)
  }
  const int R = min(top_n, C);
  ds2lm::LmView lv;
  LmBeams l0, l1;
  float* lnb_lp = nullptr;
  int* lnb_cls = nullptr;
  [[maybe_unused]] ds2hot::HotView hv;
  [[maybe_unused]] int *h0 = nullptr, *h1 = nullptr;
  if constexpr (HOT) {
    hv = ds2hot::hot_view(arm.hot_blob());
    h0 = (int*)(smem + Layout::align_up(lm_layout_total(L, lm.nbl), 16));
    h1 = (int*)((char*)h0 + hot_state_bytes(K));
    if (tid == 0 && fresh) h0[0] = 0;
  }
  if constexpr (LM) {
    if (!HOT || lm.blob) lv = ds2lm::lm_view(lm.blob);
    l0 = lm_beams_at(smem, L, 0);
    l1 = lm_beams_at(smem, L, 1);
    lnb_lp = (float*)(smem + Layout::align_up(L.total, 16) + 2 * lm_beams_bytes(K));
    lnb_cls = (int*)(lnb_lp + lm.nbl);
    if (tid == 0 && fresh) {
      for (int i = 0; i < lm.m; ++i) l0.ctx[i] = lv.h->bos;
      ds2lm::context_backoffs(lv, l0.ctx, lm.m, l0.bow);
      l0.node[0] = 0;
      l0.lmb[0] = 0.f;
    }
  }

  if (tid == 0 && fresh) {
    const Beams& s = b0;
    s.pb[0] = 0.f;
    s.pnb[0] = -INFINITY;
    s.tot[0] = 0.f;
    s.node[0] = -1;
    s.len[0] = 0;
    s.last[0] = -1;
    s.h[0] = 0x243F6A8885A308D3ull;
    s.ph[0] = 0;
    hd->nb = 1;
    hd->pad0 = hd->pad1 = 0;
  }
  if constexpr (STREAM) {
    if (!fresh) stream_load(st, b, L, smem, hd, LM, l0, h0);
    if (tid == 0) hd->pad1 = row_shift * K;   // kept in LDS, not in a register across the frame loop (pad1 is the profiling build's)
  }
  u64 ticks[4] = {0, 0, 0, 0}, stamp = PROF ? wall_clock64() : 0;
  auto lap = [&](int phase) {
    if (PROF && tid == 0) {
      const u64 now = wall_clock64();
      ticks[phase] += now - stamp;
      stamp = now;
    }
  };
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < n; ++t) {
    const int nb_old = hd->nb;
    if (nb_old == 0) break;
    const Beams o = cur ? b1 : b0, w = cur ? b0 : b1;
    [[maybe_unused]] const LmBeams mo = cur ? l1 : l0, mw = cur ? l0 : l1;
    [[maybe_unused]] const int* ho = cur ? h1 : h0;
    [[maybe_unused]] int* hw = cur ? h0 : h1;
    const float* row = probs + b * ld_b + t * ld_t;

    // 1. prune the classes
    for (int c = tid; c < PC; c += BEAM_THREADS) ck[c] = c < C ? class_key(row[c], c) : ~0ull;
    __syncthreads();
    block_sort(ck, PC, ClassLess());
    if (tid < 64) {
      int nk = R;
      if (cutoff_prob < 1.f) {
        float run = 0.f;
        for (int base = 0; base < R; base += 64) {
          const int j = base + lane;
          const float incl = wave_incl_scan(j < R ? key_prob(ck[j]) : 0.f, lane);
          const u64 m = __ballot(j < R && run + incl >= cutoff_prob);
          if (m) {
            nk = base + __ffsll((long long)m);   // the class that reaches the cutoff is kept
            break;
          }
          run += __shfl(incl, 63, 64);
        }
      }
      if (tid == 0) {
        hd->nkept = nk;
        hd->thr = ck[nk - 1];
        hd->bpos = 0x7fffffff;
        const bool bk = class_key(row[blank], blank) <= ck[nk - 1];
        hd->blank_kept = bk;
        hd->lp_blank = bk ? logf(sane_prob(row[blank])) : -INFINITY;
      }
    }
    for (int i = tid; i < HT; i += BEAM_THREADS) tab[i] = -1;
    __syncthreads();
    const int nk = hd->nkept;
    const u64 thr = hd->thr;
    const int lim = LM ? nk : min(nk, K + 2);
    for (int j = tid; j < lim; j += BEAM_THREADS)
      if ((int)(unsigned)ck[j] == blank) hd->bpos = j;
    for (int k = tid; k < nb_old; k += BEAM_THREADS) {
      int pos = (int)(o.h[k] & (u64)(HT - 1));
      while (atomicCAS(&tab[pos], -1, k) != -1) pos = (pos + 1) & (HT - 1);
    }
    __syncthreads();
    const int bpos = hd->bpos;
    for (int j = tid; j < lim; j += BEAM_THREADS) {
      if (j == bpos) continue;
      const int r = j - (j > bpos ? 1 : 0);
      if constexpr (LM) {   // every kept non-blank class: r < nk - blank kept <= min(top_n, C - 1) = lm.nbl
        lnb_cls[r] = (int)(unsigned)ck[j];
        lnb_lp[r] = logf(key_prob(ck[j]));
      } else if (r <= K) {
        nb_cls[r] = (int)(unsigned)ck[j];
        nb_lp[r] = logf(key_prob(ck[j]));
      }
    }
    const bool blank_kept = hd->blank_kept;
    const float lp_blank = hd->lp_blank;
    const int n_nb = LM ? nk - (blank_kept ? 1 : 0) : min(K + 1, nk - (blank_kept ? 1 : 0));
    __syncthreads();   // the class keys are dead from here: the candidate arrays overwrite them
    lap(0);

    // 3a. stay candidates, repeat extensions, staircase row lengths
    for (int k = tid; k < nb_old; k += BEAM_THREADS) {
      const float tot = o.tot[k], pb = o.pb[k], pnb = o.pnb[k];
      const int len = o.len[k], e = o.last[k];
      const float npb = blank_kept ? tot + lp_blank : -INFINITY;
      float npnb = -INFINITY;
      int ecls = -1;
      float es = -INFINITY, eb = -INFINITY;
      if (len > 0 && class_key(row[e], e) <= thr) {
        const float lpe = logf(sane_prob(row[e]));
        npnb = pnb + lpe;
        const int p = tab_lookup(tab, HT, o, o.ph[k], len - 1);
        if constexpr (LM) {   // the parent's extension carries the bonus of l's last label
          if (p >= 0) npnb = lae(npnb, (o.last[p] == e ? o.pb[p] : o.tot[p]) + lpe + mo.lmb[k]);
          if constexpr (HOT) eb = hot_bonus(lv, lm, mo, k, len, e, e, hv, ho[k]);
          else eb = lm_bonus(lv, lm, mo.ctx + k * LM_CTX, mo.bow + k * LM_CTX, mo.node[k], len, e, e);
          es = pb + lpe + eb;
        } else {
          if (p >= 0) npnb = lae(npnb, (o.last[p] == e ? o.pb[p] : o.tot[p]) + lpe);
          es = pb + lpe;
        }
        if (es > -INFINITY && tab_lookup(tab, HT, o, hash_ext(o.h[k], e), len + 1) < 0) ecls = e;
      }
      keys[k] = cand_key(lae(npb, npnb), len, k);
      c_src[k] = k;
      c_cls[k] = -1;
      c_pb[k] = npb;
      c_pnb[k] = npnb;
      const int s = nb_old + k;
      keys[s] = ecls >= 0 ? cand_key(es, len + 1, s) : dummy_key(s);
      c_src[s] = k;
      c_cls[s] = ecls;
      c_pb[s] = LM ? eb : -INFINITY;   // LM: an extension's pb slot holds its bonus (its pb is -inf)
      c_pnb[s] = es;
    }
    if (!LM && tid < 64) {   // exclusive prefix of the row lengths min(n_nb, K/(i+1) + 1)
      int carry = 0;
      for (int base = 0; base < nb_old; base += 64) {
        const int i = base + lane;
        const int v = i < nb_old ? min(n_nb, K / (i + 1) + 1) : 0;
        const int incl = wave_incl_scan_i(v, lane);
        if (i < nb_old) rowstart[i] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
      }
      if (lane == 0) {
        rowstart[nb_old] = carry;
        hd->ncells = carry;
      }
    }
    __syncthreads();

    // 3b. extensions inside the staircase
    const int ncells = LM ? nb_old * n_nb : hd->ncells;
    const int M = 2 * nb_old + ncells, P = pow2_ceil(M);
    if constexpr (LM) {   // the full grid: per-(beam, class) bonuses and dictionary -inf cells break the staircase's monotonicity
      for (int g = tid; g < ncells; g += BEAM_THREADS) {
        const int i = g / n_nb, r = g - i * n_nb, c = lnb_cls[r], s = 2 * nb_old + g;
        const int len = o.len[i];
        const bool rep = len > 0 && c == o.last[i];
        float bonus = -INFINITY;
        if constexpr (HOT) {
          if (!rep) bonus = hot_bonus(lv, lm, mo, i, len, o.last[i], c, hv, ho[i]);
        } else {
          bonus = rep ? -INFINITY : lm_bonus(lv, lm, mo.ctx + i * LM_CTX, mo.bow + i * LM_CTX, mo.node[i], len, o.last[i], c);
        }
        const float sc = o.tot[i] + lnb_lp[r] + bonus;
        const bool real = !rep && sc > -INFINITY && tab_lookup(tab, HT, o, hash_ext(o.h[i], c), len + 1) < 0;
        keys[s] = real ? cand_key(sc, len + 1, s) : dummy_key(s);
        c_src[s] = i;
        c_cls[s] = c;
        c_pb[s] = bonus;
        c_pnb[s] = sc;
      }
    } else
    for (int g = tid; g < ncells; g += BEAM_THREADS) {
      int lo = 0, hi = nb_old - 1;   // last row with rowstart <= g
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rowstart[mid] <= g) lo = mid;
        else hi = mid - 1;
      }
      const int i = lo, r = g - rowstart[i], c = nb_cls[r], s = 2 * nb_old + g;
      const int len = o.len[i];
      const float sc = o.tot[i] + nb_lp[r];
      const bool real = !(len > 0 && c == o.last[i]) && sc > -INFINITY && tab_lookup(tab, HT, o, hash_ext(o.h[i], c), len + 1) < 0;
      keys[s] = real ? cand_key(sc, len + 1, s) : dummy_key(s);
      c_src[s] = i;
      c_cls[s] = c;
      c_pb[s] = -INFINITY;
      c_pnb[s] = sc;
    }
    for (int s = M + tid; s < P; s += BEAM_THREADS) keys[s] = dummy_key(s);
    __syncthreads();
    lap(1);

    // 4. order the candidates
    block_sort(keys, P, CandLess{o, c_src, c_cls, n_parent, n_label, PROF ? &hd->pad0 : nullptr});
    lap(2);

    // 5. the first K finite candidates are the new beams
    const int j = tid;
    const u64 kj = j < K && j < P ? keys[j] : dummy_key(0);
    const bool live = (unsigned)(kj >> 32) != NEG_INF_HI;
    const int nb_new = __syncthreads_count(live);
    if (live) {
      const int idx = (int)(kj & 0xFFF), src = c_src[idx], cls = c_cls[idx];
      if (cls < 0) {
        w.pb[j] = c_pb[idx];
        w.pnb[j] = c_pnb[idx];
        w.tot[j] = lae(c_pb[idx], c_pnb[idx]);
        w.node[j] = o.node[src];
        w.len[j] = o.len[src];
        w.last[j] = o.last[src];
        w.h[j] = o.h[src];
        w.ph[j] = o.ph[src];
        if constexpr (LM) lm_copy(lm, mo, src, mw, j);
        if constexpr (HOT) hw[j] = ho[src];
      } else {
        int tg = t, nd = t * K + j;   // the frame's index in the stream, the node's id
        if constexpr (STREAM) {
          tg += t0;
          nd = tg * K + j + hd->pad1;
        }
        n_parent[nd] = o.node[src];
        n_label[nd] = cls;
        n_frame[nd] = tg;
        w.pb[j] = -INFINITY;
        w.pnb[j] = c_pnb[idx];
        w.tot[j] = c_pnb[idx];
        w.node[j] = nd;
        w.len[j] = o.len[src] + 1;
        w.last[j] = cls;
        w.h[j] = hash_ext(o.h[src], cls);
        w.ph[j] = o.h[src];
        if constexpr (HOT) {
          if (lm.blob) lm_child(lv, lm, mo, src, cls, c_pb[idx], mw, j);
          else mw.lmb[j] = c_pb[idx];
          float term;
          ds2hot::hot_step(hv, ho[src], cls, hw[j], term);
        } else if constexpr (LM) {
          lm_child(lv, lm, mo, src, cls, c_pb[idx], mw, j);
        }
      }
    }
    if (tid == 0) hd->nb = nb_new;
    __syncthreads();
    lap(3);
    cur ^= 1;
  }
  if (PROF && tid == 0) {
    for (int i = 0; i < 4; ++i) prof[b * 8 + i] = ticks[i];
    prof[b * 8 + 4] = (unsigned)hd->pad0;
    prof[b * 8 + 5] = (unsigned)hd->pad1;
    prof[b * 8 + 6] = n;
  }

  [[maybe_unused]] bool readout = true;
  if constexpr (STREAM) {
    // the state the next call resumes from, before the end-of-utterance stage below: that stage works on the LDS copy alone
    const int* hf = nullptr;
    if constexpr (HOT) hf = cur ? h1 : h0;
    stream_save(st, b, L, smem, hd, cur, t0 + n, LM, l0, l1, hf);
    readout = st.n_out > 0;
  }

  if constexpr (LM) {
    // end of utterance: score the partial word (word mode), give back the lead of a partial hotword match, re-sort the survivors
    if ((HOT || lm.mode == ds2lm::MODE_WORD) && hd->nb > 0 && readout) {
      const int nbf = hd->nb, P = pow2_ceil(nbf);
      const Beams f = cur ? b1 : b0, w = cur ? b0 : b1;
      const LmBeams lf = cur ? l1 : l0, lw = cur ? l0 : l1;
      u64* keys = (u64*)(smem + L.uni);
      int* c_src = (int*)(keys + PK);
      int* c_cls = c_src + PK;
      float* c_tot = (float*)(c_cls + PK);
      for (int k = tid; k < P; k += BEAM_THREADS) {
        if (k < nbf) {
          float tot = f.tot[k];
          if ((!HOT || lm.mode == ds2lm::MODE_WORD) && f.len[k] > 0 && f.last[k] != lm.space) {
            const int wd = lv.word_of[lf.node[k]];   // an incomplete partial word is out of vocabulary
            tot += lm.alpha * (wd < 0 ? ds2lm::OOV : ds2lm::cond_score(lv, lf.ctx + k * LM_CTX, lf.bow + k * LM_CTX, lm.m, wd)) + lm.beta;
          }
          if constexpr (HOT) tot -= hv.phi[(cur ? h1 : h0)[k]];
          keys[k] = cand_key(tot, f.len[k], k);
          c_src[k] = k;
          c_cls[k] = -1;
          c_tot[k] = tot;
        } else {
          keys[k] = dummy_key(k);
        }
      }
      __syncthreads();
      block_sort(keys, P, CandLess{f, c_src, c_cls, n_parent, n_label, nullptr});
      for (int j = tid; j < nbf; j += BEAM_THREADS) {
        const int idx = (int)(keys[j] & 0xFFF);
        w.pb[j] = f.pb[idx];
        w.pnb[j] = f.pnb[idx];
        w.tot[j] = c_tot[idx];
        w.node[j] = f.node[idx];
        w.len[j] = f.len[idx];
        w.last[j] = f.last[idx];
        w.h[j] = f.h[idx];
        w.ph[j] = f.ph[idx];
        lm_copy(lm, lf, idx, lw, j);
        if constexpr (HOT) (cur ? h0 : h1)[j] = (cur ? h1 : h0)[idx];
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  // results: K slots per utterance, best first; label / offset rows zero past each length
  const int nb = hd->nb;
  const Beams f = cur ? b1 : b0;
  int KO = K, TO = T;   // slots per utterance and row width of the outputs
  [[maybe_unused]] int done = 0;   // (label, offset) pairs the host holds already: a stream's read-out starts there
  if constexpr (STREAM) {
    KO = st.n_out;
    TO = st.W;
    done = ((const StreamHeader*)(st.state + (size_t)b * st.stride))->committed_len;   // (stream_save has left it as it was)
  }
  int* lab = labels + (long long)b * KO * TO;
  int* off = offsets + (long long)b * KO * TO;
  for (int j = 0; j < KO; ++j) {
    int len = j < nb ? f.len[j] : 0;
    if constexpr (STREAM) len = max(len - done, 0);   // (a row holds the pairs from the committed length on)
    for (int s = len + tid; s < TO; s += BEAM_THREADS) {
      lab[(long long)j * TO + s] = 0;
      off[(long long)j * TO + s] = 0;
    }
  }
  for (int j = tid; j < KO; j += BEAM_THREADS) {
    if (j < nb) {
      int x = f.node[j];
      if constexpr (STREAM) {   // (a stream's rows are the caller's width; the entry has checked that it holds every uncommitted pair)
        for (int s = f.len[j] - 1 - done; s >= 0; --s) {
          if (s < TO) {
            lab[(long long)j * TO + s] = n_label[x];
            off[(long long)j * TO + s] = n_frame[x];
          }
          x = n_parent[x];
        }
      } else {
        for (int s = f.len[j] - 1; s >= 0; --s) {
          lab[(long long)j * TO + s] = n_label[x];
          off[(long long)j * TO + s] = n_frame[x];
          x = n_parent[x];
        }
      }
      lens[b * KO + j] = f.len[j];
      scores[b * KO + j] = f.tot[j];
    } else {
      lens[b * KO + j] = 0;
      scores[b * KO + j] = -INFINITY;
    }
  }
  if constexpr (STREAM) stream_stable(st, b, hd, f, nb, n_parent);
}

}  // namespace

extern "C" int ds2_ctc_beam_max_width(void) { return BEAM_MAX_K; }

extern "C" size_t ds2_ctc_beam_workspace_bytes(int B, int T, int beam_width) {
  if (B <= 0 || T <= 0 || beam_width <= 0) return 0;
  return (size_t)3 * sizeof(int) * B * T * beam_width;
}

// What the three decode entries share (`who` names the entry in an error).  `arm`: the pointer an arm cannot do without, the LM or the
// hotword blob (the plain entry passes probs again).
static int beam_check(const char* who, const float* probs, const void* arm, int B, int T, int C, int blank, int beam_width, int cutoff_top_n,
                      float cutoff_prob, const int* labels, const int* offsets, const int* lens, const float* scores, const void* ws,
                      size_t ws_bytes) {
  DS2_REQUIRE(probs && labels && offsets && lens && scores && arm, "%s: null pointer", who);
  DS2_REQUIRE(beam_width >= 1 && beam_width <= BEAM_MAX_K, "%s: beam_width %d outside the supported 1..%d", who, beam_width, BEAM_MAX_K);
  DS2_REQUIRE(C >= 2 && C <= BEAM_MAX_C, "%s: %d classes outside the supported 2..%d", who, C, BEAM_MAX_C);
  DS2_REQUIRE(B > 0 && T > 0 && T <= BEAM_MAX_T && blank >= 0 && blank < C, "%s: bad dims (B=%d T=%d C=%d blank=%d; T <= %d)", who, B, T, C,
              blank, BEAM_MAX_T);
  DS2_REQUIRE(cutoff_top_n >= 1 && cutoff_prob == cutoff_prob, "%s: cutoff_top_n must be >= 1 and cutoff_prob a number", who);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_beam_workspace_bytes(B, T, beam_width), "%s: workspace too small", who);
  return 0;
}

// The language-model arguments of the LM and hotword entries (`who` names the entry in an error)
static int beam_lm_check(const char* who, size_t lm_bytes, int lm_order, int lm_mode, int space, int C, int blank, float alpha, float beta) {
  DS2_REQUIRE(lm_order >= 1 && lm_order <= ds2lm::MAX_ORDER && (lm_mode == ds2lm::MODE_CHAR || lm_mode == ds2lm::MODE_WORD) &&
                  lm_bytes >= sizeof(ds2lm::LmHeader),
              "%s: bad language model (order %d, mode %d, %zu bytes)", who, lm_order, lm_mode, lm_bytes);
  DS2_REQUIRE(lm_mode == ds2lm::MODE_CHAR || (space >= 0 && space < C && space != blank),
              "%s: word mode needs a space label other than the blank (got %d)", who, space);
  DS2_REQUIRE(alpha == alpha && beta == beta && fabsf(alpha) < INFINITY && fabsf(beta) < INFINITY, "%s: alpha and beta must be finite", who);
  return 0;
}

// the sizes a packed automaton claims, against the bytes it was given
static int hot_header_check(const char* who, const void* packed, size_t bytes) {
  using namespace ds2hot;
  DS2_REQUIRE(packed && bytes >= sizeof(HotHeader), "%s: no packed hotword automaton (%zu bytes)", who, bytes);
  const HotHeader* h = (const HotHeader*)packed;
  DS2_REQUIRE(h->magic == MAGIC, "%s: not a packed hotword automaton", who);
  DS2_REQUIRE(h->nnodes >= 2 && h->nnodes <= MAX_NODES && h->tcap == pow2_ceil(2 * (h->nnodes - 1) + 1) && h->depth >= 1 &&
                  h->depth <= MAX_DEPTH && bytes >= hot_bytes(h->tcap, h->nnodes),
              "%s: bad hotword automaton (%d nodes, table of %d, depth %d, %zu bytes)", who, h->nnodes, h->tcap, h->depth, bytes);
  return 0;
}

// The launch plan, the same for every entry: the sizes the kernel takes, the arm's LDS total and the arm's arguments.  lm_dev / hot_dev
// null: the entry has no such arm.  Both arms search the full grid of K * (nbl + 2) candidates.
struct BeamPlan {
  int K, nbl, PC, PK, HT;
  size_t lds;
  bool lm;
  const void* hot;   // the packed automaton on the device, or null
  LmArgs la;
};

static int beam_plan(BeamPlan& p, const char* who, int C, int blank, int beam_width, int cutoff_top_n, const void* lm_dev, size_t lm_bytes,
                     int lm_order, int lm_mode, int space, float alpha, float beta, const void* hot_dev, const void* hot_host,
                     size_t hot_bytes) {
  const bool lm = lm_dev != nullptr, hot = hot_dev != nullptr;
  if (hot) {
    if (hot_header_check(who, hot_host, hot_bytes)) return 1;
    DS2_REQUIRE(((const ds2hot::HotHeader*)hot_host)->C == C, "%s: the hotwords were packed for %d classes, probs have %d", who,
                ((const ds2hot::HotHeader*)hot_host)->C, C);
  }
  if (lm)
    if (int rc = beam_lm_check(who, lm_bytes, lm_order, lm_mode, space, C, blank, alpha, beta)) return rc;
  const int K = beam_width, nbl = min(cutoff_top_n, C - 1);
  DS2_REQUIRE(!(lm || hot) || (long long)K * (nbl + 2) <= ds2_ctc_beam_lm_max_candidates(),
              "%s: beam_width * (min(cutoff_top_n, C - 1) + 2) = %lld exceeds the %d candidate slots%s", who, (long long)K * (nbl + 2),
              ds2_ctc_beam_lm_max_candidates(), hot ? " (hotwords search the full grid, with or without a language model)" : "");
  const int PC = pow2_ceil(C), PK = pow2_ceil(lm || hot ? K * (nbl + 2) : max_candidates(K)), HT = 2 * pow2_ceil(K);
  const Layout lay(K, PC, PK, HT);
  // the hotword arm: the LM arm's layout and one int of hotword state per beam and buffer
  const size_t lds = hot ? hot_layout_total(lay, nbl) : lm ? lm_layout_total(lay, nbl) : lay.total;
  if (hot)
    DS2_REQUIRE(lds <= 160 * 1024, "%s: LDS layout of %zu bytes (%zu of them hotword state) does not fit the 160 KiB at beam_width %d, %d classes",
                who, lds, 2 * hot_state_bytes(K), K, C);
  else
    DS2_REQUIRE(PK <= 4096 && lds <= 160 * 1024, "%s: LDS layout of %zu bytes does not fit", who, lds);
  p = BeamPlan{K, nbl, PC, PK, HT, lds, lm, hot_dev,
               lm ? LmArgs{lm_dev, alpha, beta, lm_order - 1, lm_mode, lm_mode == ds2lm::MODE_WORD ? space : -1, nbl}
                  : LmArgs{nullptr, 0.f, 0.f, 0, 0, -1, nbl}};
  return 0;
}

// What a launch takes from its entry beside the plan
struct BeamCall {
  const float* probs;
  long long ld_b, ld_t;
  int B, T, C;
  const int* sizes;
  int blank, top_n;
  float cutoff_prob;
  int *labels, *offsets, *lens;
  float* scores;
  int* nodes;
  void* stream;
};

// The one launch site of ctc_beam_kernel<PROF, Arm>: the dynamic-LDS limit above 64 KiB, one workgroup per utterance, the launch check
template <bool PROF, class Arm>
static int beam_launch(const char* label, const BeamPlan& p, const BeamCall& c, u64* prof, const Arm& arm) {
  const auto kernel = ctc_beam_kernel<PROF, Arm>;
  if (p.lds > 64 * 1024) DS2_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  hipLaunchKernelGGL(kernel, dim3(c.B), dim3(BEAM_THREADS), p.lds, (hipStream_t)c.stream, c.probs, c.ld_b, c.ld_t, c.T, c.C, c.sizes, c.blank,
                     p.K, c.top_n, c.cutoff_prob, p.PC, p.PK, p.HT, c.labels, c.offsets, c.lens, c.scores, c.nodes, prof, arm);
  DS2_LAUNCH_CHECK(label);
  return 0;
}

// the instance for (hot, lm, streamed); st null: a one-call decode
static int beam_dispatch(const BeamPlan& p, const BeamCall& c, const StreamArgs* st) {
  const HotArgs ha{p.la, p.hot};
  if (st) {
    if (p.hot) return beam_launch<false>("ctc_beam_kernel<HOT, STREAM>", p, c, nullptr, Streamed<HotArgs>{ha, *st});
    if (p.lm) return beam_launch<false>("ctc_beam_kernel<LM, STREAM>", p, c, nullptr, Streamed<LmArgs>{p.la, *st});
    return beam_launch<false>("ctc_beam_kernel<STREAM>", p, c, nullptr, Streamed<NoArm>{NoArm{}, *st});
  }
  if (p.hot) return beam_launch<false>("ctc_beam_kernel<HOT>", p, c, nullptr, ha);
  if (p.lm) return beam_launch<false>("ctc_beam_kernel<LM>", p, c, nullptr, p.la);
  return beam_launch<false>("ctc_beam_kernel", p, c, nullptr, NoArm{});
}

extern "C" int ds2_ctc_beam_decode_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev,
                                       int blank, int beam_width, int cutoff_top_n, float cutoff_prob, int* labels, int* offsets,
                                       int* lens, float* scores, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ds2_ctc_beam_decode_f32";
  if (int rc = beam_check(who, probs, probs, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, ws, ws_bytes))
    return rc;
  BeamPlan p;
  if (int rc = beam_plan(p, who, C, blank, beam_width, cutoff_top_n, nullptr, 0, 0, 0, 0, 0.f, 0.f, nullptr, nullptr, 0)) return rc;
  const BeamCall c{probs, ld_b, ld_t, B, T, C, sizes_dev, blank, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, (int*)ws, stream};
  const char* pe = ds2_exp_getenv("DS2_BEAM_PROFILE");
  if (!(pe && pe[0] == '1')) return beam_dispatch(p, c, nullptr);
  // profiling build of the same kernel (experiments only): per-step times averaged over the utterances' frames
  u64* prof = nullptr;
  DS2_HIP(hipMalloc(&prof, (size_t)B * 8 * sizeof(u64)));
  if (int rc = beam_launch<true>("ctc_beam_kernel (profiling)", p, c, prof, NoArm{})) {
    hipFree(prof);
    return rc;
  }
  u64* h = (u64*)calloc((size_t)B * 8, sizeof(u64));
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpy(h, prof, (size_t)B * 8 * sizeof(u64), hipMemcpyDeviceToHost);
  hipFree(prof);
  if (e != hipSuccess) {
    free(h);
    return ds2_set_error("ctc_beam_kernel (profiling): %s", hipGetErrorString(e));
  }
  double sum[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 7; ++i) sum[i] += (double)h[b * 8 + i];
  free(h);
  const double fr = sum[6] > 0 ? sum[6] : 1;   // wall clock: 100 MHz
  fprintf(stderr,
          "ds2_ctc_beam profile (K=%d C=%d, %.0f frames): us/frame prune %.2f, candidates %.2f, sort %.2f, select %.2f; "
          "chain walks/frame %.1f, steps/walk %.1f\n",
          p.K, C, sum[6], sum[0] / fr / 100, sum[1] / fr / 100, sum[2] / fr / 100, sum[3] / fr / 100, sum[4] / fr,
          sum[4] > 0 ? sum[5] / sum[4] : 0.0);
  return 0;
}

// ---- language-model arm (ds2_ctc_lm_*, ds2_ctc_beam_decode_lm_f32) ----

extern "C" int ds2_ctc_beam_lm_max_candidates(void) { return 4096; }

extern "C" size_t ds2_ctc_lm_packed_bytes(int order, int n_ngrams, int n_edges, int n_nodes, int C) {
  if (order < 1 || order > ds2lm::MAX_ORDER || n_ngrams < 1 || n_edges < 0 || n_nodes < 1 || C < 1 || n_ngrams > (1 << 28) ||
      n_edges > (1 << 28))
    return 0;
  return ds2lm::lm_bytes(pow2_ceil(2 * n_ngrams), pow2_ceil(2 * n_edges + 1), n_nodes, C);
}

extern "C" int ds2_ctc_lm_pack(int order, int n_ngrams, const int* ngram_tok, const int* ngram_n, const float* prob, const float* bow,
                               int n_edges, const int* edge_node, const int* edge_label, const int* edge_child, int n_nodes,
                               const int* node_word, int C, const int* label_tok, int bos, int mode, void* out, size_t out_bytes) {
  using namespace ds2lm;
  const size_t need = ds2_ctc_lm_packed_bytes(order, n_ngrams, n_edges, n_nodes, C);
  DS2_REQUIRE(need > 0, "ds2_ctc_lm_pack: bad sizes (order %d, %d n-grams, %d trie edges, %d nodes, %d classes)", order, n_ngrams,
              n_edges, n_nodes, C);
  DS2_REQUIRE(out && out_bytes >= need, "ds2_ctc_lm_pack: output buffer of %zu bytes, %zu needed", out_bytes, need);
  DS2_REQUIRE(ngram_tok && ngram_n && prob && bow && node_word && label_tok && (n_edges == 0 || (edge_node && edge_label && edge_child)),
              "ds2_ctc_lm_pack: null pointer");
  DS2_REQUIRE(mode == MODE_CHAR || mode == MODE_WORD, "ds2_ctc_lm_pack: mode %d is neither character (1) nor word (2)", mode);
  memset(out, 0, need);
  LmHeader* h = (LmHeader*)out;
  h->magic = MAGIC;
  h->order = order;
  h->ncap = pow2_ceil(2 * n_ngrams);
  h->tcap = pow2_ceil(2 * n_edges + 1);
  h->nnodes = n_nodes;
  h->C = C;
  h->bos = bos;
  h->mode = mode;
  const LmView v = lm_view(out);
  LmEntry* ng = (LmEntry*)v.ng;
  for (int i = 0; i < n_ngrams; ++i) {
    const int n = ngram_n[i];
    const int* tok = ngram_tok + (size_t)i * order;
    DS2_REQUIRE(n >= 1 && n <= order, "ds2_ctc_lm_pack: n-gram %d has order %d (model order %d)", i, n, order);
    for (int j = 0; j < n; ++j) DS2_REQUIRE(tok[j] >= 0, "ds2_ctc_lm_pack: n-gram %d has a negative token id", i);
    DS2_REQUIRE(!ngram_find(v, n, tok), "ds2_ctc_lm_pack: n-gram %d is listed twice", i);
    int pos = (int)(ngram_hash(n, tok) & (u64)(h->ncap - 1));
    while (ng[pos].n != 0) pos = (pos + 1) & (h->ncap - 1);
    ng[pos].n = n;
    for (int j = 0; j < n; ++j) ng[pos].tok[j] = tok[j];
    ng[pos].prob = prob[i];
    ng[pos].bow = bow[i];
  }
  TrieEntry* tr = (TrieEntry*)v.trie;
  for (int i = 0; i < h->tcap; ++i) tr[i].node = -1;
  for (int i = 0; i < n_edges; ++i) {
    DS2_REQUIRE(edge_node[i] >= 0 && edge_node[i] < n_nodes && edge_child[i] > 0 && edge_child[i] < n_nodes && edge_label[i] >= 0 &&
                    edge_label[i] < C,
                "ds2_ctc_lm_pack: trie edge %d out of range", i);
    DS2_REQUIRE(trie_child(v, edge_node[i], edge_label[i]) < 0, "ds2_ctc_lm_pack: trie edge %d is listed twice", i);
    int pos = (int)(trie_hash(edge_node[i], edge_label[i]) & (u64)(h->tcap - 1));
    while (tr[pos].node >= 0) pos = (pos + 1) & (h->tcap - 1);
    tr[pos].node = edge_node[i];
    tr[pos].label = edge_label[i];
    tr[pos].child = edge_child[i];
  }
  memcpy((int*)v.word_of, node_word, 4 * (size_t)n_nodes);
  memcpy((int*)v.label_tok, label_tok, 4 * (size_t)C);
  return 0;
}

extern "C" int ds2_ctc_lm_score(const void* packed, const int* hist, int n_hist, int w, float* out) {
  using namespace ds2lm;
  DS2_REQUIRE(packed && out && (n_hist == 0 || hist), "ds2_ctc_lm_score: null pointer");
  const LmView v = lm_view(packed);
  DS2_REQUIRE(v.h->magic == MAGIC, "ds2_ctc_lm_score: not a packed language model");
  DS2_REQUIRE(n_hist == v.h->order - 1, "ds2_ctc_lm_score: %d context tokens for an order-%d model", n_hist, v.h->order);
  float bw[MAX_ORDER];
  context_backoffs(v, hist, n_hist, bw);
  *out = cond_score(v, hist, bw, n_hist, w);
  return 0;
}

extern "C" int ds2_ctc_beam_decode_lm_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev,
                                          int blank, int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev,
                                          size_t lm_bytes, int lm_order, int lm_mode, int space, float alpha, float beta, int* labels,
                                          int* offsets, int* lens, float* scores, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ds2_ctc_beam_decode_lm_f32";
  if (int rc = beam_check(who, probs, lm_dev, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, ws, ws_bytes))
    return rc;
  BeamPlan p;
  if (int rc = beam_plan(p, who, C, blank, beam_width, cutoff_top_n, lm_dev, lm_bytes, lm_order, lm_mode, space, alpha, beta, nullptr, nullptr, 0))
    return rc;
  return beam_dispatch(p, BeamCall{probs, ld_b, ld_t, B, T, C, sizes_dev, blank, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, (int*)ws,
                                   stream}, nullptr);
}

// ---- hotword arm (ds2_ctc_hot_*, ds2_ctc_beam_decode_hot_f32) ----

extern "C" size_t ds2_ctc_hot_packed_bytes(int n_nodes, int n_edges) {
  if (n_nodes < 2 || n_nodes > ds2hot::MAX_NODES || n_edges != n_nodes - 1) return 0;
  return ds2hot::hot_bytes(pow2_ceil(2 * n_edges + 1), n_nodes);
}

extern "C" int ds2_ctc_hot_pack(int n_nodes, int n_edges, const int* edge_node, const int* edge_label, const int* edge_child,
                                const int* fail, const float* phi, const int* terminal, int C, void* out, size_t out_bytes) {
  using namespace ds2hot;
  DS2_REQUIRE(n_nodes >= 2 && n_nodes <= MAX_NODES, "ds2_ctc_hot_pack: %d trie nodes outside the supported 2..%d", n_nodes, MAX_NODES);
  DS2_REQUIRE(n_edges == n_nodes - 1, "ds2_ctc_hot_pack: a trie of %d nodes has %d edges, got %d", n_nodes, n_nodes - 1, n_edges);
  DS2_REQUIRE(C >= 2 && C <= BEAM_MAX_C, "ds2_ctc_hot_pack: %d classes outside the supported 2..%d", C, BEAM_MAX_C);
  const size_t need = ds2_ctc_hot_packed_bytes(n_nodes, n_edges);
  DS2_REQUIRE(out && out_bytes >= need, "ds2_ctc_hot_pack: output buffer of %zu bytes, %zu needed", out_bytes, need);
  DS2_REQUIRE(edge_node && edge_label && edge_child && fail && phi && terminal, "ds2_ctc_hot_pack: null pointer");
  memset(out, 0, need);
  HotHeader* h = (HotHeader*)out;   // the magic goes in last: a refused automaton leaves no usable blob behind
  h->nnodes = n_nodes;
  h->tcap = pow2_ceil(2 * n_edges + 1);
  h->C = C;
  const HotView v = hot_view(out);
  ds2lm::TrieEntry* tr = (ds2lm::TrieEntry*)v.trie;
  for (int i = 0; i < h->tcap; ++i) tr[i].node = -1;
  int* parent = (int*)v.terminal;   // scratch until the terminal flags are copied in: the parent of every node
  for (int i = 0; i < n_nodes; ++i) parent[i] = -1;
  for (int i = 0; i < n_edges; ++i) {
    DS2_REQUIRE(edge_node[i] >= 0 && edge_node[i] < n_nodes && edge_child[i] > 0 && edge_child[i] < n_nodes && edge_label[i] >= 0 &&
                    edge_label[i] < C,
                "ds2_ctc_hot_pack: trie edge %d out of range", i);
    DS2_REQUIRE(parent[edge_child[i]] < 0, "ds2_ctc_hot_pack: node %d has two parents", edge_child[i]);
    DS2_REQUIRE(hot_child(v, edge_node[i], edge_label[i]) < 0, "ds2_ctc_hot_pack: trie edge %d is listed twice", i);
    parent[edge_child[i]] = edge_node[i];
    int pos = (int)(ds2lm::trie_hash(edge_node[i], edge_label[i]) & (ds2lm::u64)(h->tcap - 1));
    while (tr[pos].node >= 0) pos = (pos + 1) & (h->tcap - 1);
    tr[pos].node = edge_node[i];
    tr[pos].label = edge_label[i];
    tr[pos].child = edge_child[i];
  }
  int* depth = (int*)v.fail;   // scratch until the links are copied in
  int deepest = 0;
  for (int i = 0; i < n_nodes; ++i) {   // n_nodes - 1 edges, one parent per non-root node: a tree when every node reaches the root
    int d = 0, x = i;
    while (x != 0 && d <= MAX_DEPTH) {
      x = parent[x];
      ++d;
    }
    DS2_REQUIRE(x == 0 && d <= MAX_DEPTH, "ds2_ctc_hot_pack: node %d lies deeper than the supported %d labels per phrase", i, MAX_DEPTH);
    depth[i] = d;
    deepest = d > deepest ? d : deepest;
  }
  DS2_REQUIRE(fail[0] == 0, "ds2_ctc_hot_pack: the root's failure link must point to the root, got %d", fail[0]);
  int nterm = 0;
  for (int i = 0; i < n_nodes; ++i) {
    DS2_REQUIRE(i == 0 || (fail[i] >= 0 && fail[i] < n_nodes && depth[fail[i]] < depth[i]),
                "ds2_ctc_hot_pack: the failure link of node %d does not point to a strictly shallower node", i);
    DS2_REQUIRE(phi[i] >= 0.f && phi[i] < INFINITY, "ds2_ctc_hot_pack: the potential of node %d is not a finite number >= 0", i);
    nterm += terminal[i] != 0;
  }
  DS2_REQUIRE(phi[0] == 0.f && !terminal[0], "ds2_ctc_hot_pack: the root has potential 0 and ends no phrase");
  h->nterminal = nterm;
  h->depth = deepest;
  memcpy((int*)v.fail, fail, 4 * (size_t)n_nodes);
  memcpy((float*)v.phi, phi, 4 * (size_t)n_nodes);
  for (int i = 0; i < n_nodes; ++i) ((int*)v.terminal)[i] = terminal[i] != 0;
  h->magic = MAGIC;
  return 0;
}

extern "C" int ds2_ctc_hot_step(const void* packed, int node, int label, int* next, float* term) {
  using namespace ds2hot;
  DS2_REQUIRE(packed && next && term, "ds2_ctc_hot_step: null pointer");
  const HotHeader* h = (const HotHeader*)packed;
  DS2_REQUIRE(h->magic == MAGIC, "ds2_ctc_hot_step: not a packed hotword automaton");
  DS2_REQUIRE(node >= 0 && node < h->nnodes && label >= 0 && label < h->C, "ds2_ctc_hot_step: node %d or label %d out of range", node, label);
  hot_step(hot_view(packed), node, label, *next, *term);
  return 0;
}

extern "C" int ds2_ctc_beam_decode_hot_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev,
                                           int blank, int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev,
                                           size_t lm_bytes, int lm_order, int lm_mode, int space, float alpha, float beta,
                                           const void* hot_dev, const void* hot_host, size_t hot_bytes, int* labels, int* offsets,
                                           int* lens, float* scores, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ds2_ctc_beam_decode_hot_f32";
  if (int rc = beam_check(who, probs, hot_dev, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, ws, ws_bytes))
    return rc;
  BeamPlan p;
  if (int rc = beam_plan(p, who, C, blank, beam_width, cutoff_top_n, lm_dev, lm_bytes, lm_order, lm_mode, space, alpha, beta, hot_dev, hot_host,
                         hot_bytes)) return rc;
  return beam_dispatch(p, BeamCall{probs, ld_b, ld_t, B, T, C, sizes_dev, blank, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores, (int*)ws,
                                   stream}, nullptr);
}
