// CTC forced alignment (ds2_ctc_align_f32, contract in include/ds2hip.h): the lattice of ctc.hip over (max, +) instead of log-sum-exp,
// with 2-bit back-pointers, the backtrace and the token spans in the same launch.  Compiled inside ctc.hip's translation unit.
//
// Layout shared by both variants: PAIR j owns the adjacent states 2j (blank) and 2j + 1 (label j).  Forward in t a pair needs one value
// from outside, the odd state of pair j - 1 (s - 1 of the even state, s - 2 of the odd one; the odd state's s - 1 is the pair's own even
// state), so both of a pair's states stay in the owner's registers:
//   variant 1 (MODE 0) one wavefront per utterance, pair = lane, the neighbour's value by a one-lane DPP wave shift;
//   variant 2 (MODE 1) one workgroup per utterance, pair = thread, the neighbour's value through an LDS row of odd states and one
//             barrier per frame; (MODE 2) more pairs than threads: every thread loops over its pairs with both rows in LDS.
// The cell (align_cell) is the same function in every path: compares and one fp32 add, so all of them write the same bits.
// Back-pointers: the move into frame f + 1 is "transition f"; a pair's two back-pointers are one nibble (bits 0-1 even state, bits 2-3
// odd state), eight transitions make one dword, and the dword of (group g = f >> 3, pair j) sits at bp[g * Wp + j]: the owner
// accumulates eight frames in a register and stores once, and a store instruction of a wave covers a contiguous run.
// The backtrace (wave 0) stages whole group rows in LDS by bulk copies whose addresses do not depend on the state, then walks them; the
// per-frame states leave 64 frames at a time.  Token spans and log-probabilities are a parallel pass over the written states.
// STAR (ds2_ctc_align_star_f32, entries in ctc_align_star.h): the label value C is the wildcard, whose emission is the row g that a
// pre-pass wrote (a select on the load address and on the loaded value, both off the dependent chain), and per-utterance flags open
// the start states 2, 3 and the end states S - 3, S - 4.  STAR = false compiles to the plain kernels: no select, no flag, no g.
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_align.h is a part of ctc.hip"
#endif

namespace {

constexpr int ALIGN_STAGE_WORDS = 4096;       // LDS words of staged back-pointer rows per bulk copy (never less than one row)

struct AlignArgs {
  const float* x;
  long long ld_b, ld_t;
  int T, C;
  const int *targets, *tgt_off, *in_lens, *tgt_lens;
  int maxU;
  float* score;
  int *states, *tok_start, *tok_end;
  float* tok_logp;
  unsigned* bp;          // [B][NG][Wp]
  int Wp, NG, stage_words;
  const float* g;        // STAR only: [B][T] the wildcard's emission per frame (a log value), and the per-utterance flags (or null)
  const int* flags;
};

constexpr int ALIGN_FREE_START = 1, ALIGN_FREE_END = 2;

template <bool STAR>
__device__ __forceinline__ int align_flags(const AlignArgs& a, int b) {
  return (STAR && a.flags) ? a.flags[b] : 0;
}

// a label outside [1, C), or outside [1, C] where C is the wildcard
template <bool STAR>
__device__ __forceinline__ bool align_bad_label(int c, int C) {
  return (c < 1) || (STAR ? c > C : c >= C);
}

// e = x (log-probabilities) or log(x) on the hardware log2 (fast_log_'s two operations, kept out of any fused multiply-add so that
// every path rounds the emission the same way)
template <int IS_LOG>
__device__ __forceinline__ float align_emit(float x) {
  if (IS_LOG) return x;
  {
#pragma clang fp contract(off)
    const float l2 = __builtin_amdgcn_logf(x);
    return l2 * 0.69314718055994530942f;
  }
}

// the emission of an odd state from its loaded value: the wildcard's row is stored as a log value
template <int IS_LOG, bool STAR>
__device__ __forceinline__ float align_emit_odd(float x, bool star) {
  const float e = align_emit<IS_LOG>(x);
  return (STAR && star) ? x : e;
}

// One frame of one pair.  E, O: the pair's states in the previous frame, Om: the odd state of the pair below (NEG_INF for pair 0).
// Ties keep the smaller move (stay, then step, then skip).  Returns the nibble of back-pointers.
__device__ __forceinline__ unsigned align_cell(float& E, float& O, float Om, bool skip, float eE, float eO) {
  const bool stepE = Om > E;
  const float mE = stepE ? Om : E;
  float mO = O;
  unsigned bO = 0;
  if (E > mO) { mO = E; bO = 1; }
  if (skip && Om > mO) { mO = Om; bO = 2; }
  E = mE + eE;
  O = mO + eO;
  return (stepE ? 1u : 0u) | (bO << 2);
}

__device__ __forceinline__ void align_write_infeasible(const AlignArgs& a, int b, int U, float sc) {
  if (threadIdx.x == 0) a.score[b] = sc;
  int* st = a.states + (long long)b * a.T;
  for (int t = threadIdx.x; t < a.T; t += blockDim.x) st[t] = -1;
  const int off = a.tgt_off[b];
  for (int u = threadIdx.x; u < U; u += blockDim.x) {
    a.tok_start[off + u] = -1;
    a.tok_end[off + u] = -1;
    a.tok_logp[off + u] = NEG_INF;
  }
}

// The forward pass with one pair per thread (j = threadIdx.x): WAVE takes the neighbour by DPP, otherwise through `rowO` (2 rows of
// blockDim.x + 1 floats, entry 0 of each the NEG_INF below pair 0).  Emissions come WPF frames ahead from clamped frame indices through
// vector loads (see ctc_lattice_wave_body).  Leaves the last frame's states in E, O.
template <int IS_LOG, bool WAVE, bool STAR>
__device__ __forceinline__ void align_forward_pairs(const AlignArgs& a, int b, int Tb, int U, const int* __restrict__ lab, float* rowO,
                                                    float& E, float& O) {
  const int j = threadIdx.x;
  const bool actE = j <= U, actO = j < U;
  int cls = 0;
  bool skip = false, star = false;
  if (actO) {
    cls = lab[j];
    skip = (j >= 1) && (cls != lab[j - 1]);
    if (STAR) {
      star = cls == a.C;
      cls = star ? 0 : cls;
    }
  }
  int vz;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
  const float* xb = a.x + (long long)b * a.ld_b + vz;
  // the odd state's emission: x[t][cls], or g[t] for the wildcard (one base and one stride per thread, chosen once)
  const float* ob = xb + cls;
  long long ld_o = a.ld_t;
  if (STAR && star) {
    ob = a.g + (long long)b * a.T + vz;
    ld_o = 1;
  }
  const int last = Tb - 1;
  auto fetch = [&](int i, float& xE, float& xO) {
    const int ii = i < last ? i : last;
    xE = xb[(long long)ii * a.ld_t];
    if constexpr (STAR) xO = ob[(long long)ii * ld_o];
    else xO = xb[(long long)ii * a.ld_t + cls];
  };
  const bool stores = j < a.Wp;
  unsigned* bpp = a.bp + (long long)b * a.NG * a.Wp + (stores ? j : 0);
  float* prev = rowO;
  float* cur = rowO + blockDim.x + 1;
  E = NEG_INF;
  O = NEG_INF;
  {
    float xE, xO;
    fetch(0, xE, xO);
    const bool first = j == 0 || (STAR && j == 1 && (align_flags<STAR>(a, b) & ALIGN_FREE_START));   // pair 1: the states 2 and 3
    if (first) {
      if (!STAR || actE) E = align_emit<IS_LOG>(xE);             // (pair 0 always has its even state)
      if (actO) O = align_emit_odd<IS_LOG, STAR>(xO, star);
    }
    if (!WAVE) {
      if (j == 0) prev[0] = cur[0] = NEG_INF;
      prev[j + 1] = O;
      __syncthreads();
    }
  }
  unsigned acc = 0;
  // a pair beyond the target gets the emission NEG_INF, which holds it at NEG_INF without a select on the chain
  auto frame = [&](float xE, float xO, int k) {
    const float eE = actE ? align_emit<IS_LOG>(xE) : NEG_INF, eO = actO ? align_emit_odd<IS_LOG, STAR>(xO, star) : NEG_INF;
    const float Om = WAVE ? wave_shift1<0x138>(O) : prev[j];
    acc |= align_cell(E, O, Om, skip, eE, eO) << (4 * k);
    if (!WAVE) {
      cur[j + 1] = O;
      __syncthreads();
      float* tmp = prev; prev = cur; cur = tmp;
    }
  };
  float rE[WPF], rO[WPF];
#pragma unroll
  for (int k = 0; k < WPF; ++k) fetch(1 + k, rE[k], rO[k]);
  int i0 = 1;
  for (; i0 + WPF <= Tb; i0 += WPF) {               // whole groups: slot k holds frame i0 + k = transition i0 - 1 + k of group (i0 - 1) >> 3
    acc = 0;
#pragma unroll
    for (int k = 0; k < WPF; ++k) {
      frame(rE[k], rO[k], k);
      fetch(i0 + k + WPF, rE[k], rO[k]);                     // after the slot's use: the refill lands in the same registers, no copies
    }
    if (stores) bpp[(long long)((i0 - 1) >> 3) * a.Wp] = acc;
  }
  if (i0 < Tb) {                                    // the last Tb - i0 < WPF frames are in the ring already
    acc = 0;
#pragma unroll
    for (int k = 0; k < WPF - 1; ++k)
      if (i0 + k < Tb) frame(rE[k], rO[k], k);
    if (stores) bpp[(long long)((i0 - 1) >> 3) * a.Wp] = acc;
  }
}

// More pairs than threads: rows of both states in LDS (E[2][Wp], O[2][Wp + 1], acc[Wp]), every thread loops over its pairs.
// Leaves the last frame's end states in fin[0] (state 2U) and fin[1] (state 2U - 1); STAR: also fin[2] (2U - 2) and fin[3] (2U - 3).
template <int IS_LOG, bool STAR>
__device__ __forceinline__ void align_forward_loop(const AlignArgs& a, int b, int Tb, int U, const int* __restrict__ lab, float* smem,
                                                   float* fin) {
  const int Wp = a.Wp;
  float* pE = smem;
  float* cE = smem + Wp;
  float* pO = smem + 2 * Wp;
  float* cO = pO + Wp + 1;
  unsigned* accs = reinterpret_cast<unsigned*>(cO + Wp + 1);
  const float* xb = a.x + (long long)b * a.ld_b;
  unsigned* bpp = a.bp + (long long)b * a.NG * Wp;
  const float* gb = STAR ? a.g + (long long)b * a.T : nullptr;
  const bool fstart = (align_flags<STAR>(a, b) & ALIGN_FREE_START) != 0;
  for (int j = threadIdx.x; j < Wp; j += blockDim.x) {
    float E = NEG_INF, O = NEG_INF;
    if (j == 0) {
      E = align_emit<IS_LOG>(xb[0]);
      if (U >= 1) O = (STAR && lab[0] == a.C) ? gb[0] : align_emit<IS_LOG>(xb[lab[0]]);
      pO[0] = cO[0] = NEG_INF;
    }
    if (STAR && fstart && j == 1 && U >= 1) {                    // the states 2 and 3
      E = align_emit<IS_LOG>(xb[0]);
      if (U >= 2) O = lab[1] == a.C ? gb[0] : align_emit<IS_LOG>(xb[lab[1]]);
    }
    pE[j] = E;
    pO[j + 1] = O;
    accs[j] = 0;
  }
  __syncthreads();
  for (int i = 1; i < Tb; ++i) {
    const int f = i - 1, k = f & 7;
    const float* xt = xb + (long long)i * a.ld_t;
    const bool flush = (k == 7) || (i == Tb - 1);
    for (int j = threadIdx.x; j <= U; j += blockDim.x) {
      const bool actO = j < U;
      const int cls = actO ? lab[j] : 0;
      const bool skip = actO && (j >= 1) && (cls != lab[j - 1]);
      const bool star = STAR && cls == a.C;
      float E = pE[j], O = pO[j + 1];
      const float eE = align_emit<IS_LOG>(xt[0]);
      const float eO = actO ? align_emit_odd<IS_LOG, STAR>(star ? gb[i] : xt[cls], star) : NEG_INF;
      const unsigned nib = align_cell(E, O, pO[j], skip, eE, eO);
      cE[j] = E;
      cO[j + 1] = O;
      const unsigned w = (k == 0 ? 0u : accs[j]) | (nib << (4 * k));
      accs[j] = w;
      if (flush) bpp[(long long)(f >> 3) * Wp + j] = w;
    }
    __syncthreads();
    float* tmp = pE; pE = cE; cE = tmp;
    tmp = pO; pO = cO; cO = tmp;
  }
  if (threadIdx.x == 0) {
    fin[0] = pE[U];
    fin[1] = U >= 1 ? pO[U] : NEG_INF;
    if (STAR) {
      fin[2] = U >= 1 ? pE[U - 1] : NEG_INF;
      fin[3] = U >= 2 ? pO[U - 1] : NEG_INF;
    }
  }
}

// The end of the path from the last frame's values l1 .. l4 of the states S - 1 .. S - 4 (NEG_INF where a state does not exist): the
// largest of the allowed ones, a tie going to the larger state.
template <bool STAR>
__device__ __forceinline__ void align_pick_end(int U, int flags, float l1, float l2, float l3, float l4, float& sc, int& end) {
  sc = l2 > l1 ? l2 : l1;
  end = l2 > l1 ? 2 * U - 1 : 2 * U;
  if (STAR && (flags & ALIGN_FREE_END)) {
    if (l3 > sc) { sc = l3; end = 2 * U - 2; }
    if (l4 > sc) { sc = l4; end = 2 * U - 3; }
  }
}

// Token spans and log-probabilities of the written states (all threads of the workgroup; the states are visible to them).
template <int IS_LOG, bool STAR>
__device__ __forceinline__ void align_spans(const AlignArgs& a, int b, int Tb, int U, const int* __restrict__ lab, const int* st) {
  const int tid = threadIdx.x;
  const int off = a.tgt_off[b];
  if (STAR) {                                                   // a first or last token that the path leaves out has no frame to write it
    if (tid == 0 && U >= 1) {
      a.tok_start[off] = a.tok_end[off] = -1;
      a.tok_start[off + U - 1] = a.tok_end[off + U - 1] = -1;
    }
    __syncthreads();
  }
  // token spans: frame t opens its token when the frame before is in another state, and closes it when the frame after is
  for (int t = tid; t < Tb; t += blockDim.x) {
    const int s = st[t];
    if (s & 1) {
      if (t == 0 || st[t - 1] != s) a.tok_start[off + (s >> 1)] = t;
      if (t == Tb - 1 || st[t + 1] != s) a.tok_end[off + (s >> 1)] = t + 1;
    }
  }
  __syncthreads();
  const float* xb = a.x + (long long)b * a.ld_b;
  for (int u = tid; u < U; u += blockDim.x) {
    int t0 = a.tok_start[off + u], t1 = a.tok_end[off + u];
    const int c = lab[u];
    if (STAR) {
      if (t0 < 0) {                                             // a skipped optional token
        a.tok_logp[off + u] = 0.f;
        continue;
      }
      if (c == a.C) {
        const float* gb = a.g + (long long)b * a.T;
        t0 = t0 < Tb ? t0 : Tb - 1;
        t1 = t1 < Tb ? t1 : Tb;
        float sum = gb[t0];
        for (int t = t0 + 1; t < t1; ++t) sum += gb[t];
        a.tok_logp[off + u] = sum;
        continue;
      }
    }
    t0 = t0 < 0 ? 0 : (t0 < Tb ? t0 : Tb - 1);                 // (a valid walk visits every token; no stray index either way)
    t1 = t1 < Tb ? t1 : Tb;
    float sum = align_emit<IS_LOG>(xb[(long long)t0 * a.ld_t + c]);
    for (int t = t0 + 1; t < t1; ++t) sum += align_emit<IS_LOG>(xb[(long long)t * a.ld_t + c]);
    a.tok_logp[off + u] = sum;
  }
}

// Wave 0 walks the back-pointers from (Tb - 1, end) to frame 0.  `stage` holds G = stage_words / Wp whole group rows per bulk copy.
__device__ __forceinline__ void align_backtrace(const AlignArgs& a, int b, int Tb, int end, unsigned* stage) {
  const int l = threadIdx.x, Wp = a.Wp;
  const unsigned* bpp = a.bp + (long long)b * a.NG * Wp;
  int* st = a.states + (long long)b * a.T;
  const int G = a.stage_words / Wp;
  int s = end, stv = -1;
  for (int gtop = (Tb - 2) >> 3; gtop >= 0; gtop -= G) {      // Tb == 1: no transition, no trip
    const int gbase = gtop - G + 1 > 0 ? gtop - G + 1 : 0;
    const int n = (gtop - gbase + 1) * Wp;
    const unsigned* src = bpp + (long long)gbase * Wp;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // the walk below has read the previous copy
    for (int idx = l; idx < n; idx += 64) stage[idx] = src[idx];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int ftop = gtop * 8 + 7 < Tb - 2 ? gtop * 8 + 7 : Tb - 2;
    for (int f = ftop; f >= gbase * 8; --f) {                 // the state of frame f + 1 is s
      stv = (l == (f & 63)) ? s : stv;
      if ((f & 63) == 0 && f + 1 + l < Tb) st[f + 1 + l] = stv;
      const unsigned w = stage[((f >> 3) - gbase) * Wp + (s >> 1)];
      s -= (w >> (4 * (f & 7) + 2 * (s & 1))) & 3u;
      s = s > 0 ? s : 0;                                      // (a valid walk never leaves the lattice; no stray index either way)
    }
  }
  if (l == 0) st[0] = s;
}

// MODE 0: one wavefront, 1: one workgroup with a pair per thread, 2: one workgroup looping over pairs
template <int IS_LOG, int MODE, bool STAR>
__device__ __forceinline__ void align_body(const AlignArgs& a, float* smem) {
  __shared__ float fin[STAR ? 4 : 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = a.in_lens ? min(a.in_lens[b], a.T) : a.T;
  const int U = a.tgt_lens[b];
  if (U < 0 || U > a.maxU) {                                   // outside what the workspace and the launch were sized for
    align_write_infeasible(a, b, U, NEG_INF);                  // (U < 0: no token entries)
    return;
  }
  const int* lab = a.targets + a.tgt_off[b];
  int bad = 0;
  for (int u = tid; u < U; u += blockDim.x) {
    const int c = lab[u];
    bad |= align_bad_label<STAR>(c, a.C);
  }
  bad = __syncthreads_or(bad);
  if (Tb <= 0 || bad) {
    align_write_infeasible(a, b, U, (U == 0 && !bad) ? 0.f : NEG_INF);
    return;
  }
  if (MODE == 2) {
    align_forward_loop<IS_LOG, STAR>(a, b, Tb, U, lab, smem, fin);
  } else {
    float E, O;
    align_forward_pairs<IS_LOG, MODE == 0, STAR>(a, b, Tb, U, lab, smem, E, O);
    if (tid == U) fin[0] = E;                                  // state S - 1 = 2U
    if (U >= 1 && tid == U - 1) fin[1] = O;                    // state S - 2
    if (STAR) {
      if (U >= 1 && tid == U - 1) fin[2] = E;                  // state S - 3
      if (U >= 2 && tid == U - 2) fin[3] = O;                  // state S - 4
    }
  }
  __syncthreads();                                             // also: the back-pointer stores have completed before wave 0 reads them
  const float l1 = fin[0], l2 = U >= 1 ? fin[1] : NEG_INF;
  const float l3 = (STAR && U >= 1) ? fin[STAR ? 2 : 0] : NEG_INF, l4 = (STAR && U >= 2) ? fin[STAR ? 3 : 0] : NEG_INF;
  float sc;
  int end;
  align_pick_end<STAR>(U, align_flags<STAR>(a, b), l1, l2, l3, l4, sc, end);
  if (sc == NEG_INF) {
    align_write_infeasible(a, b, U, NEG_INF);
    return;
  }
  int* st = a.states + (long long)b * a.T;
  for (int t = Tb + tid; t < a.T; t += blockDim.x) st[t] = -1;
  if (tid == 0) a.score[b] = sc;
  if (tid < 64) align_backtrace(a, b, Tb, end, reinterpret_cast<unsigned*>(smem));
  __syncthreads();
  align_spans<IS_LOG, STAR>(a, b, Tb, U, lab, st);
}

template <int IS_LOG, bool STAR>
__global__ __launch_bounds__(64) void ctc_align_wave_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  align_body<IS_LOG, 0, STAR>(a, smem);
}

template <int IS_LOG, int MODE, bool STAR>
__global__ __launch_bounds__(1024) void ctc_align_block_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  align_body<IS_LOG, MODE, STAR>(a, smem);
}

// The launch that both entries share (`who` names the entry in an error).  a.bp, a.g, a.flags and a.maxU are set by the caller.
template <bool STAR>
int align_launch(const char* who, AlignArgs& a, int B, int is_log, int variant, int max_target_len, void* stream) {
  a.Wp = max_target_len + 1;
  a.NG = ceil_div(a.T, 8);
  a.stage_words = a.Wp > ALIGN_STAGE_WORDS ? a.Wp : ALIGN_STAGE_WORDS;
  const size_t stage_bytes = (size_t)a.stage_words * sizeof(unsigned);
  hipStream_t s = (hipStream_t)stream;
  if (variant == 1 || (variant == 0 && 2 * max_target_len + 1 <= 128)) {
    if (is_log) hipLaunchKernelGGL((ctc_align_wave_kernel<1, STAR>), dim3(B), dim3(64), stage_bytes, s, a);
    else hipLaunchKernelGGL((ctc_align_wave_kernel<0, STAR>), dim3(B), dim3(64), stage_bytes, s, a);
    DS2_LAUNCH_CHECK("ctc_align_wave_kernel");
    return 0;
  }
  const int threads = a.Wp > 1024 ? 1024 : ceil_div(a.Wp, 64) * 64;
  const bool loop = a.Wp > threads;                 // more pairs than threads: MODE 2, with both rows and the accumulators in LDS
  size_t lds = (loop ? (size_t)5 * a.Wp + 2 : (size_t)2 * (threads + 1)) * sizeof(float);
  if (lds < stage_bytes) lds = stage_bytes;
  DS2_REQUIRE(!loop || lds <= 64 * 1024, "%s: target too long for LDS lattice rows (max_target_len=%d)", who, max_target_len);
  if (!loop && is_log) hipLaunchKernelGGL((ctc_align_block_kernel<1, 1, STAR>), dim3(B), dim3(threads), lds, s, a);
  else if (!loop) hipLaunchKernelGGL((ctc_align_block_kernel<0, 1, STAR>), dim3(B), dim3(threads), lds, s, a);
  else if (is_log) hipLaunchKernelGGL((ctc_align_block_kernel<1, 2, STAR>), dim3(B), dim3(threads), lds, s, a);
  else hipLaunchKernelGGL((ctc_align_block_kernel<0, 2, STAR>), dim3(B), dim3(threads), lds, s, a);
  DS2_LAUNCH_CHECK("ctc_align_block_kernel");
  return 0;
}

// What all four entries share (`who` names the entry in an error): the checks of their common arguments, and those arguments' fields of
// AlignArgs (the fields behind tok_logp: zero and null).  bp, g and flags, and every check of an entry's own, stay with the entry.
int align_entry_args(const char* who, AlignArgs& a, const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                     const int* targets, const int* tgt_off, const int* in_lens, const int* tgt_lens, int maxU, float* score, int* states,
                     int* tok_start, int* tok_end, float* tok_logp) {
  DS2_REQUIRE(x && tgt_off && tgt_lens && score && states, "%s: null pointer", who);
  DS2_REQUIRE(B > 0 && T > 0 && C > 0 && maxU >= 0 && ld_b > 0 && ld_t > 0, "%s: bad dims (B=%d T=%d C=%d U=%d)", who, B, T, C, maxU);
  DS2_REQUIRE(maxU == 0 || (targets && tok_start && tok_end && tok_logp), "%s: null target / token pointer", who);
  DS2_REQUIRE(is_log == 0 || is_log == 1, "%s: is_log must be 0 or 1", who);
  a = AlignArgs{x, ld_b, ld_t, T, C, targets, tgt_off, in_lens, tgt_lens, maxU, score, states, tok_start, tok_end, tok_logp};
  return 0;
}

}  // namespace

extern "C" size_t ds2_ctc_align_workspace_bytes(int B, int T, int max_target_len) {
  if (B <= 0 || T <= 0 || max_target_len < 0) return 0;
  return (size_t)B * (size_t)ceil_div(T, 8) * ((size_t)max_target_len + 1) * sizeof(unsigned);
}

extern "C" int ds2_ctc_align_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* targets_dev,
                                 const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, int variant,
                                 float* score, int* states, int* tok_start, int* tok_end, float* tok_logp, void* ws, size_t ws_bytes,
                                 void* stream) {
  AlignArgs a;
  if (int rc = align_entry_args("ds2_ctc_align_f32", a, x, ld_b, ld_t, B, T, C, is_log, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev,
                                max_target_len, score, states, tok_start, tok_end, tok_logp)) return rc;
  DS2_REQUIRE(variant >= 0 && variant <= 2, "ds2_ctc_align_f32: variant must be 0, 1 or 2");
  const int Smax = 2 * max_target_len + 1;
  DS2_REQUIRE(variant != 1 || Smax <= 128, "ds2_ctc_align_f32: variant 1 (one wavefront) needs 2 * max_target_len + 1 <= 128, got %d", Smax);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_align_workspace_bytes(B, T, max_target_len), "ds2_ctc_align_f32: workspace too small");
  a.bp = (unsigned*)ws;
  return align_launch<false>("ds2_ctc_align_f32", a, B, is_log, variant, max_target_len, stream);
}
