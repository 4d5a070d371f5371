// CTC forced alignment of long recordings (ds2_ctc_align_tiled_f32, contract in include/ds2hip.h): the lattice of ctc_align.h cut into
// tiles of (tile_pairs state pairs) x (tile_frames frames) and spread over the GPU.  Compiled inside ctc.hip's translation unit, after
// ctc_align.h, whose cell (align_cell), emission (align_emit), arguments (AlignArgs) and back-pointer layout (bp[g * Wp + j]) it shares:
// every value is computed by the same expressions, so the outputs are the same bits.
//
// Tile (k, fb) of an utterance owns the pairs [k P, k P + P) (one per thread) over the frames [fb TF + 1, fb TF + TF] (transitions
// fb TF .. fb TF + TF - 1: with TF a multiple of 8 every back-pointer dword has one writer); block 0 also sets up frame 0.  It needs
//   from tile (k, fb - 1) the E / O of its pairs at frame fb TF:                            carry[b][j] (2 floats per pair), which the
//                                                                                           same tile position overwrites at its end;
//   from tile (k - 1, fb) the odd state of that tile's top pair at the frames fb TF .. fb TF + TF - 1 (the first of them written by
//   tile (k - 1, fb - 1)):                                                                  col[b][k - 1][t] (K x T floats).
// So the tiles with k + fb = d are independent: ONE LAUNCH PER ANTI-DIAGONAL d, a grid of (tiles of the diagonal) x B, and the kernel boundary
// is the only synchronisation between workgroups (no flags, no polling, no co-residency assumption).  Inside a tile the neighbour's
// value comes through an LDS row and one barrier per frame, or, with one wavefront per tile (P = 64), through a one-lane DPP shift.
// A tile outside its utterance's (T_b, U_b) extent returns at once, and so does one that no legal path can touch: every state above
// 2t + 1 (its readers then see the -inf that the hand-off arrays are filled with, which is the true value), or every state too low to
// reach state S - 2 by frame T_b - 1 (its readers then compute cells that cannot reach the end either: no value and no back-pointer
// on an optimal path depends on them).  The values of states S - 1 and S - 2 at frame T_b - 1 are captured by the tile that passes them.
// The backtrace is one further launch, one workgroup per utterance: a group row no longer fits LDS, but the state falls by at most 2
// per frame, so it stages, for TILED_BT_GROUPS groups at a time, the window of 8 * groups + 1 pairs below the current one.
// STAR (ds2_ctc_align_star_tiled_f32, entry in ctc_align_star.h): the wildcard label and the optional ends of ctc_align.h.  An utterance
// that may start in the states 2 and 3 reaches every state up to 2t + 3, and one that may end in S - 3 and S - 4 needs only state S - 4
// by frame T_b - 1: the two skip tests move by one pair, per utterance, and four end values are captured (fin has 4 floats each).
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_align_tiled.h is a part of ctc.hip"
#endif

namespace {

constexpr int TILED_DEFAULT_FRAMES = 64;                               // 64 x 64: the fastest shape measured, at 20 000 frames and at an hour
constexpr int TILED_DEFAULT_PAIRS = 64;                                // (scripts/time_align_long.py, profiles/align_long_timing.txt)
constexpr int TILED_RING = 16;                                        // frames of emissions in flight per thread: two back-pointer groups
constexpr int TILED_BT_GROUPS = 32;                                   // groups of 8 transitions per staged window
constexpr int TILED_BT_PAIRS = 8 * TILED_BT_GROUPS + 1;               // pairs the state can cross in them, plus its own
constexpr int TILED_BT_THREADS = 512;

struct AlignTiledArgs {
  AlignArgs a;           // a.bp [B][NG][Wp] as in ctc_align.h (stage_words unused)
  float* col;            // [B][K][T]   odd state of tile k's top pair per frame
  float* carry;          // [B][K * P][2]  E, O of every pair at the last frame of the frame block before
  float* fin;            // [B][2]      states S - 1 and S - 2 at frame T_b - 1 (STAR: [B][4], down to S - 4)
  int B, K, TF;
  int k_lo, d;           // this launch: block = tile * B + b, tiles k = k_lo + tile, fb = d - k
};

__global__ __launch_bounds__(256) void ctc_align_tiled_fill_kernel(float* p, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = NEG_INF;
}

// lane l <- lane l - 1, lane 0 <- old
__device__ __forceinline__ float wave_shift_up_old(float v, float old) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

template <int IS_LOG, bool WAVE, bool STAR>
__device__ __forceinline__ void align_tile_body(const AlignTiledArgs& ta, float* rowO) {
  const AlignArgs& a = ta.a;
  const int b = blockIdx.x % ta.B, k = ta.k_lo + blockIdx.x / ta.B, fb = ta.d - k;
  const int p = threadIdx.x, P = blockDim.x;
  const int Tb = a.in_lens ? min(a.in_lens[b], a.T) : a.T;
  const int U = a.tgt_lens[b];
  if (U < 0 || U > a.maxU || Tb <= 0) return;                          // (the backtrace launch writes the infeasible outputs)
  const int j0 = k * P;
  const long long t0 = (long long)fb * ta.TF;                           // the frame that the carry holds
  if (j0 > U || (fb > 0 && t0 >= Tb - 1)) return;                       // outside the utterance (block 0 always sets up frame 0)
  const int tl = (int)(t0 + ta.TF < Tb - 1 ? t0 + ta.TF : Tb - 1);      // the tile's last frame
  const int fl = align_flags<STAR>(a, b);
  const int free_s = (fl & ALIGN_FREE_START) ? 1 : 0, free_e = (fl & ALIGN_FREE_END) ? 1 : 0;
  if (j0 > tl + free_s) return;                                        // every state 2 j0 .. lies above 2 tl + 1 (free start: 2 tl + 3)
  const int jtop = j0 + P - 1;
  if (jtop < U && 2 * (long long)jtop + 1 + 2 * ((long long)Tb - 1 - t0) < 2 * (long long)U - 1 - 2 * free_e) return;   // cannot reach S - 2 (free end: S - 4)
  const int j = j0 + p;
  const bool actE = j <= U, actO = j < U;
  const int* __restrict__ lab = a.targets + a.tgt_off[b];
  int cls = 0;
  bool skip = false, star = false;
  if (actO) {
    cls = lab[j];
    skip = (j >= 1) && (cls != lab[j - 1]);
    star = STAR && cls == a.C;
    cls = (cls < 1 || cls >= a.C) ? 0 : cls;                           // a bad label: the utterance is infeasible, nothing is read out of bounds
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
  const bool below = k > 0;                                            // (uniform) there is a tile below: every thread loads its column
                                                                       // entry from the one address, thread / lane 0 is the one that uses it
  const float* colr = ta.col + ((long long)b * ta.K + (k > 0 ? k - 1 : 0)) * a.T;
  float* colw = ta.col + ((long long)b * ta.K + k) * a.T;
  const bool top = p == P - 1;
  auto fetch = [&](int i, float& xE, float& xO, float& xB) {
    const int ii = i < tl ? i : tl;
    xE = xb[(long long)ii * a.ld_t];
    if constexpr (STAR) xO = ob[(long long)ii * ld_o];
    else xO = xb[(long long)ii * a.ld_t + cls];
    xB = below ? colr[ii] : NEG_INF;
  };
  const bool stores = j < a.Wp;
  unsigned* bpp = a.bp + (long long)b * a.NG * a.Wp + (stores ? j : 0);
  float2* cr = reinterpret_cast<float2*>(ta.carry) + (long long)b * ta.K * P + j;
  float E = NEG_INF, O = NEG_INF;
  if (fb == 0) {
    if (j == 0 || (STAR && free_s && j == 1)) {                          // pair 1: the states 2 and 3
      if (!STAR || actE) E = align_emit<IS_LOG>(xb[0]);                  // (pair 0 always has its even state)
      if (actO) O = align_emit_odd<IS_LOG, STAR>(STAR ? ob[0] : xb[cls], star);
    }
    if (top) colw[0] = O;
  } else {
    const float2 c = *cr;
    E = c.x;
    O = c.y;
  }
  float bprev = below ? colr[t0] : NEG_INF;                            // the odd state below pair j0 in the frame before
  float* prev = rowO;
  float* cur = rowO + P + 1;
  if (!WAVE) {
    if (p == 0) prev[0] = bprev;
    prev[p + 1] = O;
    __syncthreads();
  }
  unsigned acc = 0;
  float oc[8];                                                         // the group's odd states: the top pair's go to the column, 8 at a time
  auto frame = [&](float xE, float xO, float xB, int kk) {
    const float eE = actE ? align_emit<IS_LOG>(xE) : NEG_INF, eO = actO ? align_emit_odd<IS_LOG, STAR>(xO, star) : NEG_INF;
    const float Om = WAVE ? wave_shift_up_old(O, bprev) : prev[p];
    acc |= align_cell(E, O, Om, skip, eE, eO) << (4 * kk);
    oc[kk] = O;
    if (WAVE) {
      bprev = xB;
    } else {
      if (p == 0) cur[0] = xB;
      cur[p + 1] = O;
      __syncthreads();
      float* tmp = prev; prev = cur; cur = tmp;
    }
  };
  const int Te = tl + 1;
  float rE[TILED_RING], rO[TILED_RING], rB[TILED_RING];
  int i0 = (int)t0 + 1;
#pragma unroll
  for (int kk = 0; kk < TILED_RING; ++kk) fetch(i0 + kk, rE[kk], rO[kk], rB[kk]);
  for (; i0 + TILED_RING <= Te; i0 += TILED_RING) {  // slot h * 8 + kk holds frame i0 + h * 8 + kk = transition kk of group ((i0 - 1) >> 3) + h
#pragma unroll
    for (int h = 0; h < TILED_RING / 8; ++h) {
      acc = 0;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int sl = h * 8 + kk;
        frame(rE[sl], rO[sl], rB[sl], kk);
        fetch(i0 + sl + TILED_RING, rE[sl], rO[sl], rB[sl]);      // after the slot's use: the refill lands in the same registers
      }
      if (stores) bpp[(long long)(((i0 - 1) >> 3) + h) * a.Wp] = acc;
      if (top) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) colw[i0 + h * 8 + kk] = oc[kk];
      }
    }
  }
#pragma unroll
  for (int h = 0; h < TILED_RING / 8; ++h) {         // the last Te - i0 < TILED_RING frames are in the ring already
    if (i0 + h * 8 < Te) {
      acc = 0;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int sl = h * 8 + kk;
        if (i0 + sl < Te) frame(rE[sl], rO[sl], rB[sl], kk);
      }
      if (stores) bpp[(long long)(((i0 - 1) >> 3) + h) * a.Wp] = acc;
      if (top) {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
          if (i0 + h * 8 + kk < Te) colw[i0 + h * 8 + kk] = oc[kk];
      }
    }
  }
  if (tl == Tb - 1) {
    constexpr int NF = STAR ? 4 : 2;
    if (j == U) ta.fin[NF * b] = E;
    if (j == U - 1) ta.fin[NF * b + 1] = O;
    if (STAR) {
      if (j == U - 1) ta.fin[NF * b + 2] = E;
      if (j == U - 2) ta.fin[NF * b + 3] = O;
    }
  } else {
    *cr = make_float2(E, O);
  }
}

template <int IS_LOG, bool STAR>
__global__ __launch_bounds__(64) void ctc_align_tile_wave_kernel(AlignTiledArgs ta) {
  align_tile_body<IS_LOG, true, STAR>(ta, nullptr);
}

template <int IS_LOG, bool STAR>
__global__ __launch_bounds__(1024) void ctc_align_tile_block_kernel(AlignTiledArgs ta) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  align_tile_body<IS_LOG, false, STAR>(ta, smem);
}

// The walk from (Tb - 1, end) to frame 0 through a moving window: for the groups [gbase, gtop] the whole workgroup stages the pairs
// [jlo, jhi], jhi the pair of the state at the top of the window and jlo = jhi - 8 * groups (the walk cannot leave them), every thread
// issuing its loads back to back; then wave 0 walks them and hands the state it reached to the next window through `sh_s`.
__device__ __forceinline__ void align_tiled_backtrace(const AlignArgs& a, int b, int Tb, int end, unsigned* stage, int* sh_s) {
  constexpr int NL = (TILED_BT_GROUPS * TILED_BT_PAIRS + TILED_BT_THREADS - 1) / TILED_BT_THREADS;
  const int tid = threadIdx.x, l = tid & 63, Wp = a.Wp;
  const unsigned* bpp = a.bp + (long long)b * a.NG * Wp;
  int* st = a.states + (long long)b * a.T;
  int s = __builtin_amdgcn_readfirstlane(end);      // wave-uniform, and kept in scalar registers by the walk
  if (tid == 0) *sh_s = end;
  for (int gtop = (Tb - 2) >> 3; gtop >= 0; gtop -= TILED_BT_GROUPS) {   // Tb == 1: no transition, no trip
    __syncthreads();                                          // sh_s is written, and the walk has read the previous window
    const int gbase = gtop - TILED_BT_GROUPS + 1 > 0 ? gtop - TILED_BT_GROUPS + 1 : 0;
    const int ng = gtop - gbase + 1;
    const int jhi = *sh_s >> 1;
    const int jlo = jhi - (TILED_BT_PAIRS - 1) > 0 ? jhi - (TILED_BT_PAIRS - 1) : 0;
    const int wn = jhi - jlo + 1;
    const unsigned* src = bpp + (long long)gbase * Wp + jlo;
    unsigned v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * TILED_BT_THREADS, r = idx / TILED_BT_PAIRS, c = idx - r * TILED_BT_PAIRS;
      v[i] = (r < ng && c < wn) ? src[(long long)r * Wp + c] : 0u;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * TILED_BT_THREADS;
      if (idx < TILED_BT_GROUPS * TILED_BT_PAIRS) stage[idx] = v[i];
    }
    __syncthreads();
    if (tid < 64) {
      // per group, lane i takes the dword of the pair i below the current one with one LDS read; the state is wave-uniform, so the
      // eight transitions of the group are scalar: a lane read and a few scalar operations each, no LDS latency on the chain
      for (int g = gtop; g >= gbase; --g) {
        const int c0 = (s >> 1) - jlo;
        const int ci = c0 - l > 0 ? c0 - l : 0;
        const unsigned wv = stage[(g - gbase) * TILED_BT_PAIRS + ci];
#pragma unroll
        for (int kk = 7; kk >= 0; --kk) {
          if (g * 8 + kk <= Tb - 2) {                         // (false only in the top group) the state of frame g * 8 + kk + 1 is s
            st[g * 8 + kk + 1] = s;                           // every lane stores the one value to the one address: no branch on the chain
            int d = c0 - ((s >> 1) - jlo);                    // 0 .. 7 on a valid walk: the state falls by at most 2 per transition
            d = d < 0 ? 0 : (d > 63 ? 63 : d);                // (no stray lane either way)
            const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, d);
            s -= (int)((w >> (4 * kk + 2 * (s & 1))) & 3u);
            s = s > 0 ? s : 0;
          }
        }
      }
      if (l == 0) *sh_s = s;
    }
  }
  if (tid == 0) st[0] = s;
}

// One workgroup per utterance: the feasibility checks of align_body, the end state from the captured values, the walk, and the span
// pass of ctc_align.h (the same expressions on the same values).
template <int IS_LOG, bool STAR>
__global__ __launch_bounds__(TILED_BT_THREADS) void ctc_align_tiled_backtrace_kernel(AlignTiledArgs ta) {
  __shared__ unsigned stage[TILED_BT_GROUPS * TILED_BT_PAIRS];
  __shared__ int sh_s;
  const AlignArgs& a = ta.a;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = a.in_lens ? min(a.in_lens[b], a.T) : a.T;
  const int U = a.tgt_lens[b];
  if (U < 0 || U > a.maxU) {
    align_write_infeasible(a, b, U, NEG_INF);
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
  constexpr int NF = STAR ? 4 : 2;
  const float l1 = ta.fin[NF * b], l2 = U >= 1 ? ta.fin[NF * b + 1] : NEG_INF;
  const float l3 = (STAR && U >= 1) ? ta.fin[NF * b + (STAR ? 2 : 0)] : NEG_INF, l4 = (STAR && U >= 2) ? ta.fin[NF * b + (STAR ? 3 : 0)] : NEG_INF;
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
  align_tiled_backtrace(a, b, Tb, end, stage, &sh_s);
  __syncthreads();
  align_spans<IS_LOG, STAR>(a, b, Tb, U, lab, st);
}

// 0 / 0 -> the defaults; false when the shape is not a legal one
inline bool align_tiled_shape(int& tile_frames, int& tile_pairs) {
  if (tile_frames == 0) tile_frames = TILED_DEFAULT_FRAMES;
  if (tile_pairs == 0) tile_pairs = TILED_DEFAULT_PAIRS;
  return tile_frames > 0 && tile_frames % 8 == 0 && tile_pairs > 0 && tile_pairs % 64 == 0 && tile_pairs <= 1024;
}

struct AlignTiledLayout {
  size_t bp_words, col_words, carry_words, fin_words;
  int K, F, NG, Wp;
};

inline AlignTiledLayout align_tiled_layout(int B, int T, int max_target_len, int tile_frames, int tile_pairs, bool star = false) {
  AlignTiledLayout L;
  L.Wp = max_target_len + 1;
  L.NG = ceil_div(T, 8);
  L.K = ceil_div(L.Wp, tile_pairs);
  L.F = T > 1 ? (int)(((long long)T - 2) / tile_frames) + 1 : 1;
  L.bp_words = (size_t)B * (size_t)L.NG * (size_t)L.Wp;
  L.col_words = (size_t)B * (size_t)L.K * (size_t)T;
  L.carry_words = (size_t)B * (size_t)L.K * (size_t)tile_pairs * 2;
  L.fin_words = (size_t)B * (star ? 4 : 2);
  return L;
}

// The launches that both entries share (`who` names the entry in an error): the fill, one launch per anti-diagonal, the backtrace.
// `ws` holds carry, fin, col and the back-pointers in this order (STAR: the caller keeps g behind them); a.g, a.flags and a.maxU are the
// caller's.
template <bool STAR>
int align_tiled_launch(const char* who, const AlignArgs& a0, int B, int is_log, int max_target_len, int tile_frames, int tile_pairs,
                       float* ws, void* stream) {
  const AlignTiledLayout L = align_tiled_layout(B, a0.T, max_target_len, tile_frames, tile_pairs, STAR);
  AlignTiledArgs ta;
  ta.a = a0;
  AlignArgs& a = ta.a;
  ta.carry = ws;                                       // (read and written as float2: an even number of words from the aligned base)
  ta.fin = ta.carry + L.carry_words;
  ta.col = ta.fin + L.fin_words;
  a.bp = (unsigned*)(ta.col + L.col_words);
  a.Wp = L.Wp; a.NG = L.NG; a.stage_words = 0;
  ta.B = B; ta.K = L.K; ta.TF = tile_frames;
  DS2_REQUIRE((long long)B * (L.K < L.F ? L.K : L.F) <= 0x7fffffffLL, "%s: too many tiles on one anti-diagonal", who);
  hipStream_t s = (hipStream_t)stream;
  {
    const long long n = (long long)(L.col_words + L.carry_words + L.fin_words);
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(ctc_align_tiled_fill_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, ta.carry, n);
    DS2_LAUNCH_CHECK("ctc_align_tiled_fill_kernel");
  }
  const size_t lds = (size_t)2 * (tile_pairs + 1) * sizeof(float);
  for (int d = 0; d < L.K + L.F - 1; ++d) {
    ta.d = d;
    ta.k_lo = d - L.F + 1 > 0 ? d - L.F + 1 : 0;
    const int k_hi = d < L.K - 1 ? d : L.K - 1;
    const dim3 grid((unsigned)(k_hi - ta.k_lo + 1) * (unsigned)B);
    if (tile_pairs == 64) {
      if (is_log) hipLaunchKernelGGL((ctc_align_tile_wave_kernel<1, STAR>), grid, dim3(64), 0, s, ta);
      else hipLaunchKernelGGL((ctc_align_tile_wave_kernel<0, STAR>), grid, dim3(64), 0, s, ta);
    } else {
      if (is_log) hipLaunchKernelGGL((ctc_align_tile_block_kernel<1, STAR>), grid, dim3(tile_pairs), lds, s, ta);
      else hipLaunchKernelGGL((ctc_align_tile_block_kernel<0, STAR>), grid, dim3(tile_pairs), lds, s, ta);
    }
    DS2_LAUNCH_CHECK("ctc_align_tile_kernel");
  }
  if (is_log) hipLaunchKernelGGL((ctc_align_tiled_backtrace_kernel<1, STAR>), dim3(B), dim3(TILED_BT_THREADS), 0, s, ta);
  else hipLaunchKernelGGL((ctc_align_tiled_backtrace_kernel<0, STAR>), dim3(B), dim3(TILED_BT_THREADS), 0, s, ta);
  DS2_LAUNCH_CHECK("ctc_align_tiled_backtrace_kernel");
  return 0;
}

}  // namespace

extern "C" size_t ds2_ctc_align_tiled_workspace_bytes(int B, int T, int max_target_len, int tile_frames, int tile_pairs) {
  if (B <= 0 || T <= 0 || max_target_len < 0 || !align_tiled_shape(tile_frames, tile_pairs)) return 0;
  const AlignTiledLayout L = align_tiled_layout(B, T, max_target_len, tile_frames, tile_pairs);
  return (L.bp_words + L.col_words + L.carry_words + L.fin_words) * sizeof(float);
}

extern "C" int ds2_ctc_align_tiled_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                                       const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                                       int max_target_len, int tile_frames, int tile_pairs, float* score, int* states, int* tok_start,
                                       int* tok_end, float* tok_logp, void* ws, size_t ws_bytes, void* stream) {
  AlignArgs a;
  if (int rc = align_entry_args("ds2_ctc_align_tiled_f32", a, x, ld_b, ld_t, B, T, C, is_log, targets_dev, tgt_off_dev, in_lens_dev,
                                tgt_lens_dev, max_target_len, score, states, tok_start, tok_end, tok_logp)) return rc;
  DS2_REQUIRE(align_tiled_shape(tile_frames, tile_pairs),
              "ds2_ctc_align_tiled_f32: tile_frames must be a positive multiple of 8 and tile_pairs a positive multiple of 64 up to 1024 "
              "(or 0 for the default), got %d x %d", tile_frames, tile_pairs);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_align_tiled_workspace_bytes(B, T, max_target_len, tile_frames, tile_pairs),
              "ds2_ctc_align_tiled_f32: workspace too small");
  return align_tiled_launch<false>("ds2_ctc_align_tiled_f32", a, B, is_log, max_target_len, tile_frames, tile_pairs, (float*)ws, stream);
}
