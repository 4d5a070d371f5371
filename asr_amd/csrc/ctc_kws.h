// Keyword search over CTC posteriors (ds2_ctc_kws_f32, contract in include/ds2hip.h): WHERE a phrase was said, and whether at all.
// The (max, +) lattice of ctc_align.h entered at any frame, on emissions taken relative to the frame's best class, so that a path's
// value is its log-likelihood ratio against the frame-wise best path.  Compiled inside ctc.hip's translation unit, after
// ctc_align_star.h, whose pre-pass (align_star_row_launch, penalty 0) writes the best-class row g.
//
// Lattice kernel: one wavefront per (utterance, keyword), pair j = states (2j, 2j + 1) on lane j as in the aligner's variant 1, the
// neighbour's odd state by the same one-lane DPP shift.  Every state carries its path's start frame beside its value; the start takes
// the selects that the value takes (align_cell's nibble says which move won) and never feeds back into a value.
//   The entering move costs nothing: DPP leaves lane 0, which has no lane below it, the `old` operand, and where the aligner puts
//   NEG_INF there this kernel puts the value 0 and the start t.  Lane 0's skip flag is set, so "enter" is the aligner's skip move from
//   a virtual state -1 of constant value 0: the last move in the tie order, taken on a strict > only.  State 0 does not exist: lane 0's
//   even state gets the emission NEG_INF like every state beyond the keyword.
//   There are no back-pointers, so nothing is sized by T x states and T has no limit.  The end state 2U - 1 lives on lane U - 1; per
//   frame its value and start are read into scalar registers (v_readlane, U is uniform) and kept by lane t & 63; 64 frames leave as two
//   256-byte stores.  Emissions and g come WPF frames ahead through vector loads, as in align_forward_pairs.
// Pick kernel (second launch, same stream): one wavefront per (utterance, keyword) compacts the frames at or above the threshold into a
// list in the workspace (ballot + prefix count, ascending t), then runs the greedy rounds on the list alone; a round's scan applies the
// previous winner's kill and finds the next winner in the same pass.
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_kws.h is a part of ctc.hip"
#endif
#include <type_traits>

namespace {

constexpr int KWS_MAX_LEN = 63, KWS_MAX_HITS = 1024;

struct KwsArgs {
  const float* x;
  long long ld_b, ld_t;
  int T, C, K;
  const int *in_lens, *kw_labels, *kw_off, *kw_lens;
  int maxU;
  const float* thr;
  int max_hits;
  float* fscore;         // [B][K][T]
  int* fstart;           // [B][K][T]
  int *hit_start, *hit_end;
  float* hit_score;      // [B][K][max_hits]
  int* n_hits;           // [B][K]
  const float* g;        // workspace: [B][T] the frame's best emission (a log value; frames t >= T_b unwritten)
  int* cand;             // workspace: [B][K][T] the compacted candidate frames of the pick
};

// lane l <- lane l - 1; lane 0 keeps `first`
__device__ __forceinline__ int kws_shift1(int first, int v) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// A = KwsArgs: the one-call search.  A = KwsStreamArgs (ctc_kws_stream.h): the streaming instance, which loads the four registers of
// every lane and the frames consumed so far (n0) from the state, counts the start frames from n0, and stores them after the last frame;
// every difference is under `if constexpr (STREAM)`.  Frame indices stay relative to the chunk (loads, the staging by l == (t & 63),
// the stores of the per-frame arrays): only the start that the entering move writes is absolute.
template <int IS_LOG, class A = KwsArgs>
__global__ __launch_bounds__(64) void ctc_kws_wave_kernel(A a) {
  constexpr bool STREAM = !std::is_same<A, KwsArgs>::value;
  const int l = threadIdx.x;
  const int b = blockIdx.x / a.K, k = blockIdx.x - b * a.K;
  const long long row = (long long)blockIdx.x * a.T;
  float* fs = a.fscore + row;
  int* fst = a.fstart + row;
  int Tb = a.in_lens ? min(a.in_lens[b], a.T) : a.T;
  float E = NEG_INF, O = NEG_INF;
  int sE = -1, sO = -1;
  int n0 = 0, Tadv = 0;                                          // STREAM: frames before this chunk, frames this chunk advances by
  if constexpr (STREAM) {
    n0 = a.stream_load(l, E, O, sE, sO);
    Tb = Tadv = max(min(Tb, 0x7fffffff - n0), 0);
  }
  const int U = __builtin_amdgcn_readfirstlane(a.kw_lens[k]);
  const int* lab = a.kw_labels + a.kw_off[k];
  bool ok = U >= 1 && U <= a.maxU && U <= KWS_MAX_LEN && Tb > 0;
  if (ok) {
    const int c = l < U ? lab[l] : 1;
    ok = !__any(c < 1 || c >= a.C);
  }
  if (!ok) Tb = 0;                                             // no keyword, a bad label, no frame: (-inf, -1) everywhere
  if (Tb > 0) {
    const bool actO = l < U, actE = l >= 1 && l < U;           // (state 0 does not exist)
    const int cls = actO ? lab[l] : 0;
    const bool skip = l == 0 || (actO && cls != lab[l - 1]);   // lane 0: the entering move
    const int ul = U - 1;
    int vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    const float* xb = a.x + (long long)b * a.ld_b + vz;
    const float* gb = a.g + (long long)b * a.T + vz;
    const int last = Tb - 1;
    auto fetch = [&](int i, float& xE, float& xO, float& gg) {  // frame index clamped: always a valid address
      const int ii = i < last ? i : last;
      xE = xb[(long long)ii * a.ld_t];
      xO = xb[(long long)ii * a.ld_t + cls];
      gg = gb[ii];
    };
    float sv = NEG_INF;
    int ss = -1;
    auto frame = [&](float xE, float xO, float gg, int t) {
      float dE, dO;
      {
#pragma clang fp contract(off)
        dE = align_emit<IS_LOG>(xE) - gg;
        dO = align_emit<IS_LOG>(xO) - gg;
      }
      dE = actE ? dE : NEG_INF;
      dO = actO ? dO : NEG_INF;
      const float Om = __int_as_float(kws_shift1(__float_as_int(0.f), __float_as_int(O)));
      const int sOm = kws_shift1(STREAM ? t + n0 : t, sO), sE0 = sE;
      const unsigned nib = align_cell(E, O, Om, skip, dE, dO);
      sE = (nib & 1u) ? sOm : sE0;
      sO = (nib & 8u) ? sOm : ((nib & 4u) ? sE0 : sO);
      // the end state's pair of this frame, kept by lane t & 63 until the block of 64 frames leaves
      const float ve = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(O), ul));
      const int se = __builtin_amdgcn_readlane(sO, ul);
      const bool mine = l == (t & 63);
      sv = mine ? ve : sv;
      ss = mine ? se : ss;
    };
    float rE[WPF], rO[WPF], rG[WPF];
#pragma unroll
    for (int q = 0; q < WPF; ++q) fetch(q, rE[q], rO[q], rG[q]);
    int t0 = 0;
    for (; t0 + WPF <= Tb; t0 += WPF) {                          // whole groups: slot q holds frame t0 + q, refilled with t0 + q + WPF
#pragma unroll
      for (int q = 0; q < WPF; ++q) {
        frame(rE[q], rO[q], rG[q], t0 + q);
        fetch(t0 + q + WPF, rE[q], rO[q], rG[q]);
      }
      if (((t0 + WPF) & 63) == 0) {                              // 64 frames are complete: one store of each array, a contiguous run
        const int t = t0 + WPF - 64 + l;
        fs[t] = sv;
        fst[t] = sv == NEG_INF ? -1 : ss;
      }
    }
#pragma unroll
    for (int q = 0; q < WPF - 1; ++q)                            // the last Tb - t0 < WPF frames are in the ring already
      if (t0 + q < Tb) frame(rE[q], rO[q], rG[q], t0 + q);
    const int t = (Tb & ~63) + l;                                // the last, partial block
    if (t < Tb) {
      fs[t] = sv;
      fst[t] = sv == NEG_INF ? -1 : ss;
    }
  }
  for (int t = Tb + l; t < a.T; t += 64) {
    fs[t] = NEG_INF;
    fst[t] = -1;
  }
  if constexpr (STREAM) a.stream_save(l, k, n0, Tadv, E, O, sE, sO);
}

__global__ __launch_bounds__(64) void ctc_kws_pick_kernel(KwsArgs a) {
  const int l = threadIdx.x;
  const int k = blockIdx.x % a.K;
  const long long row = (long long)blockIdx.x * a.T;
  const float* fs = a.fscore + row;
  const int* fst = a.fstart + row;
  int* cand = a.cand + row;
  const float thr = a.thr[k];
  int n = 0;
  for (int t0 = 0; t0 < a.T; t0 += 64) {                         // compaction, ascending t
    const int t = t0 + l;
    bool c = false;
    if (t < a.T) {
      const float v = fs[t];
      c = v > NEG_INF && v >= thr;
    }
    const unsigned long long m = __ballot(c);
    if (c) cand[n + __popcll(m & ((1ull << l) - 1ull))] = t;
    n += __popcll(m);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");         // the list is read by other lanes than wrote it
  __builtin_amdgcn_wave_barrier();
  const long long hrow = (long long)blockIdx.x * a.max_hits;
  int nh = 0, pt = -1, ps = 0;                                   // [ps, pt]: the span of the previous winner (pt < 0: none yet)
  for (int h = 0; h <= a.max_hits; ++h) {
    float bv = NEG_INF;
    int bt = 0x7fffffff, bs = -1;
    for (int i = l; i < n; i += 64) {                            // (a lane reads and kills its own entries only)
      const int t = cand[i];
      if (t < 0) continue;
      const int s = fst[t];
      if (pt >= 0 && s <= pt && ps <= t) {
        cand[i] = -1;
        continue;
      }
      const float v = fs[t];
      if (v > bv) { bv = v; bt = t; bs = s; }                    // ascending t within a lane: a tie keeps the smaller t
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int ot = __shfl_xor(bt, o), os = __shfl_xor(bs, o);
      if (ov > bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; bs = os; }
    }
    if (bt == 0x7fffffff) break;                                 // no live candidate
    if (h == a.max_hits) {                                       // a live candidate beyond the last slot
      nh = a.max_hits + 1;
      break;
    }
    if (l == 0) {
      a.hit_start[hrow + h] = bs;
      a.hit_end[hrow + h] = bt + 1;
      a.hit_score[hrow + h] = bv;
    }
    nh = h + 1;
    pt = bt;
    ps = bs;
  }
  for (int h = (nh < a.max_hits ? nh : a.max_hits) + l; h < a.max_hits; h += 64) {
    a.hit_start[hrow + h] = -1;
    a.hit_end[hrow + h] = -1;
    a.hit_score[hrow + h] = NEG_INF;
  }
  if (l == 0) a.n_hits[blockIdx.x] = nh;
}

}  // namespace

extern "C" size_t ds2_ctc_kws_workspace_bytes(int B, int T, int K, int max_hits) {
  if (B <= 0 || T <= 0 || K <= 0 || max_hits < 1 || max_hits > KWS_MAX_HITS) return 0;
  return ((size_t)B * (size_t)T + (size_t)B * (size_t)K * (size_t)T) * sizeof(float);
}

extern "C" int ds2_ctc_kws_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* in_lens_dev,
                               const int* kw_labels_dev, const int* kw_off_dev, const int* kw_lens_dev, int K, int max_kw_len,
                               const float* thr_dev, int max_hits, float* frame_score, int* frame_start, int* hit_start, int* hit_end,
                               float* hit_score, int* n_hits, void* ws, size_t ws_bytes, void* stream) {
  DS2_REQUIRE(x && kw_off_dev && kw_lens_dev && thr_dev && frame_score && frame_start && hit_start && hit_end && hit_score && n_hits,
              "ds2_ctc_kws_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && C > 0 && K > 0 && ld_b > 0 && ld_t > 0 && (long long)B * K <= 0x7fffffffLL,
              "ds2_ctc_kws_f32: bad dims (B=%d T=%d C=%d K=%d)", B, T, C, K);
  DS2_REQUIRE(max_kw_len >= 0 && max_kw_len <= KWS_MAX_LEN,
              "ds2_ctc_kws_f32: max_kw_len must lie in [0, %d] (one wavefront, two states per lane), got %d", KWS_MAX_LEN, max_kw_len);
  DS2_REQUIRE(max_kw_len == 0 || kw_labels_dev, "ds2_ctc_kws_f32: null keyword labels");
  DS2_REQUIRE(is_log == 0 || is_log == 1, "ds2_ctc_kws_f32: is_log must be 0 or 1");
  DS2_REQUIRE(max_hits >= 1 && max_hits <= KWS_MAX_HITS, "ds2_ctc_kws_f32: max_hits must lie in [1, %d], got %d", KWS_MAX_HITS, max_hits);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_kws_workspace_bytes(B, T, K, max_hits), "ds2_ctc_kws_f32: workspace too small");
  float* g = (float*)ws;
  if (int rc = align_star_row_launch(x, ld_b, ld_t, B, T, C, is_log, in_lens_dev, 0.f, g, stream)) return rc;
  KwsArgs a{x, ld_b, ld_t, T, C, K, in_lens_dev, kw_labels_dev, kw_off_dev, kw_lens_dev, max_kw_len, thr_dev, max_hits, frame_score,
            frame_start, hit_start, hit_end, hit_score, n_hits, g, (int*)(g + (size_t)B * (size_t)T)};
  const dim3 grid((unsigned)(B * K));
  hipStream_t s = (hipStream_t)stream;
  if (is_log) hipLaunchKernelGGL(ctc_kws_wave_kernel<1>, grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(ctc_kws_wave_kernel<0>, grid, dim3(64), 0, s, a);
  DS2_LAUNCH_CHECK("ctc_kws_wave_kernel");
  hipLaunchKernelGGL(ctc_kws_pick_kernel, grid, dim3(64), 0, s, a);
  DS2_LAUNCH_CHECK("ctc_kws_pick_kernel");
  return 0;
}
