// Word and character confidences (ds2_ctc_conf_f32, contract in include/ds2hip.h): for a hypothesis y and a unit = (labels [lo, hi),
// frames [ts, te)), the probability that the whole utterance spells y given that the frames outside the window spell the rest of y.
// Compiled inside ctc.hip's translation unit: alpha / beta are the MW = true instances of ctc_lattice_wave_kernel / ctc_lattice_kernel
// at K = 1 behind the plain entry's ctc_lse_kernel (both directions always run there).  What is new here:
//   ctc_conf_kernel  grid (unit slot, utterance), ONE wavefront per unit.  The unit's states are [2lo-1, 2hi+1]: lane j <= hi - lo
//                    holds the pair O = state 2(lo+j)-1 (label lo+j-1) and E = state 2(lo+j) (blank), and every lane carries X = state
//                    2hi+1 (label hi), which inside the window only stays where it is: at most 63 labels fill the 64 lanes.  beta'
//                    is swept back from frame te to ts with the lattice's cell, one lane shift (DPP) per frame; then lane 0 forms
//                    num, A and Bq.  Windows are tens of frames: the dependent chain is short and nothing is scanned in parallel.
// Operand order of every log-sum-exp (a0 = the state itself, a1 = state + 1, a2 = state + 2; the bits are defined by it):
//   cell of O            lse3(O, E, skip ? O' : -inf) + emission      O' = lane j + 1's O, X for the top lane j = hi - lo
//   cell of E            lse2(E, O') + emission
//   cell of X            X + emission                                 (= lse3(X, -inf, -inf) + emission, the same bits)
//   Bq                   lse2(beta[te][2hi], beta[te][2hi+1])
//   A                    lse2(alpha[ts-1][2lo-1], alpha[ts-1][2lo])
//   num, ts > 0          lse2(alpha[ts-1][2lo-1] + lse3(b'[2lo-1], b'[2lo], skip ? b'[2lo+1] : -inf), alpha[ts-1][2lo] + lse2(b'[2lo], b'[2lo+1]))
//   num, ts = 0          lse2(b'[0], b'[1])
//   logconf              min(0, num - (A + Bq))
// Workspace: lse (T, B) | alpha / beta [2][B][T][Smax], Smax = 2 max_hyp_len + 1.
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_conf.h is a part of ctc.hip"
#endif
#include <limits.h>

namespace {

constexpr int CONF_MAX_UNIT = 63;                             // labels of one unit: hi - lo + 1 state pairs in 64 lanes
constexpr int CONF_PF = 4;                                    // frames of emissions in flight

__global__ __launch_bounds__(64) void ctc_conf_kernel(const float* __restrict__ logits, int ld, int T, int Bn, int C,
                                                      const int* __restrict__ hyps, const long long* __restrict__ off64,
                                                      const int* __restrict__ lens, const int* __restrict__ in_lens,
                                                      const float* __restrict__ lse, const float* __restrict__ ab, int Smax,
                                                      const int* __restrict__ n_units, const int* __restrict__ unit_lo,
                                                      const int* __restrict__ unit_hi, const int* __restrict__ win_start,
                                                      const int* __restrict__ win_end, int Wmax, float* __restrict__ logconf) {
  const int w = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
  const long long slot = (long long)b * Wmax + w;
  const float qnan = __int_as_float(0x7fc00000);
  // every test below is uniform across the wave; nothing is read through a value before it is checked
  const int nu = n_units[b], U = lens[b], Tb = min(in_lens[b], T);
  bool ok = nu >= 0 && nu <= Wmax && w < nu && U >= 0 && 2 * U + 1 <= Smax && Tb > 0;
  int lo = 0, hi = 0, ts = 0, te = 0;
  if (ok) {
    lo = unit_lo[slot]; hi = unit_hi[slot]; ts = win_start[slot]; te = win_end[slot];
    ok = lo >= 0 && lo < hi && hi <= U && hi - lo <= CONF_MAX_UNIT && ts >= 0 && ts < te && te <= Tb;
  }
  const int* lab = hyps;
  if (ok) {
    lab = hyps + off64[b];
    for (int u0 = 0; u0 < U; u0 += 64) {                      // a label outside [1, C - 1]: the lattices were never written
      const int u = u0 + j;
      const bool bad = u < U && (lab[u] < 1 || lab[u] >= C);
      if (__ballot(bad) != 0) ok = false;
    }
  }
  // the context is impossible: no frames before the window spell a non-empty y[:lo], none after it a non-empty y[hi:]
  if (ok && ((ts == 0 && lo != 0) || (te == Tb && hi != U))) ok = false;
  if (!ok) {
    if (j == 0) logconf[slot] = qnan;
    return;
  }
  const float* alpha = ab + ((long long)b * T) * Smax;
  const float* beta = ab + (((long long)Bn + b) * T) * Smax;
  const int n = hi - lo;                                      // lanes 0 .. n hold state pairs
  const bool act = j <= n, top = j == n, hasX = hi < U;
  const int uO = lo + j - 1;                                  // the label of this lane's odd state
  const bool actO = act && uO >= 0;
  const int clsO = actO ? lab[uO] : 0, clsX = hasX ? lab[hi] : 0;
  const bool skip = actO && uO + 1 < U && clsO != lab[uO + 1];   // state 2 uO + 1 may move on to 2 uO + 3
  float E = NEG_INF, O = NEG_INF, X = NEG_INF, Bq;
  int t;                                                      // the first frame the sweep computes
  if (te < Tb) {                                              // beta[te] with every state but 2hi and 2hi + 1 at -inf
    const float* br = beta + (long long)te * Smax;
    const float bE = br[2 * hi], bX = hasX ? br[2 * hi + 1] : NEG_INF;
    if (top) E = bE;
    X = bX;
    Bq = lse2(bE, bX);
    t = te - 1;
  } else {                                                    // te = T_b (hi = U): beta[T_b - 1] itself
    const float* br = beta + (long long)(Tb - 1) * Smax;
    if (act) E = br[2 * (lo + j)];
    if (actO) O = br[2 * (lo + j) - 1];
    Bq = 0.f;
    t = Tb - 2;
  }
  // emissions CONF_PF frames ahead, frame index clamped into the window: always a valid row with t < T_b
  auto fetch = [&](int tt, float& eO, float& eE, float& eX) {
    const int ti = tt > ts ? tt : ts;
    const float* lg = logits + ((long long)ti * Bn + b) * ld;
    const float ls = lse[(long long)ti * Bn + b];
    eE = lg[0] - ls;
    eO = lg[clsO] - ls;
    eX = lg[clsX] - ls;
  };
  float rO[CONF_PF], rE[CONF_PF], rX[CONF_PF];
#pragma unroll
  for (int k = 0; k < CONF_PF; ++k) fetch(t - k, rO[k], rE[k], rX[k]);
  for (; t >= ts; --t) {
    const float lpO = actO ? rO[0] : NEG_INF, lpE = act ? rE[0] : NEG_INF, lpX = hasX ? rX[0] : NEG_INF;
#pragma unroll
    for (int k = 0; k + 1 < CONF_PF; ++k) { rO[k] = rO[k + 1]; rE[k] = rE[k + 1]; rX[k] = rX[k + 1]; }
    fetch(t - CONF_PF, rO[CONF_PF - 1], rE[CONF_PF - 1], rX[CONF_PF - 1]);
    float Op = wave_shift1<0x130>(O);                         // state 2(lo + j) + 1
    Op = top ? X : Op;
    const float mO = lse3_sel(O, E, skip ? Op : NEG_INF);
    const float mE = lse2_sel(E, Op);
    O = (mO == NEG_INF) ? NEG_INF : mO + lpO;
    E = (mE == NEG_INF) ? NEG_INF : mE + lpE;
    X = X + lpX;
  }
  float Op = wave_shift1<0x130>(O);
  Op = top ? X : Op;
  if (j == 0) {                                               // O, E, Op = beta'[ts] of the states 2lo - 1, 2lo, 2lo + 1
    float num, A;
    if (ts == 0) {                                            // lo = 0
      num = lse2(E, Op);
      A = 0.f;
    } else {
      const float* ar = alpha + (long long)(ts - 1) * Smax;
      const float aM = lo >= 1 ? ar[2 * lo - 1] : NEG_INF, aE = ar[2 * lo];
      const float tM = aM + lse3(O, E, skip ? Op : NEG_INF);
      const float tE = aE + lse2(E, Op);
      num = lse2(tM, tE);
      A = lse2(aM, aE);
    }
    float r;
    if (A == NEG_INF || Bq == NEG_INF) r = qnan;
    else if (num == NEG_INF) r = NEG_INF;
    else r = fminf(0.f, num - (A + Bq));
    logconf[slot] = r;
  }
}

struct ConfLayout {
  size_t lse, ab, total;
  int Smax;
};
ConfLayout conf_layout(int T, int B, int max_hyp_len) {
  ConfLayout m;
  m.Smax = 2 * max_hyp_len + 1;
  m.lse = 0;
  m.ab = align_up((size_t)T * B * sizeof(float), 256);
  m.total = m.ab + align_up(2 * (size_t)B * T * (size_t)m.Smax * sizeof(float), 256);
  return m;
}

}  // namespace

extern "C" int ds2_ctc_conf_max_unit_labels(void) { return CONF_MAX_UNIT; }

extern "C" size_t ds2_ctc_conf_workspace_bytes(int T, int B, int max_hyp_len) {
  if (T <= 0 || B <= 0 || max_hyp_len < 0) return 0;
  return conf_layout(T, B, max_hyp_len).total;
}

extern "C" int ds2_ctc_conf_f32(const float* logits, int ld, int T, int B, int C, const int* hyps_dev, const long long* hyp_off_dev,
                                const int* hyp_lens_dev, const int* in_lens_dev, int max_hyp_len, const int* n_units_dev,
                                const int* unit_lo_dev, const int* unit_hi_dev, const int* win_start_dev, const int* win_end_dev, int W_max,
                                float* nll_dev, float* logconf_dev, int lattice, void* ws, size_t ws_bytes, void* stream) {
  // every size and pointer is checked before the first launch
  DS2_REQUIRE(logits && hyps_dev && hyp_off_dev && hyp_lens_dev && in_lens_dev && n_units_dev && unit_lo_dev && unit_hi_dev && win_start_dev &&
                  win_end_dev && nll_dev && logconf_dev,
              "ds2_ctc_conf_f32: null pointer");
  DS2_REQUIRE(T > 0 && B > 0 && C > 1, "ds2_ctc_conf_f32: bad dims (T=%d B=%d C=%d)", T, B, C);
  DS2_REQUIRE(W_max >= 1, "ds2_ctc_conf_f32: W_max must be >= 1, got %d", W_max);
  DS2_REQUIRE(B <= 65535 && (long long)T * B <= INT_MAX && (long long)B * W_max <= INT_MAX,
              "ds2_ctc_conf_f32: B, T * B or B * W_max too large (T=%d B=%d W_max=%d)", T, B, W_max);
  DS2_REQUIRE(max_hyp_len >= 0 && max_hyp_len <= (INT_MAX - 1) / 2, "ds2_ctc_conf_f32: max_hyp_len must be >= 0, got %d", max_hyp_len);
  DS2_REQUIRE(ld >= C, "ds2_ctc_conf_f32: row pitch below C (ld=%d C=%d)", ld, C);
  DS2_REQUIRE(lattice == 0 || lattice == 1, "ds2_ctc_conf_f32: lattice must be 0 or 1");
  const ConfLayout m = conf_layout(T, B, max_hyp_len);
  const int Smax = m.Smax;
  const size_t lds = (size_t)2 * Smax * sizeof(float);
  const bool wave = lattice == 0 && Smax <= 128;
  DS2_REQUIRE(wave || lds <= 64 * 1024, "ds2_ctc_conf_f32: hypotheses too long for LDS lattice rows (Smax=%d)", Smax);
  DS2_REQUIRE(ws && ws_bytes >= m.total, "ds2_ctc_conf_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* lse = (float*)((char*)ws + m.lse);
  float* ab = (float*)((char*)ws + m.ab);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3(ceil_div(T * B, 4)), dim3(256), 0, s, logits, ld, T, B, C, in_lens_dev, lse);
  DS2_LAUNCH_CHECK("ctc_lse_kernel");
  if (wave) {
    hipLaunchKernelGGL((ctc_lattice_wave_kernel<false, true>), dim3(B, 2), dim3(64), 0, s, logits, ld, T, B, C, hyps_dev, (const int*)nullptr,
                       in_lens_dev, hyp_lens_dev, (const float*)lse, ab, Smax, nll_dev, 0.f, (const int*)nullptr, 1, hyp_off_dev,
                       (const int*)nullptr);
    DS2_LAUNCH_CHECK("ctc_lattice_wave_kernel (conf)");
  } else {
    int threads = ceil_div(Smax, 64) * 64;
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL((ctc_lattice_kernel<false, true>), dim3(B, 2), dim3(threads), lds, s, logits, ld, T, B, C, hyps_dev, (const int*)nullptr,
                       in_lens_dev, hyp_lens_dev, (const float*)lse, ab, Smax, nll_dev, 0.f, (const int*)nullptr, 1, hyp_off_dev,
                       (const int*)nullptr);
    DS2_LAUNCH_CHECK("ctc_lattice_kernel (conf)");
  }
  hipLaunchKernelGGL(ctc_conf_kernel, dim3(W_max, B), dim3(64), 0, s, logits, ld, T, B, C, hyps_dev, hyp_off_dev, hyp_lens_dev, in_lens_dev,
                     (const float*)lse, (const float*)ab, Smax, n_units_dev, unit_lo_dev, unit_hi_dev, win_start_dev, win_end_dev, W_max,
                     logconf_dev);
  DS2_LAUNCH_CHECK("ctc_conf_kernel");
  return 0;
}
