// Fused log-softmax + CTC loss + gradient (fp32, log space), blank = 0, reduction = per-utterance nll.
// Replaces `out.float().log_softmax(2)` + `torch.nn.CTCLoss(reduction="sum")` forward AND their
// autograd backward (deepspeech_trainer.py:108-112, trainers/__main__.py:53).
//
//   input  logits (T,B,C) row pitch ld      (need not be normalised: the row log-sum-exp is computed
//                                            here; feeding log-probs gives lse = 0 -> same result)
//   output nll[b] = -log p(target_b | logits[:T_b, b])           (+inf if no valid alignment)
//          grad[t,b,c] = scale * (softmax(logits)[t,b,c] - occupancy[t,b,c]) for t < T_b, else 0
//          (= d(sum_b nll_b)/d logits * scale; rows of an infeasible utterance get 0)
//
// Kernels: (1) one wavefront per (t,b) row: max/sum shuffles -> lse.  (2) the lattices: 2U+1 <= 128 for the
// whole batch: one WAVEFRONT per (utterance, direction), the row in registers (ctc_lattice_wave_kernel);
// longer targets: one workgroup per (utterance, direction), the row in LDS, one barrier per frame, emission
// gathers prefetched 4 frames ahead (ctc_lattice_kernel).  (3) occupancy + gradient, deterministic (no float atomics):
// repeated labels are summed by the thread owning the first occurrence walking a next-same chain.
#include "common.h"
#include <math.h>

namespace {

constexpr float NEG_INF = -INFINITY;

// log-sum-exp of the lattice recurrences on the hardware exp2 / log2 (v_exp_f32, v_log_f32: 1 ulp each): every argument is <= 0 and
// the sum lies in [1, 3], so the only extra error over libm's expf / logf is the fp32 scaling of the argument (|x| 2^-24 in the
// exponent: < 5e-6 relative, and only on terms that are themselves < e^-80 of the sum).  The lattice is ONE dependent lse3 per frame per
// lane: with libm's range-reduced expf / logf (~25 instructions each) a frame cost 0.56 us, with these 0.45 us (c3: 278 -> 227 us per step;
// the rest is the LDS round trip + barrier + the dependent exp2 / log2 chain).  A first one-wave-per-lattice form (K states per lane) lost
// to it; the one below (ctc_lattice_wave_kernel: two states per lane, branch-free lse, vector-load ring) takes 0.19 us per frame.
__device__ __forceinline__ float fast_exp_(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float fast_log_(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994530942f; }
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + fast_log_(fast_exp_(a - m) + fast_exp_(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == NEG_INF) return NEG_INF;
  return m + fast_log_(fast_exp_(a - m) + fast_exp_(b - m) + fast_exp_(c - m));
}

// one wave per row
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ logits, int ld, int T, int Bn, int C,
                                                      const int* __restrict__ in_lens, float* __restrict__ lse) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T * Bn) return;
  const int t = row / Bn, b = row % Bn;
  if (t >= in_lens[b]) return;
  const int lane = threadIdx.x & 63;
  const float* p = logits + (long long)row * ld;
  float m = NEG_INF;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, p[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(p[c] - m);
  s = wave_sum(s);
  if (lane == 0) lse[row] = m + logf(s);
}

// The STAR = true instances of the three kernels below are the wildcard loss (ds2_ctc_star_loss_f32, contract in include/ds2hip.h): a
// label equal to C is the wildcard, whose state emits the constant star_pen instead of a log-softmax value; flags[b] bit 0 lets a path
// start in states 2 and 3 as well, bit 1 lets it end in states S-3 and S-4 as well.  The class used for an ADDRESS is clamped to the blank
// for a wildcard (one past the row otherwise) and the constant is selected into the loaded emission, off the dependent chain.  A label
// outside [1, C] is found before anything is read with it.  STAR = false: none of it is compiled, the kernels are the ones they were.
// -log of the summed end states: S-1, S-2 and, with flag bit 1, S-3, S-4 (a state that does not exist is passed as NEG_INF)
__device__ __forceinline__ float star_end_nll(float l1, float l2, float l3, float l4) { return -lse2(lse2(l1, l2), lse2(l3, l4)); }
__device__ __forceinline__ float star_cell(float a0, float a1, float a2, float lp, bool star);   // (below, next to lse3_sel)

// MW = true instances of the two lattice kernels are the n-best lattices of ds2_ctc_mwer_f32 (ctc_mwer.h, contract in include/ds2hip.h):
// blockIdx.x is the lattice n of B * K, which reads the logits, lse and in_lens of utterance n / K; labels, lengths, nll and the ab rows
// are indexed by n, the label offsets are 64-bit (off64; tgt_off is unused), and a slot that is not valid (valid, NULL = all valid),
// whose length lies outside [0, (Smax - 1) / 2] or whose labels leave [1, C - 1] gets nll = +inf before anything is read through it.
// MW = false: none of it is compiled, n = b and the kernels are the ones they were.
// blockIdx.x = utterance, blockIdx.y = 0: alpha (forward in t), 1: beta (backward in t).
// ab layout: [2][B][T][Smax]  (MW: [2][B * K][T][Smax])
template <bool STAR, bool MW = false>
__global__ __launch_bounds__(1024) void ctc_lattice_kernel(const float* __restrict__ logits, int ld, int T, int Bn, int C,
                                                           const int* __restrict__ targets, const int* __restrict__ tgt_off,
                                                           const int* __restrict__ in_lens, const int* __restrict__ tgt_lens,
                                                           const float* __restrict__ lse, float* __restrict__ ab, int Smax,
                                                           float* __restrict__ nll, float star_pen, const int* __restrict__ flags,
                                                           int K, const long long* __restrict__ off64, const int* __restrict__ valid) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [2][S] rows
  const int n = blockIdx.x, dirn = blockIdx.y;                  // n: the lattice, b: the utterance whose frames it reads
  const int b = MW ? n / K : n;
  const int Tb = min(in_lens[b], T), U = tgt_lens[n];
  const int S = 2 * U + 1;
  float* out = ab + (((long long)dirn * (MW ? Bn * K : Bn) + n) * T) * Smax;
  if constexpr (MW) {
    if ((valid && !valid[n]) || U < 0 || S > Smax) {            // uniform
      if (dirn == 0 && threadIdx.x == 0) nll[n] = INFINITY;
      return;
    }
  }
  if (Tb <= 0) {
    if (dirn == 0 && threadIdx.x == 0) nll[n] = (U == 0) ? 0.f : INFINITY;
    return;
  }
  const int* lab = MW ? targets + off64[n] : targets + tgt_off[n];
  float* row0 = smem;
  float* row1 = smem + Smax;
  const int nthr = blockDim.x;
  int nfree0 = 2, nfree1 = 2;                                 // STAR: how many states a path may start in / end in
  if constexpr (STAR) {
    int bad = 0;
    for (int u = threadIdx.x; u < U; u += nthr) bad |= (lab[u] < 1 || lab[u] > C);
    if (__syncthreads_or(bad)) {                              // uniform: the utterance is infeasible, its lattice stays unwritten
      if (dirn == 0 && threadIdx.x == 0) nll[n] = INFINITY;
      return;
    }
    const int f = flags ? flags[b] : 0;
    nfree0 = (f & 1) ? 4 : 2;
    nfree1 = (f & 2) ? 4 : 2;
  }
  if constexpr (MW) {
    int bad = 0;
    for (int u = threadIdx.x; u < U; u += nthr) bad |= (lab[u] < 1 || lab[u] >= C);
    if (__syncthreads_or(bad)) {                              // uniform
      if (dirn == 0 && threadIdx.x == 0) nll[n] = INFINITY;
      return;
    }
  }
  // this thread owns states s = tid, tid + nthr, ... (normally exactly one)
  // generic loop for very long targets; the common case S <= blockDim.x runs one iteration.
  const int step = dirn == 0 ? 1 : -1;
  const int tfirst = dirn == 0 ? 0 : Tb - 1;

  // init row
  for (int s = threadIdx.x; s < S; s += nthr) {
    int cls = (s & 1) ? lab[s >> 1] : 0;
    bool star = false;
    if constexpr (STAR) { star = cls == C; cls = star ? 0 : cls; }
    float lp = logits[((long long)tfirst * Bn + b) * ld + cls] - lse[tfirst * Bn + b];
    if constexpr (STAR) lp = star ? star_pen : lp;
    float v = NEG_INF;
    if constexpr (STAR) {
      if (dirn == 0) { if (s < nfree0) v = lp; }
      else { if (s >= S - nfree1) v = lp; }
    } else {
      if (dirn == 0) { if (s == 0 || s == 1) v = lp; }
      else { if (s == S - 1 || s == S - 2) v = lp; }
    }
    row0[s] = v;
    out[(long long)tfirst * Smax + s] = v;
  }
  __syncthreads();
  float* prev = row0;
  float* cur = row1;
  if (S <= nthr) {
    // Hot loop, written for instruction count (one dependent lattice row per frame: every instruction here is on the critical path).
    // Per-thread pointers advance by constant strides; emissions are loaded unconditionally 4 frames ahead from CLAMPED frame indices
    // (no exec-mask branches, no per-frame index arithmetic); only the stores are predicated.
    const int s = threadIdx.x;
    const bool act = s < S;
    int cls = 0;
    bool skip = false;
    if (act) {
      cls = (s & 1) ? lab[s >> 1] : 0;
      if (dirn == 0) skip = (s >= 2) && (s & 1) && (lab[s >> 1] != lab[(s >> 1) - 1]);
      else skip = (s + 2 < S) && (s & 1) && (lab[s >> 1] != lab[(s >> 1) + 1]);
    }
    bool star = false;
    if constexpr (STAR) { star = cls == C; cls = star ? 0 : cls; }
    const long long lg_stride = (long long)step * Bn * ld;
    const int ls_stride = step * Bn, out_stride = step * Smax;
    const float* lgp = logits + ((long long)tfirst * Bn + b) * ld + cls;        // frame tfirst, this state's class
    const float* lsp = lse + (long long)tfirst * Bn + b;
    float* op = out + (long long)tfirst * Smax + (act ? s : 0);
    const int s1 = dirn == 0 ? (s >= 1 ? s - 1 : 0) : (s + 1 < S ? s + 1 : 0);    // neighbour indices, clamped into the row
    const int s2 = dirn == 0 ? (s >= 2 ? s - 2 : 0) : (s + 2 < S ? s + 2 : 0);
    const bool has1 = dirn == 0 ? (s >= 1) : (s + 1 < S);
    const int last = Tb - 1;
    auto emission = [&](int i) {                                                  // frame index clamped: always a valid address
      const int ii = i < last ? i : last;
      const float e = lgp[(long long)ii * lg_stride] - lsp[(long long)ii * ls_stride];
      if constexpr (STAR) return star ? star_pen : e;           // selected 4 frames ahead of its use
      return e;
    };
    float nx0 = emission(1), nx1 = emission(2), nx2 = emission(3), nx3 = emission(4);
    const int sa = act ? s : 0;
    for (int i = 1; i < Tb; ++i) {
      const float lp = nx0;
      nx0 = nx1; nx1 = nx2; nx2 = nx3;
      nx3 = emission(i + 4);
      op += out_stride;
      const float a0 = prev[sa];
      const float a1 = has1 ? prev[s1] : NEG_INF;
      const float a2 = skip ? prev[s2] : NEG_INF;
      float v;
      if constexpr (STAR) {
        v = star_cell(a0, a1, a2, lp, star);
      } else {
        const float m = lse3(a0, a1, a2);
        v = (m == NEG_INF) ? NEG_INF : m + lp;
      }
      if (act) {
        cur[s] = v;
        *op = v;
      }
      __syncthreads();
      float* tmp = prev; prev = cur; cur = tmp;
    }
  } else {
    for (int i = 1; i < Tb; ++i) {
      const int t = tfirst + step * i;
      for (int s = threadIdx.x; s < S; s += nthr) {
        int cls = (s & 1) ? lab[s >> 1] : 0;
        bool star = false;
        if constexpr (STAR) { star = cls == C; cls = star ? 0 : cls; }
        float lp = logits[((long long)t * Bn + b) * ld + cls] - lse[t * Bn + b];
        if constexpr (STAR) lp = star ? star_pen : lp;
        float a0 = prev[s], a1, a2;
        if (dirn == 0) {
          const bool skip = (s >= 2) && (s & 1) && (lab[s >> 1] != lab[(s >> 1) - 1]);
          a1 = (s >= 1) ? prev[s - 1] : NEG_INF;
          a2 = skip ? prev[s - 2] : NEG_INF;
        } else {
          const bool skip = (s + 2 < S) && (s & 1) && (lab[s >> 1] != lab[(s >> 1) + 1]);
          a1 = (s + 1 < S) ? prev[s + 1] : NEG_INF;
          a2 = skip ? prev[s + 2] : NEG_INF;
        }
        float v;
        if constexpr (STAR) {
          v = star_cell(a0, a1, a2, lp, star);
        } else {
          const float m = lse3(a0, a1, a2);
          v = (m == NEG_INF) ? NEG_INF : m + lp;
        }
        cur[s] = v;
        out[(long long)t * Smax + s] = v;
      }
      __syncthreads();
      float* tmp = prev; prev = cur; cur = tmp;
    }
  }
  if (dirn == 0 && threadIdx.x == 0) {
    const float l1 = prev[S - 1];
    const float l2 = (S >= 2) ? prev[S - 2] : NEG_INF;
    if (STAR && nfree1 == 4) nll[n] = star_end_nll(l1, l2, (S >= 3) ? prev[S - 3] : NEG_INF, (S >= 4) ? prev[S - 4] : NEG_INF);
    else nll[n] = -lse2(l1, l2);
  }
}

// The same lattice for S <= 128 as ONE wavefront per (utterance, direction): lane l owns the adjacent states 2l (blank) and 2l + 1
// (label l), the row stays in registers, and the only cross-lane traffic per frame is a one-lane wave shift (DPP, no LDS, no barrier):
// forward in t the odd state of lane l - 1 (s - 1 of the even state, s - 2 of the odd one; the odd state's s - 1 is its own lane's even
// state), backward in t both states of lane l + 1.  The two lse3 chains of a lane are independent within a frame and overlap.  Emissions
// are loaded WPF frames ahead from clamped frame indices into a register ring; the ab stores hang off the chain.  Every value is
// computed by the expressions of ctc_lattice_kernel in the same operand order (a0, a1, a2), so ab / nll are the same bits: an even
// state's a2 is always NEG_INF there, whose term is exp2(-inf) = +0 added last — leaving it out changes nothing.  States >= S are held
// at NEG_INF (backward in t, state S - 1 reads state S).
constexpr int WPF = 8;
typedef float f32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
template <int CTRL>
__device__ __forceinline__ float wave_shift1(float v) {      // CTRL 0x138: lane l <- lane l - 1 ; 0x130: lane l <- lane l + 1 ; the end lane gets NEG_INF
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(NEG_INF), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// lse3 / lse3(a, b, NEG_INF) as selects instead of an early return: the same value (the discarded arm may be NaN), and a frame's two
// chains stay in one basic block where they interleave
__device__ __forceinline__ float lse3_sel(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float r = m + fast_log_(fast_exp_(a - m) + fast_exp_(b - m) + fast_exp_(c - m));
  return (m == NEG_INF) ? NEG_INF : r;
}
__device__ __forceinline__ float lse2_sel(float a, float b) {
  const float m = fmaxf(a, fmaxf(b, NEG_INF));
  const float r = m + fast_log_(fast_exp_(a - m) + fast_exp_(b - m));
  return (m == NEG_INF) ? NEG_INF : r;
}

// One lattice cell of the STAR instances: lse3 of the predecessors + the emission.  For every state but a wildcard these are the
// expressions of lse3 / lse3_sel and of the add that follows them, in their operand order: (m + log(sum)) + lp.  A wildcard's emission is
// the SAME constant in every frame: added to the finished lse, a value of the magnitude of alpha (hundreds), it is rounded to that
// value's grid in the same direction every frame, and the error does not average out but drifts (T = 420, U = 200: 1.5e-3 in nll, 1.2e-3
// relative in the gradient, five times the plain loss's error).  So a wildcard adds its constant to log(sum) first, m + (log(sum) + lp):
// the one rounding at alpha's magnitude then sees a value that differs from frame to frame, as for every other state.
__device__ __forceinline__ float star_cell(float a0, float a1, float a2, float lp, bool star) {
  const float m = fmaxf(a0, fmaxf(a1, a2));
  const float lg = fast_log_(fast_exp_(a0 - m) + fast_exp_(a1 - m) + fast_exp_(a2 - m));
  const float x = (star ? lp : m) + lg;
  const float y = star ? m : lp;
  return (m == NEG_INF) ? NEG_INF : x + y;
}

template <int DIRN, bool STAR>
__device__ __forceinline__ void ctc_lattice_wave_body(const float* __restrict__ logits, int ld, int T, int Bn, int C,
                                                      const int* __restrict__ lab, int b, int n, int Tb, int U, const float* __restrict__ lse,
                                                      float* __restrict__ out, int Smax, float* __restrict__ nll, float star_pen, int flag) {
  // b: the utterance (logits, lse); n: the lattice (nll[n]; n = b but for the MW instances); out: this lattice's rows
  const int S = 2 * U + 1;
  const int l = threadIdx.x;
  const bool actE = 2 * l < S, actO = 2 * l + 1 < S;
  const int step = DIRN == 0 ? 1 : -1;
  const int tfirst = DIRN == 0 ? 0 : Tb - 1;
  int cls = 0;
  bool skip = false;
  if (actO) {
    cls = lab[l];
    if (DIRN == 0) skip = (l >= 1) && (cls != lab[l - 1]);
    else skip = (l + 1 < U) && (cls != lab[l + 1]);
  }
  // STAR: a wildcard lane loads the blank's logit (a valid address) and never uses it: `frame` takes the odd state's emission through ONE
  // select as before, whose arms become (loaded emission | lane constant) with the constant star_pen for a wildcard and NEG_INF for a
  // state >= S, so a frame has the instructions it had
  bool ldO = actO, starO = false;
  float cstO = NEG_INF;
  if constexpr (STAR) {
    const bool star = actO && cls == C;
    starO = star;
    cls = star ? 0 : cls;
    ldO = actO && !star;
    cstO = star ? star_pen : NEG_INF;
  }
  const long long lg_stride = (long long)step * Bn * ld;
  const int ls_stride = step * Bn, out_stride = step * Smax;
  // the frame's three loads (this lane's label logit, the blank's logit, the row's lse) are all VECTOR loads — the last two through a
  // lane offset the compiler cannot see is zero: scalar loads return out of order, so waiting for the oldest of a ring of them waits for
  // all, and the ring would hide one frame of latency instead of WPF
  int vz;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
  const float* lgb = logits + ((long long)tfirst * Bn + b) * ld + vz;         // frame tfirst: the blank's logit; + cls: this lane's label
  const float* lsp = lse + (long long)tfirst * Bn + b + vz;
  float* op = out + (long long)tfirst * Smax + (actE ? 2 * l : 0);
  const int last = Tb - 1;
  auto fetch = [&](int i, float& lgE, float& lgO, float& ls) {                 // frame index clamped: always a valid address
    const int ii = i < last ? i : last;
    ls = lsp[(long long)ii * ls_stride];
    lgE = lgb[(long long)ii * lg_stride];
    lgO = lgb[(long long)ii * lg_stride + cls];
  };
  float E = NEG_INF, O = NEG_INF;
  // the lane's two states leave as ONE 8-byte store (rows of `ab` are only 4-byte aligned: Smax is odd), so that a store instruction
  // covers a contiguous run of the row; written one state per instruction — every other dword — the lattice's 26 MB of half-filled
  // 32-byte sectors were still draining when ctc_grad_kernel read them back (54 -> 183 us)
  auto store_pair = [&]() {
    if (actO) *reinterpret_cast<f32x2_a4*>(op) = f32x2_a4{E, O};
    else if (actE) op[0] = E;
  };
  // init row
  {
    float lgE, lgO, ls;
    fetch(0, lgE, lgO, ls);
    const float eE = lgE - ls;
    float eO = lgO - ls;
    if constexpr (STAR) {
      eO = ldO ? eO : cstO;
      const int n0 = (flag & 1) ? 4 : 2, n1 = (flag & 2) ? 4 : 2;
      if (DIRN == 0) { if (actE && 2 * l < n0) E = eE; if (actO && 2 * l + 1 < n0) O = eO; }
      else { if (actE && 2 * l >= S - n1) E = eE; if (actO && 2 * l + 1 >= S - n1) O = eO; }
    } else {
      if (DIRN == 0) { if (l == 0) { E = eE; if (actO) O = eO; } }
      else { if (2 * l == S - 1) E = eE; if (actO && 2 * l + 1 == S - 2) O = eO; }
    }
    store_pair();
  }
  // one frame: a state >= S gets the emission NEG_INF, which holds it at NEG_INF without a select on the chain
  auto frame = [&](float lgE, float lgO, float ls) {
    const float lpE = actE ? lgE - ls : NEG_INF, lpO = STAR ? (ldO ? lgO - ls : cstO) : (actO ? lgO - ls : NEG_INF);
    op += out_stride;
    float mE, mO = NEG_INF, nO = NEG_INF;                                         // (nO: the odd state's new value, STAR)
    if (DIRN == 0) {
      const float Om = wave_shift1<0x138>(O);                                   // state 2l - 1
      mE = lse2_sel(E, Om);
      if constexpr (STAR) nO = star_cell(O, E, skip ? Om : NEG_INF, lpO, starO);
      else mO = lse3_sel(O, E, skip ? Om : NEG_INF);
    } else {
      const float Ep = wave_shift1<0x130>(E), Op = wave_shift1<0x130>(O);       // states 2l + 2, 2l + 3
      mE = lse2_sel(E, O);
      if constexpr (STAR) nO = star_cell(O, Ep, skip ? Op : NEG_INF, lpO, starO);
      else mO = lse3_sel(O, Ep, skip ? Op : NEG_INF);
    }
    E = (mE == NEG_INF) ? NEG_INF : mE + lpE;
    if constexpr (STAR) O = nO;
    else O = (mO == NEG_INF) ? NEG_INF : mO + lpO;
    store_pair();
  };
  float rE[WPF], rO[WPF], rL[WPF];
#pragma unroll
  for (int k = 0; k < WPF; ++k) fetch(1 + k, rE[k], rO[k], rL[k]);
  int i0 = 1;
  for (; i0 + WPF <= Tb; i0 += WPF) {                                           // whole groups: slot k holds frame i0 + k, refilled with i0 + k + WPF
#pragma unroll
    for (int k = 0; k < WPF; ++k) {
      const float lgE = rE[k], lgO = rO[k], ls = rL[k];
      fetch(i0 + k + WPF, rE[k], rO[k], rL[k]);
      frame(lgE, lgO, ls);
    }
  }
#pragma unroll
  for (int k = 0; k < WPF - 1; ++k)                                             // the last Tb - i0 < WPF frames are in the ring already
    if (i0 + k < Tb) frame(rE[k], rO[k], rL[k]);
  if (DIRN == 0) {
    const float l1 = __shfl(E, U, 64);                                          // state S - 1 = 2U
    const float l2 = __shfl(O, U >= 1 ? U - 1 : 0, 64);                         // state S - 2
    if constexpr (STAR) {
      const float l3 = __shfl(E, U >= 1 ? U - 1 : 0, 64);                       // state S - 3
      const float l4 = __shfl(O, U >= 2 ? U - 2 : 0, 64);                       // state S - 4
      if (l == 0) {
        if (flag & 2) nll[n] = star_end_nll(l1, (S >= 2) ? l2 : NEG_INF, (S >= 3) ? l3 : NEG_INF, (S >= 4) ? l4 : NEG_INF);
        else nll[n] = -lse2(l1, (S >= 2) ? l2 : NEG_INF);
      }
    } else {
      if (l == 0) nll[n] = -lse2(l1, (S >= 2) ? l2 : NEG_INF);
    }
  }
}

// blockIdx.x = utterance, blockIdx.y = direction; 64 threads.  Needs 2 * tgt_lens[b] + 1 <= 128 for every b (the launcher checks Smax).
template <bool STAR, bool MW = false>
__global__ __launch_bounds__(64) void ctc_lattice_wave_kernel(const float* __restrict__ logits, int ld, int T, int Bn, int C,
                                                              const int* __restrict__ targets, const int* __restrict__ tgt_off,
                                                              const int* __restrict__ in_lens, const int* __restrict__ tgt_lens,
                                                              const float* __restrict__ lse, float* __restrict__ ab, int Smax,
                                                              float* __restrict__ nll, float star_pen, const int* __restrict__ flags,
                                                              int K, const long long* __restrict__ off64, const int* __restrict__ valid) {
  const int n = blockIdx.x, dirn = blockIdx.y;                // n: the lattice, b: the utterance whose frames it reads (see ctc_lattice_kernel)
  const int b = MW ? n / K : n;
  const int Tb = min(in_lens[b], T), U = tgt_lens[n];
  float* out = ab + (((long long)dirn * (MW ? Bn * K : Bn) + n) * T) * Smax;
  if constexpr (MW) {
    if ((valid && !valid[n]) || U < 0 || 2 * U + 1 > Smax) {  // uniform (Smax <= 128 here: U <= 63)
      if (dirn == 0 && threadIdx.x == 0) nll[n] = INFINITY;
      return;
    }
  }
  if (Tb <= 0) {
    if (dirn == 0 && threadIdx.x == 0) nll[n] = (U == 0) ? 0.f : INFINITY;
    return;
  }
  const int* lab = MW ? targets + off64[n] : targets + tgt_off[n];
  int flag = 0;
  if constexpr (STAR) {
    const int l = threadIdx.x;
    const bool bad = l < U && (lab[l] < 1 || lab[l] > C);     // one label per lane (U <= 63)
    if (__ballot(bad) != 0) {                                 // uniform: the utterance is infeasible, its lattice stays unwritten
      if (dirn == 0 && l == 0) nll[n] = INFINITY;
      return;
    }
    flag = flags ? flags[b] : 0;
  }
  if constexpr (MW) {
    const int l = threadIdx.x;
    const bool bad = l < U && (lab[l] < 1 || lab[l] >= C);    // one label per lane
    if (__ballot(bad) != 0) {                                 // uniform
      if (dirn == 0 && l == 0) nll[n] = INFINITY;
      return;
    }
  }
  if (dirn == 0) ctc_lattice_wave_body<0, STAR>(logits, ld, T, Bn, C, lab, b, n, Tb, U, lse, out, Smax, nll, star_pen, flag);
  else ctc_lattice_wave_body<1, STAR>(logits, ld, T, Bn, C, lab, b, n, Tb, U, lse, out, Smax, nll, star_pen, flag);
}

// grid = (ceil(T / TCH), B); block = 128 threads; dynamic LDS: q[C] + val[S] + nxt[U] (ints) + lab[U]
// STAR: q has the slot C for the wildcard's occupancy (its labels chain like any repeated label: one writer), the wildcard's emission is
// the constant, and the softmax term is multiplied by 1 - q[C]:  grad = scale * (softmax * (1 - occ_star) - occ)
constexpr int TCH = 8;
template <bool STAR>
__global__ __launch_bounds__(128) void ctc_grad_kernel(const float* __restrict__ logits, int ld, float* __restrict__ grad, int ldg, int T,
                                                       int Bn, int C, const int* __restrict__ targets,
                                                       const int* __restrict__ tgt_off, const int* __restrict__ in_lens,
                                                       const int* __restrict__ tgt_lens, const float* __restrict__ lse,
                                                       const float* __restrict__ ab, int Smax, const float* __restrict__ nll,
                                                       float scale, float star_pen) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float bred[2];
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * TCH;
  const int Tb = min(in_lens[b], T), U = tgt_lens[b];
  const int S = 2 * U + 1;
  const float nl = nll[b];
  const bool feasible = (nl != INFINITY) && (nl == nl);
  constexpr int QX = STAR ? 1 : 0;
  float* q = smem;                      // [C] (STAR: [C + 1])
  float* val = q + C + QX;              // [S]
  int* nxt = (int*)(val + Smax);        // [U]
  int* labs = nxt + (Smax / 2 + 1);     // [U]
  int* hd = labs + (Smax / 2 + 1);      // [U] 1 = first occurrence of its label (the thread that sums the chain)
  const int* lab = targets + tgt_off[b];
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int u = tid; u < U; u += nthr) labs[u] = lab[u];
  __syncthreads();
  // nxt[u] = next index with the same label, or -1 ; head flag encoded as nxt sign trick: store separately
  for (int u = tid; u < U; u += nthr) {
    const int l = labs[u];
    int n = -1;
    for (int v = u + 1; v < U; ++v)
      if (labs[v] == l) { n = v; break; }
    nxt[u] = n;
    int head = 1;                        // (was re-derived for every frame)
    for (int v = 0; v < u; ++v)
      if (labs[v] == l) { head = 0; break; }
    hd[u] = head;
  }
  __syncthreads();
  const float* alpha = ab + (((long long)0 * Bn + b) * T) * Smax;
  const float* beta = ab + (((long long)1 * Bn + b) * T) * Smax;
  for (int tt = 0; tt < TCH; ++tt) {
    const int t = t0 + tt;
    if (t >= T) break;
    float* g = grad + ((long long)t * Bn + b) * ldg;
    if (t >= Tb || !feasible) {
      for (int c = tid; c < C; c += nthr) g[c] = 0.f;
      continue;  // uniform across the block
    }
    const float* lg = logits + ((long long)t * Bn + b) * ld;
    const float ls = lse[t * Bn + b];
    for (int c = tid; c < C + QX; c += nthr) q[c] = 0.f;
    float bsum = 0.f;
    for (int s = tid; s < S; s += nthr) {
      int cls = (s & 1) ? labs[s >> 1] : 0;
      bool star = false;
      if constexpr (STAR) { star = cls == C; cls = star ? 0 : cls; }
      const float a = alpha[(long long)t * Smax + s] + beta[(long long)t * Smax + s];
      float e = lg[cls] - ls;
      if constexpr (STAR) e = star ? star_pen : e;
      float v = 0.f;
      if (a != NEG_INF) v = expf(a - e + nl);
      if (s & 1) val[s >> 1] = v;
      else bsum += v;
    }
    bsum = wave_sum(bsum);
    if ((tid & 63) == 0) bred[tid >> 6] = bsum;
    __syncthreads();
    // heads: u is a head if no earlier index has the same label
    for (int u = tid; u < U; u += nthr) {
      const int l = labs[u];
      if (hd[u]) {
        float sacc = 0.f;
        for (int v = u; v >= 0; v = nxt[v]) sacc += val[v];
        q[l] += sacc;  // single writer per class (l != 0 guaranteed for labels; blank handled below)
      }
    }
    if (tid == 0) q[0] += bred[0] + bred[1];
    __syncthreads();
    if constexpr (STAR) {
      const float keep = 1.f - q[C];
      for (int c = tid; c < C; c += nthr) g[c] = scale * (expf(lg[c] - ls) * keep - q[c]);
    } else {
      for (int c = tid; c < C; c += nthr) g[c] = scale * (expf(lg[c] - ls) - q[c]);
    }
    __syncthreads();
  }
}

// softmax over the last dim, one wave per row (InferenceBatchSoftmax, modules/blocks.py:59-64)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int rows,
                                                           int C) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* p = x + (long long)row * ldx;
  float* q = y + (long long)row * ldy;
  float m = NEG_INF;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, p[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(p[c] - m);
  s = wave_sum(s);
  const float inv = 1.f / s;
  for (int c = lane; c < C; c += 64) q[c] = expf(p[c] - m) * inv;
}

}  // namespace

extern "C" int ds2_softmax_rows_f32(const float* x, int ldx, float* y, int ldy, int rows, int C, void* stream) {
  DS2_REQUIRE(x && y && rows > 0 && C > 0, "ds2_softmax_rows_f32: bad args");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, rows, C);
  DS2_LAUNCH_CHECK("softmax_rows_kernel");
  return 0;
}

namespace {
// loss = sum_b nll[b] / B in a fixed order (lane-strided partial sums, then a shuffle tree): one wave
__global__ __launch_bounds__(64) void batch_mean_kernel(const float* __restrict__ nll, int B, float* __restrict__ out) {
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 64) s += nll[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) out[0] = s / (float)B;
}
}  // namespace

// out[0] = (sum of the per-utterance losses) / B: `loss = criterion(...) / inputs.size(0)` (trainers/deepspeech_trainer.py:110-112) on the device
extern "C" int ds2_ctc_batch_mean_f32(const float* nll_dev, int B, float* out_dev, void* stream) {
  DS2_REQUIRE(nll_dev && out_dev && B > 0, "ds2_ctc_batch_mean_f32: bad args");
  hipLaunchKernelGGL(batch_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, nll_dev, B, out_dev);
  DS2_LAUNCH_CHECK("batch_mean_kernel");
  return 0;
}

extern "C" size_t ds2_ctc_workspace_bytes(int T, int B, int max_target_len) {
  const size_t Smax = 2 * (size_t)max_target_len + 1;
  return align_up((size_t)T * B * sizeof(float), 256) + 2 * (size_t)B * T * Smax * sizeof(float);
}

namespace {
template <bool STAR>
int ctc_loss_launch(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev,
                    const int* tgt_lens_dev, int max_target_len, float star_pen, const int* flags_dev, float* nll_dev, float* grad, int ldg,
                    float grad_scale, int lattice, void* ws, hipStream_t s) {
  const int Smax = 2 * max_target_len + 1;
  float* lse = (float*)ws;
  float* ab = (float*)((char*)ws + align_up((size_t)T * B * sizeof(float), 256));
  // every size is checked before the first launch
  const size_t lds = (size_t)2 * Smax * sizeof(float);
  const bool wave = lattice == 0 && Smax <= 128;
  DS2_REQUIRE(wave || lds <= 64 * 1024, "ds2_ctc_loss_f32: target too long for LDS lattice rows (Smax=%d)", Smax);
  const size_t lds2 = ((size_t)C + (STAR ? 1 : 0) + Smax) * sizeof(float) + 3 * ((size_t)Smax / 2 + 1) * sizeof(int);
  DS2_REQUIRE(!grad || lds2 <= 64 * 1024, "ds2_ctc_loss_f32: C/S too large for LDS (C=%d Smax=%d)", C, Smax);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3(ceil_div(T * B, 4)), dim3(256), 0, s, logits, ld, T, B, C, in_lens_dev, lse);
  DS2_LAUNCH_CHECK("ctc_lse_kernel");
  if (wave) {
    hipLaunchKernelGGL(ctc_lattice_wave_kernel<STAR>, dim3(B, 2), dim3(64), 0, s, logits, ld, T, B, C, targets_dev, tgt_off_dev, in_lens_dev,
                       tgt_lens_dev, (const float*)lse, ab, Smax, nll_dev, star_pen, flags_dev, 1, (const long long*)nullptr,
                       (const int*)nullptr);
    DS2_LAUNCH_CHECK("ctc_lattice_wave_kernel");
  } else {
    int threads = ceil_div(Smax, 64) * 64;
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL(ctc_lattice_kernel<STAR>, dim3(B, 2), dim3(threads), lds, s, logits, ld, T, B, C, targets_dev, tgt_off_dev,
                       in_lens_dev, tgt_lens_dev, (const float*)lse, ab, Smax, nll_dev, star_pen, flags_dev, 1, (const long long*)nullptr,
                       (const int*)nullptr);
    DS2_LAUNCH_CHECK("ctc_lattice_kernel");
  }
  if (grad) {
    hipLaunchKernelGGL(ctc_grad_kernel<STAR>, dim3(ceil_div(T, TCH), B), dim3(128), lds2, s, logits, ld, grad, ldg, T, B, C, targets_dev,
                       tgt_off_dev, in_lens_dev, tgt_lens_dev, (const float*)lse, (const float*)ab, Smax, (const float*)nll_dev,
                       grad_scale, star_pen);
    DS2_LAUNCH_CHECK("ctc_grad_kernel");
  }
  return 0;
}
}  // namespace

// targets: flat labels (device int32), tgt_off[b] = start of utterance b in `targets` (device int32).
// lattice: 0 = the launcher chooses (one wave per lattice when 2 * max_target_len + 1 <= 128, else one workgroup per lattice),
//          1 = always one workgroup per lattice (ctc_lattice_kernel; the two produce the same bits: tests/test_gpu_ctc_wave.py)
extern "C" int ds2_ctc_loss_ex_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                                   const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float* nll_dev, float* grad, int ldg,
                                   float grad_scale, int lattice, void* ws, size_t ws_bytes, void* stream) {
  DS2_REQUIRE(logits && targets_dev && tgt_off_dev && in_lens_dev && tgt_lens_dev && nll_dev, "ds2_ctc_loss_f32: null pointer");
  DS2_REQUIRE(T > 0 && B > 0 && C > 0 && max_target_len >= 0, "ds2_ctc_loss_f32: bad dims");
  DS2_REQUIRE(lattice == 0 || lattice == 1, "ds2_ctc_loss_ex_f32: lattice must be 0 or 1");
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_workspace_bytes(T, B, max_target_len), "ds2_ctc_loss_f32: workspace too small");
  return ctc_loss_launch<false>(logits, ld, T, B, C, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_target_len, 0.f, nullptr, nll_dev,
                                grad, ldg, grad_scale, lattice, ws, (hipStream_t)stream);
}

// The wildcard loss (contract: include/ds2hip.h): the STAR = true instances of the same kernels, the same workspace.
extern "C" size_t ds2_ctc_star_workspace_bytes(int T, int B, int max_target_len) { return ds2_ctc_workspace_bytes(T, B, max_target_len); }

extern "C" int ds2_ctc_star_loss_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                                     const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float star_penalty,
                                     const int* flags_dev, float* nll_dev, float* grad, int ldg, float grad_scale, int lattice, void* ws,
                                     size_t ws_bytes, void* stream) {
  DS2_REQUIRE(logits && targets_dev && tgt_off_dev && in_lens_dev && tgt_lens_dev && nll_dev, "ds2_ctc_star_loss_f32: null pointer");
  DS2_REQUIRE(T > 0 && B > 0 && C > 0 && max_target_len >= 0, "ds2_ctc_star_loss_f32: bad dims");
  DS2_REQUIRE(lattice == 0 || lattice == 1, "ds2_ctc_star_loss_f32: lattice must be 0 or 1");
  DS2_REQUIRE(star_penalty <= 0.f && star_penalty >= -3.402823466e+38f, "ds2_ctc_star_loss_f32: star_penalty must be finite and <= 0, got %g",
              (double)star_penalty);                                                          // (NaN fails the first test)
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_star_workspace_bytes(T, B, max_target_len), "ds2_ctc_star_loss_f32: workspace too small");
  return ctc_loss_launch<true>(logits, ld, T, B, C, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_target_len, star_penalty,
                               flags_dev, nll_dev, grad, ldg, grad_scale, lattice, ws, (hipStream_t)stream);
}

extern "C" int ds2_ctc_loss_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                                const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float* nll_dev,
                                float* grad, int ldg, float grad_scale, void* ws, size_t ws_bytes, void* stream) {
  return ds2_ctc_loss_ex_f32(logits, ld, T, B, C, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_target_len, nll_dev, grad, ldg,
                             grad_scale, 0, ws, ws_bytes, stream);
}

// CTC forced alignment (ds2_ctc_align_*): the same lattice over (max, +) with back-pointers and a backtrace.  It lives in its own file
// and is compiled in this translation unit, next to the lattice helpers it shares (wave_shift1, WPF, NEG_INF).
#define DS2_CTC_ALIGN_TU
#include "ctc_align.h"
// ... and its tiled form for long recordings (ds2_ctc_align_tiled_*), which shares the cell, the emission and the back-pointer layout
#include "ctc_align_tiled.h"
// ... and the wildcard / free-ends entries (ds2_ctc_align_star_*), which instantiate both with STAR = true behind a pre-pass
#include "ctc_align_star.h"
// Keyword search (ds2_ctc_kws_*): the one-wavefront lattice entered at any frame, a start frame per state instead of back-pointers,
// behind the same pre-pass with penalty 0, and a pick of non-overlapping detections
#include "ctc_kws.h"
// ... and its streaming form (ds2_ctc_kws_stream_*): the same lattice kernel resumed from a state blob, and a pick that reports a
// detection as final once no later frame can change it
#include "ctc_kws_stream.h"
// Minimum-error-rate training on an n-best list (ds2_ctc_mwer_*): the MW = true instances of the two lattice kernels above, a weights
// launch and a gradient kernel that folds the K occupancies of an utterance into one row
#include "ctc_mwer.h"
// Word and character confidences (ds2_ctc_conf_*): the MW = true lattices at K = 1 and one short masked backward sweep per unit
#include "ctc_conf.h"
