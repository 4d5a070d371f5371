// Minimum-error-rate training on an n-best list (ds2_ctc_mwer_f32, contract in include/ds2hip.h): the expected risk of K hypotheses per
// utterance under their renormalised CTC posteriors, and its gradient with respect to the logits.  Compiled inside ctc.hip's
// translation unit: the B * K lattices are the MW = true instances of ctc_lattice_wave_kernel / ctc_lattice_kernel (lattice n reads
// utterance n / K), behind the plain entry's ctc_lse_kernel.  What is new here:
//   ctc_mwer_weights_kernel  one thread per utterance, K slots in slot order: p_k (max-subtracted softmax of -nll over the finite
//                            slots), loss_b = sum p_k R_k, w_k = p_k (R_k - loss_b)
//   ctc_mwer_chain_kernel    one workgroup per hypothesis with w_k != 0: the next-same-label chain and the head flags that
//                            ctc_grad_kernel derives per block (O(U^2)), once per hypothesis into the workspace
//   ctc_mwer_grad_kernel     ctc_grad_kernel's blocks over (frame chunk, utterance), looping k in slot order: w_k * occ_k summed into
//                            one LDS class row per frame of the chunk (repeated labels by their chain head: one writer), then ONE
//                            read-modify-write of the gradient rows.  sum_k w_k = 0 cancels the K softmax terms, so none is computed.
// Workspace: lse (T, B) | alpha / beta [2][B K][T][Smax] | chain [B K][2][Umax] | w [B K], Smax = 2 max_hyp_len + 1, Umax = max(max_hyp_len, 1).
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_mwer.h is a part of ctc.hip"
#endif
#include <limits.h>

namespace {

__device__ __forceinline__ bool mwer_finite(float v) { return fabsf(v) < INFINITY; }        // false for NaN

__global__ __launch_bounds__(64) void ctc_mwer_weights_kernel(const float* __restrict__ nll_hyp, const float* __restrict__ risk,
                                                              const int* __restrict__ in_lens, int Bn, int K, float* __restrict__ post,
                                                              float* __restrict__ loss, float* __restrict__ w) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= Bn) return;
  const float* nl = nll_hyp + (long long)b * K;
  const float* R = risk + (long long)b * K;
  float* p = post + (long long)b * K;
  float* wk = w + (long long)b * K;
  float m = INFINITY;
  for (int k = 0; k < K; ++k)
    if (mwer_finite(nl[k])) m = fminf(m, nl[k]);
  float Z = 0.f;
  for (int k = 0; k < K; ++k)
    if (mwer_finite(nl[k])) Z += expf(m - nl[k]);
  float L = 0.f;
  for (int k = 0; k < K; ++k) {
    const bool fin = mwer_finite(nl[k]);
    const float pk = fin ? expf(m - nl[k]) / Z : 0.f;
    p[k] = pk;
    if (fin) L += pk * R[k];
  }
  const bool live = in_lens[b] > 0;
  if (!live) L = 0.f;
  loss[b] = L;
  for (int k = 0; k < K; ++k) wk[k] = (live && mwer_finite(nl[k])) ? p[k] * (R[k] - L) : 0.f;
}

// chain layout per hypothesis: nxt[Umax] (next index with the same label, or -1) | head[Umax] (1 = first occurrence of its label)
__global__ __launch_bounds__(128) void ctc_mwer_chain_kernel(const int* __restrict__ hyps, const long long* __restrict__ off64,
                                                             const int* __restrict__ lens, const float* __restrict__ nll_hyp,
                                                             const float* __restrict__ w, int Umax, int* __restrict__ chain) {
  extern __shared__ __attribute__((aligned(16))) int mw_labs[];
  const int n = blockIdx.x;
  if (!mwer_finite(nll_hyp[n]) || w[n] == 0.f) return;       // uniform; a finite nll says the slot is valid, 0 <= U <= Umax, labels in range
  const int U = lens[n];
  const int* lab = hyps + off64[n];
  int* nxt = chain + (long long)n * 2 * Umax;
  int* hd = nxt + Umax;
  for (int u = threadIdx.x; u < U; u += blockDim.x) mw_labs[u] = lab[u];
  __syncthreads();
  for (int u = threadIdx.x; u < U; u += blockDim.x) {
    const int l = mw_labs[u];
    int nx = -1;
    for (int v = u + 1; v < U; ++v)
      if (mw_labs[v] == l) { nx = v; break; }
    int head = 1;
    for (int v = 0; v < u; ++v)
      if (mw_labs[v] == l) { head = 0; break; }
    nxt[u] = nx;
    hd[u] = head;
  }
}

// grid = (ceil(T / TCH), B); block = 128 threads; dynamic LDS: q[TCH][C] + val[Umax] + labs[Umax] + nxt[Umax] + hd[Umax]
__global__ __launch_bounds__(128) void ctc_mwer_grad_kernel(const float* __restrict__ logits, int ld, float* __restrict__ grad, int ldg, int T,
                                                            int Bn, int C, int K, const int* __restrict__ hyps,
                                                            const long long* __restrict__ off64, const int* __restrict__ lens,
                                                            const int* __restrict__ in_lens, const float* __restrict__ lse,
                                                            const float* __restrict__ ab, int Smax, const float* __restrict__ nll_hyp,
                                                            const float* __restrict__ w, const int* __restrict__ chain, int Umax, float scale,
                                                            int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float bred[2];
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * TCH;
  const int Tb = min(in_lens[b], T);
  const int nt = max(0, min(TCH, Tb - t0));                   // valid frames of this chunk
  float* q = smem;                                            // [TCH][C]
  float* val = q + TCH * C;                                   // [Umax]
  int* labs = (int*)(val + Umax);
  int* nxt = labs + Umax;
  int* hd = nxt + Umax;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long long N = (long long)Bn * K;
  if (nt > 0) {
    for (int i = tid; i < nt * C; i += nthr) q[i] = 0.f;
    __syncthreads();
    for (int k = 0; k < K; ++k) {
      const long long n = (long long)b * K + k;
      const float wk = w[n], nl = nll_hyp[n];
      if (wk == 0.f || !mwer_finite(nl)) continue;            // uniform across the block
      const int U = lens[n], S = 2 * U + 1;
      const int* lab = hyps + off64[n];
      const int* cn = chain + n * 2 * Umax;
      for (int u = tid; u < U; u += nthr) {
        labs[u] = lab[u];
        nxt[u] = cn[u];
        hd[u] = cn[Umax + u];
      }
      __syncthreads();
      const float* alpha = ab + (n * T) * Smax;
      const float* beta = ab + ((N + n) * T) * Smax;
      for (int tt = 0; tt < nt; ++tt) {
        const int t = t0 + tt;
        const float* lg = logits + ((long long)t * Bn + b) * ld;
        const float ls = lse[t * Bn + b];
        float bsum = 0.f;
        for (int s = tid; s < S; s += nthr) {
          const int cls = (s & 1) ? labs[s >> 1] : 0;
          const float a = alpha[(long long)t * Smax + s] + beta[(long long)t * Smax + s];
          const float e = lg[cls] - ls;
          float v = 0.f;
          if (a != NEG_INF) v = expf(a - e + nl);
          if (s & 1) val[s >> 1] = v;
          else bsum += v;
        }
        bsum = wave_sum(bsum);
        if ((tid & 63) == 0) bred[tid >> 6] = bsum;
        __syncthreads();
        float* qt = q + tt * C;
        for (int u = tid; u < U; u += nthr) {
          if (hd[u]) {
            float sacc = 0.f;
            for (int v = u; v >= 0; v = nxt[v]) sacc += val[v];
            qt[labs[u]] += wk * sacc;                          // single writer per class
          }
        }
        if (tid == 0) qt[0] += wk * (bred[0] + bred[1]);
        __syncthreads();
      }
    }
  }
  for (int tt = 0; tt < TCH; ++tt) {
    const int t = t0 + tt;
    if (t >= T) break;
    float* g = grad + ((long long)t * Bn + b) * ldg;
    if (tt < nt) {
      if (accumulate) for (int c = tid; c < C; c += nthr) g[c] += scale * q[tt * C + c];
      else for (int c = tid; c < C; c += nthr) g[c] = scale * q[tt * C + c];
    } else if (!accumulate) {
      for (int c = tid; c < C; c += nthr) g[c] = 0.f;
    }
  }
}

struct MwerLayout {
  size_t lse, ab, chain, w, total;
  int Smax, Umax;
};
MwerLayout mwer_layout(int T, int B, int K, int max_hyp_len) {
  MwerLayout m;
  const size_t N = (size_t)B * K;
  m.Smax = 2 * max_hyp_len + 1;
  m.Umax = max_hyp_len > 0 ? max_hyp_len : 1;
  m.lse = 0;
  m.ab = align_up((size_t)T * B * sizeof(float), 256);
  m.chain = m.ab + align_up(2 * N * T * (size_t)m.Smax * sizeof(float), 256);
  m.w = m.chain + align_up(N * 2 * (size_t)m.Umax * sizeof(int), 256);
  m.total = m.w + align_up(N * sizeof(float), 256);
  return m;
}

}  // namespace

extern "C" size_t ds2_ctc_mwer_workspace_bytes(int T, int B, int K, int max_hyp_len) {
  if (T <= 0 || B <= 0 || K <= 0 || max_hyp_len < 0) return 0;
  return mwer_layout(T, B, K, max_hyp_len).total;
}

extern "C" int ds2_ctc_mwer_f32(const float* logits, int ld, int T, int B, int C, int K, const int* hyps_dev, const long long* hyp_off_dev,
                                const int* hyp_lens_dev, const int* hyp_valid_dev, const int* in_lens_dev, int max_hyp_len,
                                const float* risk_dev, float* loss_dev, float* nll_hyp_dev, float* post_dev, float* grad, int ldg,
                                float grad_scale, int accumulate, int lattice, void* ws, size_t ws_bytes, void* stream) {
  // every size and pointer is checked before the first launch
  DS2_REQUIRE(logits && hyps_dev && hyp_off_dev && hyp_lens_dev && in_lens_dev && risk_dev && loss_dev && nll_hyp_dev && post_dev,
              "ds2_ctc_mwer_f32: null pointer");
  DS2_REQUIRE(T > 0 && B > 0 && C > 1, "ds2_ctc_mwer_f32: bad dims (T=%d B=%d C=%d)", T, B, C);
  DS2_REQUIRE(K >= 1, "ds2_ctc_mwer_f32: K must be >= 1, got %d", K);
  DS2_REQUIRE((long long)B * K <= INT_MAX / 2 && (long long)T * B <= INT_MAX, "ds2_ctc_mwer_f32: B * K or T * B too large (T=%d B=%d K=%d)", T, B, K);
  DS2_REQUIRE(max_hyp_len >= 0 && max_hyp_len <= (INT_MAX - 1) / 2, "ds2_ctc_mwer_f32: max_hyp_len must be >= 0, got %d", max_hyp_len);
  DS2_REQUIRE(ld >= C && (!grad || ldg >= C), "ds2_ctc_mwer_f32: row pitch below C (ld=%d ldg=%d C=%d)", ld, ldg, C);
  DS2_REQUIRE(accumulate == 0 || accumulate == 1, "ds2_ctc_mwer_f32: accumulate must be 0 or 1");
  DS2_REQUIRE(lattice == 0 || lattice == 1, "ds2_ctc_mwer_f32: lattice must be 0 or 1");
  DS2_REQUIRE(grad_scale - grad_scale == 0.f, "ds2_ctc_mwer_f32: grad_scale must be finite, got %g", (double)grad_scale);   // (NaN, +-inf fail)
  const MwerLayout m = mwer_layout(T, B, K, max_hyp_len);
  const int Smax = m.Smax, Umax = m.Umax;
  const size_t lds = (size_t)2 * Smax * sizeof(float);
  const bool wave = lattice == 0 && Smax <= 128;
  DS2_REQUIRE(wave || lds <= 64 * 1024, "ds2_ctc_mwer_f32: hypotheses too long for LDS lattice rows (Smax=%d)", Smax);
  const size_t lds_chain = (size_t)Umax * sizeof(int);
  const size_t lds2 = ((size_t)TCH * C + Umax) * sizeof(float) + 3 * (size_t)Umax * sizeof(int);
  DS2_REQUIRE(!grad || (lds2 <= 64 * 1024 && lds_chain <= 64 * 1024), "ds2_ctc_mwer_f32: C/S too large for LDS (C=%d Smax=%d)", C, Smax);
  DS2_REQUIRE(ws && ws_bytes >= m.total, "ds2_ctc_mwer_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int N = B * K;
  float* lse = (float*)((char*)ws + m.lse);
  float* ab = (float*)((char*)ws + m.ab);
  int* chain = (int*)((char*)ws + m.chain);
  float* w = (float*)((char*)ws + m.w);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3(ceil_div(T * B, 4)), dim3(256), 0, s, logits, ld, T, B, C, in_lens_dev, lse);
  DS2_LAUNCH_CHECK("ctc_lse_kernel");
  if (wave) {
    hipLaunchKernelGGL((ctc_lattice_wave_kernel<false, true>), dim3(N, 2), dim3(64), 0, s, logits, ld, T, B, C, hyps_dev, (const int*)nullptr,
                       in_lens_dev, hyp_lens_dev, (const float*)lse, ab, Smax, nll_hyp_dev, 0.f, (const int*)nullptr, K, hyp_off_dev,
                       hyp_valid_dev);
    DS2_LAUNCH_CHECK("ctc_lattice_wave_kernel (mwer)");
  } else {
    int threads = ceil_div(Smax, 64) * 64;
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL((ctc_lattice_kernel<false, true>), dim3(N, 2), dim3(threads), lds, s, logits, ld, T, B, C, hyps_dev, (const int*)nullptr,
                       in_lens_dev, hyp_lens_dev, (const float*)lse, ab, Smax, nll_hyp_dev, 0.f, (const int*)nullptr, K, hyp_off_dev,
                       hyp_valid_dev);
    DS2_LAUNCH_CHECK("ctc_lattice_kernel (mwer)");
  }
  hipLaunchKernelGGL(ctc_mwer_weights_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, s, (const float*)nll_hyp_dev, risk_dev, in_lens_dev, B, K,
                     post_dev, loss_dev, w);
  DS2_LAUNCH_CHECK("ctc_mwer_weights_kernel");
  if (grad) {
    hipLaunchKernelGGL(ctc_mwer_chain_kernel, dim3(N), dim3(128), lds_chain, s, hyps_dev, hyp_off_dev, hyp_lens_dev, (const float*)nll_hyp_dev,
                       (const float*)w, Umax, chain);
    DS2_LAUNCH_CHECK("ctc_mwer_chain_kernel");
    hipLaunchKernelGGL(ctc_mwer_grad_kernel, dim3(ceil_div(T, TCH), B), dim3(128), lds2, s, logits, ld, grad, ldg, T, B, C, K, hyps_dev,
                       hyp_off_dev, hyp_lens_dev, in_lens_dev, (const float*)lse, (const float*)ab, Smax, (const float*)nll_hyp_dev,
                       (const float*)w, (const int*)chain, Umax, grad_scale, accumulate);
    DS2_LAUNCH_CHECK("ctc_mwer_grad_kernel");
  }
  return 0;
}
