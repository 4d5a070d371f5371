// Fused flat-buffer AdamW (decoupled weight decay), one launch for all parameters.
// Same update as torch.optim.AdamW single-tensor path (trainers/__main__.py:41-47; hyper-parameters
// asr_deepspeech/config.yml:41-47):  p *= 1 - lr*wd ; m,v EMA ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
// HBM-bound: 16 B read + 12 B write per parameter... (p,g,m,v in; p,m,v out) = 28 B/param.
#include "common.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2_sqrt, float gscale, const int* __restrict__ apply) {
  if (apply && *apply <= 0) return;                     // device-side gate (1 = apply; 0 / -1: the step was found invalid after this launch was enqueued)
  const long long n4 = n / 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    pp *= (1.f - lr * wd);
    mm = b1 * mm + (1.f - b1) * gg;
    vv = b2 * vv + (1.f - b2) * gg * gg;
    f32x4 den;
    den.x = sqrtf(vv.x) / bc2_sqrt + eps; den.y = sqrtf(vv.y) / bc2_sqrt + eps;
    den.z = sqrtf(vv.z) / bc2_sqrt + eps; den.w = sqrtf(vv.w) / bc2_sqrt + eps;
    pp -= (lr / bc1) * mm / den;
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  // tail
  const long long tail0 = n4 * 4;
  for (long long i = tail0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pp = p[i], gg = g[i] * gscale, mm = m[i], vv = v[i];
    pp *= (1.f - lr * wd);
    mm = b1 * mm + (1.f - b1) * gg;
    vv = b2 * vv + (1.f - b2) * gg * gg;
    pp -= (lr / bc1) * mm / (sqrtf(vv) / bc2_sqrt + eps);
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, long long n, float s) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= s;
}

// fp32 mode's split products for the conv stack (engine.F32_CONV): r = x - float(bf16(x)), the part of x a bf16 operand drops; feeding r
// through the bf16 mode's own cast / pack kernels yields the "lo" operand of the three-term product
__global__ __launch_bounds__(256) void bf16_residual_kernel(const float* __restrict__ x, float* __restrict__ r, long long n4, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float4 o;
    o.x = v.x - (float)(__bf16)v.x; o.y = v.y - (float)(__bf16)v.y; o.z = v.z - (float)(__bf16)v.z; o.w = v.w - (float)(__bf16)v.w;
    reinterpret_cast<float4*>(r)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    r[i] = x[i] - (float)(__bf16)x[i];
  }
}

// out = a + b + c (out may be a; c may be NULL: out = a + b): the partial results of a split product
__global__ __launch_bounds__(256) void sum3_kernel(const float* a, const float* __restrict__ b, const float* __restrict__ c, float* out,
                                                   long long n4, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
    const float4 w = c ? reinterpret_cast<const float4*>(c)[i] : float4{0.f, 0.f, 0.f, 0.f};
    float4 o;
    o.x = u.x + v.x + w.x; o.y = u.y + v.y + w.y; o.z = u.z + v.z + w.z; o.w = u.w + v.w + w.w;
    reinterpret_cast<float4*>(out)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    out[i] = a[i] + b[i] + (c ? c[i] : 0.f);
  }
}

}  // namespace

// step is 1-based.  grad_scale multiplies g on the fly (e.g. 1/world_size after an all-reduce SUM).
// apply_flag: NULL, or a device int the kernel reads when it RUNS: <= 0 = leave everything untouched.  It lets the host enqueue the update
// before it knows whether the step is valid (finite loss on every rank, no starved recurrence launch: ds2_rnn_step_gate), i.e. without
// a host synchronisation between backward and the optimizer.
extern "C" int ds2_adamw_gated_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, float grad_scale, const int* apply_flag, void* stream) {
  DS2_REQUIRE(p && g && m && v && n >= 0 && step >= 1, "ds2_adamw_f32: bad args");
  DS2_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0,
              "ds2_adamw_f32: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, bc1, (float)sqrt(bc2), grad_scale, apply_flag);
  DS2_LAUNCH_CHECK("adamw_kernel");
  return 0;
}

extern "C" int ds2_adamw_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, float grad_scale, void* stream) {
  return ds2_adamw_gated_f32(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, nullptr, stream);
}

namespace {
__global__ void add_i64_kernel(long long* __restrict__ x, int n, long long v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += v;
}
}  // namespace

// x[0..n) += v for a small int64 vector: every BatchNorm's num_batches_tracked in one launch (they are views of one buffer: asr_amd/params.py)
extern "C" int ds2_add_i64(long long* x, int n, long long v, void* stream) {
  DS2_REQUIRE(x && n >= 0, "ds2_add_i64: bad args");
  if (n == 0) return 0;
  hipLaunchKernelGGL(add_i64_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, n, v);
  DS2_LAUNCH_CHECK("add_i64_kernel");
  return 0;
}

extern "C" int ds2_scale_f32(float* x, long long n, float s, void* stream) {
  DS2_REQUIRE(x && n >= 0, "ds2_scale_f32: bad args");
  if (n == 0) return 0;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, s);
  DS2_LAUNCH_CHECK("scale_kernel");
  return 0;
}

extern "C" int ds2_bf16_residual_f32(const float* x, float* r, long long n, void* stream) {
  DS2_REQUIRE(x && r && n >= 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)r % 16) == 0, "ds2_bf16_residual_f32: bad args");
  if (n == 0) return 0;
  long long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
  hipLaunchKernelGGL(bf16_residual_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, r, n / 4, n);
  DS2_LAUNCH_CHECK("bf16_residual_kernel");
  return 0;
}

extern "C" int ds2_sum3_f32(const float* a, const float* b, const float* c, float* out, long long n, void* stream) {
  DS2_REQUIRE(a && b && out && n >= 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)out) % 16) == 0, "ds2_sum3_f32: bad args");
  if (n == 0) return 0;
  long long blocks = (n / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
  hipLaunchKernelGGL(sum3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, c, out, n / 4, n);
  DS2_LAUNCH_CHECK("sum3_kernel");
  return 0;
}

// ---- weight-operand preparation of a whole recurrent stack in ONE launch (bf16 mode, once per optimizer step) -------------------------
// Per layer: the packed bf16 W_hh fragments of both recurrences (the layout of ds2_rnn_pack_whh, bf16 = 1) and the bf16 copies of W_ih
// (the layout of ds2_cast_bf16_both / ds2_cast_transpose_bf16), byte for byte what those per-layer entry points write.  A table in the
// kernel arguments maps a workgroup to its job; every job works on 64 x 64 fp32 tiles staged in LDS, read with 16-byte loads, written with
// 16-byte stores.  One tile of W_hh yields its forward AND its backward fragments (the per-layer kernel reads W_hh once for each, the
// backward half with 64-byte runs of scalar loads).
namespace {

typedef __bf16 pbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pbf16x4 __attribute__((ext_vector_type(4)));

enum { PREP_PACK_TILE = 0, PREP_PACK_VEC = 1, PREP_CAST_T = 2 };
constexpr int PREP_MAX_JOBS = 32;
struct PrepJob {
  const float* src;
  void* d0;            // pack: forward fragments ; cast: transposed copy
  void* d1;            // pack: backward fragments ; cast: row-major copy or NULL
  int kind, first;     // first workgroup of this job
  int G, H;            // pack
  int R, Cc, lds, ldt, ldr, vec, gx;   // cast: src (R, Cc) pitch lds ; dT pitch ldt ; dR pitch ldr ; float4-readable ; tiles along Cc
};
struct PrepTable {
  int njobs;
  PrepJob job[PREP_MAX_JOBS];
};

constexpr int PT = 68;   // tile pitch of the pack jobs (16-byte aligned rows); the cast jobs keep cast_transpose_bf16_kernel's 65

__device__ __forceinline__ pbf16x8 to_bf16x8(const float* v) {
  pbf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
  return o;
}

// H % 16 == 0: a 64-row tile of the (G*H, H) matrix of one direction never cuts a 16-unit slice, and its row chunks of 32 are the backward
// operand's chunks.  Everything outside the matrix is staged as zero, as rnn_pack_kernel pads.
__device__ __forceinline__ void prep_pack_tile(const PrepJob& jb, int lb, float* tile) {
  const int G = jb.G, H = jb.H, GH = G * H;
  const int rt = (GH + 63) >> 6, ct = (H + 63) >> 6;
  const int dir = lb / (rt * ct), rem = lb % (rt * ct);
  const int r0 = (rem / ct) * 64, c0 = (rem % ct) * 64;
  const int nsl = H >> 4, nch = (H + 31) >> 5, nchb = (GH + 31) >> 5;
  const float* src = jb.src + (long long)dir * GH * H;
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int rl = pass * 16 + (tid >> 4), cl = (tid & 15) * 4;
    const int r = r0 + rl, c = c0 + cl;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (r < GH && c < H) q = *reinterpret_cast<const f32x4*>(src + (long long)r * H + c);      // (H % 4 == 0: c < H is c + 4 <= H)
    *reinterpret_cast<f32x4*>(tile + rl * PT + cl) = q;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {                                  // forward fragments: [dir][slice][gate][32-k chunk][lane] = 8 consecutive k of row (g, j)
    const int v = p * 256 + tid, lane = v & 63, cc = (v >> 6) & 1, i = v >> 7;
    const int row = r0 + 16 * i, c = (c0 >> 5) + cc;
    if (row < GH && c < nch) {
      const int g = row / H, slice = (row % H) >> 4;
      const float* t = tile + (16 * i + (lane & 15)) * PT + cc * 32 + (lane >> 4) * 8;
      float x[8];
      *reinterpret_cast<f32x4*>(x) = *reinterpret_cast<const f32x4*>(t);
      *reinterpret_cast<f32x4*>(x + 4) = *reinterpret_cast<const f32x4*>(t + 4);
      reinterpret_cast<pbf16x8*>(jb.d0)[((((long long)dir * nsl + slice) * G + g) * nch + c) * 64 + lane] = to_bf16x8(x);
    }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {                                  // backward fragments: [dir][slice][32-row chunk][lane] = 8 consecutive rows of column j
    const int v = p * 256 + tid, lane = v & 63, sj = (v >> 6) & 3, ci = v >> 8;
    const int cb = (r0 >> 5) + ci, slice = (c0 >> 4) + sj;
    if (cb < nchb && slice < nsl) {
      const float* t = tile + (ci * 32 + (lane >> 4) * 8) * PT + sj * 16 + (lane & 15);
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = t[e * PT];
      reinterpret_cast<pbf16x8*>(jb.d1)[(((long long)dir * nsl + slice) * nchb + cb) * 64 + lane] = to_bf16x8(x);
    }
  }
}

// any H % 4 == 0: rnn_pack_kernel<true>'s own indexing, one 16-byte fragment per thread
__device__ __forceinline__ void prep_pack_vec(const PrepJob& jb, int lb) {
  const int G = jb.G, H = jb.H;
  const int nsl = (H + 15) >> 4, nch = (H + 31) >> 5, nchb = (G * H + 31) >> 5;
  const long long nf = (long long)2 * nsl * G * nch * 64, nb = (long long)2 * nsl * nchb * 64;
  const long long i = (long long)lb * 256 + threadIdx.x;
  if (i >= nf + nb) return;
  const bool fwd = i < nf;
  const long long ii = fwd ? i : i - nf;
  const int lane = (int)(ii & 63);
  long long r = ii >> 6;
  float v[8];
  if (fwd) {
    const int c = r % nch; r /= nch;
    const int g = r % G; r /= G;
    const int slice = r % nsl, dir = r / nsl;
    const int j = slice * 16 + (lane & 15), k0 = c * 32 + (lane >> 4) * 8;
    const float* src = jb.src + ((long long)dir * G * H + g * H + j) * H + k0;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (j < H && k0 + e < H) ? src[e] : 0.f;
  } else {
    const int c = r % nchb; r /= nchb;
    const int slice = r % nsl, dir = r / nsl;
    const int j = slice * 16 + (lane & 15), k0 = c * 32 + (lane >> 4) * 8;
    const float* src = jb.src + ((long long)dir * G * H + k0) * H + j;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (j < H && k0 + e < G * H) ? src[(long long)e * H] : 0.f;
  }
  reinterpret_cast<pbf16x8*>(fwd ? jb.d0 : jb.d1)[ii] = to_bf16x8(v);
}

// cast_transpose_bf16_kernel (gemm_bf16.hip) without the column sums: dT[c][r] = bf16(src[r][c]), optionally dR[r][c] = bf16(src[r][c])
__device__ __forceinline__ void prep_cast_t(const PrepJob& jb, int lb, float* tile) {
  const int R = jb.R, Cc = jb.Cc, ldt = jb.ldt, ldr = jb.ldr;
  __bf16* dstT = (__bf16*)jb.d0;
  __bf16* dstR = (__bf16*)jb.d1;
  const int r0 = (lb / jb.gx) * 64, c0 = (lb % jb.gx) * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int rl = pass * 16 + (tid >> 4), cl = (tid & 15) * 4;
    const int r = r0 + rl, c = c0 + cl;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      const float* sp = jb.src + (long long)r * jb.lds + c;
      if (jb.vec && c + 4 <= Cc) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(sp);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c + j < Cc) ? sp[j] : 0.f;
      }
      if (dstR && c < ldr) *reinterpret_cast<pbf16x4*>(dstR + (long long)r * ldr + c) = pbf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[rl * 65 + cl + j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int cl = pass * 32 + (tid >> 3), rl = (tid & 7) * 8;
    const int c = c0 + cl, r = r0 + rl;
    if (c < Cc && r < ldt) {                      // rows >= R were staged as zeros; ldt % 8 == 0 keeps the 8-run inside the pitch
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = tile[(rl + j) * 65 + cl];
      *reinterpret_cast<pbf16x8*>(dstT + (long long)c * ldt + r) = to_bf16x8(x);
    }
  }
}

__global__ __launch_bounds__(256) void weight_prep_kernel(const PrepTable tab) {
  __shared__ __attribute__((aligned(16))) float tile[64 * PT];
  const int bid = blockIdx.x;
  int j = 0;
  while (j + 1 < tab.njobs && bid >= tab.job[j + 1].first) ++j;      // (uniform: a few scalar loads)
  const PrepJob& jb = tab.job[j];
  const int lb = bid - jb.first;
  if (jb.kind == PREP_PACK_TILE) prep_pack_tile(jb, lb, tile);
  else if (jb.kind == PREP_PACK_VEC) prep_pack_vec(jb, lb);
  else prep_cast_t(jb, lb, tile);
}

}  // namespace

// layers[i]: whh (2, gates*H, H) fp32 contiguous -> wp_fwd / wp_bwd (ds2_rnn_packed_bytes(gates, H, 0 | 1, 1) bytes), skipped when whh is
// NULL; wih (R, Cc) fp32, row pitch ld_wih -> wih_t (Cc, ld_t) bf16 = wih^T (ld_t % 8 == 0, ld_t >= R) and, when wih_r is not NULL,
// wih_r (R, ld_r) bf16 (ld_r % 8 == 0, Cc <= ld_r <= the next multiple of 64); pads zero; skipped when wih is NULL.
extern "C" int ds2_weight_prep_bf16(const ds2_prep_layer* layers, int n, void* stream) {
  DS2_REQUIRE(layers && n > 0, "ds2_weight_prep_bf16: bad args");
  PrepTable tab;
  tab.njobs = 0;
  long long blocks = 0;
  auto flush = [&]() -> int {
    if (tab.njobs == 0) return 0;
    hipLaunchKernelGGL(weight_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tab);
    DS2_LAUNCH_CHECK("weight_prep_kernel");
    tab.njobs = 0;
    blocks = 0;
    return 0;
  };
  for (int i = 0; i < n; ++i) {
    const ds2_prep_layer& L = layers[i];
    if (tab.njobs + 2 > PREP_MAX_JOBS && flush()) return 1;                       // (more than 16 layers: a second launch)
    if (L.whh) {
      DS2_REQUIRE(L.gates == 1 || L.gates == 3 || L.gates == 4, "ds2_weight_prep_bf16: gates must be 1, 3 or 4");
      DS2_REQUIRE(L.wp_fwd && L.wp_bwd && L.H > 0 && (L.H % 4) == 0 && ((uintptr_t)L.whh % 16) == 0 && ((uintptr_t)L.wp_fwd % 16) == 0 &&
                      ((uintptr_t)L.wp_bwd % 16) == 0,
                  "ds2_weight_prep_bf16: bad W_hh arguments (layer %d)", i);
      PrepJob& jb = tab.job[tab.njobs++];
      jb = PrepJob{};
      jb.src = L.whh; jb.d0 = L.wp_fwd; jb.d1 = L.wp_bwd; jb.G = L.gates; jb.H = L.H; jb.first = (int)blocks;
      if ((L.H % 16) == 0) {
        jb.kind = PREP_PACK_TILE;
        blocks += 2LL * ceil_div(L.gates * L.H, 64) * ceil_div(L.H, 64);
      } else {
        jb.kind = PREP_PACK_VEC;
        const long long nsl = ceil_div(L.H, 16);
        const long long nv = 2 * nsl * L.gates * ceil_div(L.H, 32) * 64 + 2 * nsl * ceil_div(L.gates * L.H, 32) * 64;
        blocks += (nv + 255) / 256;
      }
    }
    if (L.wih) {
      DS2_REQUIRE(L.wih_t && L.R > 0 && L.Cc > 0 && L.ld_wih >= L.Cc && L.ld_t >= L.R && (L.ld_t % 8) == 0 && ((uintptr_t)L.wih_t % 16) == 0,
                  "ds2_weight_prep_bf16: bad W_ih arguments (layer %d)", i);
      DS2_REQUIRE(!L.wih_r || (L.ld_r >= L.Cc && L.ld_r <= ceil_div(L.Cc, 64) * 64 && (L.ld_r % 8) == 0 && ((uintptr_t)L.wih_r % 16) == 0),
                  "ds2_weight_prep_bf16: bad row-major pitch (layer %d, ld_r=%d)", i, L.ld_r);
      PrepJob& jb = tab.job[tab.njobs++];
      jb = PrepJob{};
      jb.kind = PREP_CAST_T;
      jb.src = L.wih; jb.d0 = L.wih_t; jb.d1 = L.wih_r; jb.first = (int)blocks;
      jb.R = L.R; jb.Cc = L.Cc; jb.lds = L.ld_wih; jb.ldt = L.ld_t; jb.ldr = L.wih_r ? L.ld_r : 0;
      jb.vec = ((L.ld_wih % 4) == 0) && (((uintptr_t)L.wih % 16) == 0);
      jb.gx = ceil_div(L.wih_r ? (L.Cc > L.ld_r ? L.Cc : L.ld_r) : L.Cc, 64);
      blocks += (long long)jb.gx * ceil_div(L.ld_t, 64);
    }
    DS2_REQUIRE(blocks < (1LL << 31), "ds2_weight_prep_bf16: too many tiles");
  }
  return flush();
}
