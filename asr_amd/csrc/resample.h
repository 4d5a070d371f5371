// Sample-rate conversion of the packed waveform feed (get_loader(front_end="gpu", resample=True)): the unpack pass of stft.hip with a
// band-limited interpolation in it.  A ragged batch of waveforms at ANY rate -> the zero-padded (B, n_out_max) fp32 batch at the target
// rate that tempo.hip's and stft.hip's kernels read; the off-rate samples never exist as fp32 rows in HBM.  Contract: include/ds2hip.h.
//
// Per utterance the rates reduce to L / M (up / down); output m sits at input time m M / L: i0 = (m M) div L, phase p = (m M) mod L, and
//     y[m] = sum_{j < P} tab[p][j] * x[i0 - J + 1 + j],   P = 2 J,   x = 0 outside [0, n)
// with the (L, P) Kaiser-windowed sinc table the caller built (asr_amd.ops.resample_taps).
//
// Mapping: one workgroup per (output row, tile of kRsTile outputs).  The tile's input window — (kRsTile - 1) M / L + P samples, at most
// kRsWin — is staged ONCE in LDS as fp32 (int16 converted on the way), with one 128-bit load per 8 int16 samples (two per 8 fp32) under the
// packed buffer's alignment rule.  A thread then owns four outputs 256 apart (consecutive lanes = consecutive outputs: coalesced stores;
// lane stride M / L dwords in the window) and runs the P-tap dot product sequentially in fp32 with fused multiply-adds.
// Taps: a table of at most kRsTabLds floats (L <= 2 at any supported ratio; every L * P <= 4096) is copied to LDS, where the L = 1 reads
// are broadcasts; a larger one (44.1 kHz -> 16 kHz: 160 x 188) is read per lane through L1 / L2 — consecutive outputs use phases
// M mod L apart, each lane walks its own row.  No atomics, a fixed summation order: reruns are bit-identical.
// Included at the end of stft.hip, next to wave_unpack_kernel, whose vector types, chunk size (kChunk = 8) and dtype tags it shares.
#pragma once
#ifndef DS2_STFT_UNPACK_DEFS
#error "resample.h is the tail of stft.hip (it uses wave_unpack_kernel's kChunk, i16x8 and dtype tags): include it nowhere else"
#endif
#include "common.h"

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsPerThread = 4;
constexpr int kRsTile = kRsThreads * kRsPerThread;      // outputs per workgroup
constexpr int kRsMaxJ = 512;                            // taps per side: P = 2 J <= 1024
constexpr int kRsMaxRatio = 8;                          // M <= 8 L and L <= 8 M
constexpr int kRsMaxLM = 1 << 16;                       // keeps (k M + r) for k < kRsTile inside 32 bits
// window: lead (<= 7, the start rounded down to a multiple of 8) + (kRsTile - 1) * kRsMaxRatio + 2 * kRsMaxJ samples, rounded up to 8
constexpr int kRsWin = 9216;
constexpr int kRsTabLds = 4096;                         // tables up to this many floats are staged in LDS
constexpr long long kRsMaxTabElems = 1LL << 22;

static_assert(7 + (kRsTile - 1) * kRsMaxRatio + 2 * kRsMaxJ <= kRsWin && kRsWin % kChunk == 0, "the window of a tile fits its LDS buffer");

// acc[q] = sum_j T[tap[q] + j] * win[xb[q] + j], j ascending, one fused multiply-add per tap
__device__ __forceinline__ void dot4(const float* __restrict__ T, const float* __restrict__ win, const int (&tap)[kRsPerThread],
                                     const int (&xb)[kRsPerThread], int P, float (&acc)[kRsPerThread]) {
#pragma unroll 4
  for (int j = 0; j < P; ++j) {
#pragma unroll
    for (int q = 0; q < kRsPerThread; ++q) acc[q] = fmaf(T[tap[q] + j], win[xb[q] + j], acc[q]);
  }
}

// A row whose description is outside the contract is written as zeros: nothing is read outside [0, packed_elems) or [0, tab_elems).
// The host wrapper rejects such descriptions before the launch (ops.wave_resample); this is the second line.
template <bool I16>
__global__ __launch_bounds__(kRsThreads) void wave_resample_kernel(const void* __restrict__ packed, long long packed_elems,
                                                                   const int* __restrict__ offsets, const int* __restrict__ lengths,
                                                                   const int* __restrict__ src_index, const int* __restrict__ Ls,
                                                                   const int* __restrict__ Ms, const int* __restrict__ Js,
                                                                   const int* __restrict__ tab_bases, const float* __restrict__ tab,
                                                                   long long tab_elems, int B, int n_out_max, float* __restrict__ out,
                                                                   long long ld_out) {
  __shared__ __attribute__((aligned(16))) float win[kRsWin];
  __shared__ float taps[kRsTabLds];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * kRsTile;
  if (m0 >= n_out_max) return;
  const int m_hi = min(m0 + kRsTile, n_out_max);
  float* y = out + (long long)b * ld_out;

  const int src = src_index[b];
  int off = 0, len = 0, L = 1, M = 1, J = 0;
  long long tb = 0, n_out = 0;
  if (src >= 0 && src < B) {
    off = offsets[src], len = lengths[src], L = Ls[src], M = Ms[src], J = Js[src], tb = tab_bases[src];
    const long long end = (long long)off + (((long long)len + kChunk - 1) & ~(long long)(kChunk - 1));
    bool ok = off >= 0 && !(off & (kChunk - 1)) && len >= 0 && end <= packed_elems && L >= 1 && M >= 1 && L <= kRsMaxLM && M <= kRsMaxLM &&
              (long long)M <= (long long)kRsMaxRatio * L && (long long)L <= (long long)kRsMaxRatio * M;
    if (ok && !(L == 1 && M == 1)) ok = J >= 1 && J <= kRsMaxJ && tb >= 0 && tb + (long long)L * 2 * J <= tab_elems;
    if (ok) {
      n_out = ((long long)len * L + M - 1) / M;
      ok = n_out <= n_out_max;
    }
    if (!ok) n_out = 0, len = 0;
  }
  if (m0 >= n_out) {                                    // padding, an empty or a rejected row
    for (int m = m0 + tid; m < m_hi; m += kRsThreads) y[m] = 0.0f;
    return;
  }
  if (L == 1 && M == 1) {                               // already at the target rate: the unpack pass, bit for bit
    for (int m = m0 + tid; m < m_hi; m += kRsThreads) {
      float v = 0.0f;
      if (m < len) v = I16 ? (float)static_cast<const short*>(packed)[off + m] * 0x1p-15f : static_cast<const float*>(packed)[off + m];
      y[m] = v;
    }
    return;
  }

  const int P = 2 * J;
  const long long t0 = (long long)m0 * M;
  const long long q0 = t0 / L;                          // i0 of the tile's first output
  const int r0 = (int)(t0 - q0 * L);                    // and its phase
  const int m_end = (int)min((long long)m_hi, n_out);   // outputs [m0, m_end) are computed, [m_end, m_hi) are zeros
  const int di_last = (int)(((long long)(m_end - 1 - m0) * M + r0) / L);
  const long long i_lo = q0 - J + 1;                    // first input sample the tile reads
  const long long a_lo = i_lo & ~(long long)(kChunk - 1);      // rounded down to a multiple of 8 (also below 0)
  const int lead = (int)(i_lo - a_lo);
  const int W = lead + di_last + P;                     // the window is x[a_lo .. a_lo + W)
  if (W > kRsWin) {                                     // (unreachable inside the limits above)
    for (int m = m0 + tid; m < m_hi; m += kRsThreads) y[m] = 0.0f;
    return;
  }
  const int chunks = (W + kChunk - 1) / kChunk;
  for (int c = tid; c < chunks; c += kRsThreads) {
    const long long g = a_lo + (long long)c * kChunk;
    float v[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) v[i] = 0.0f;
    if (g >= 0 && g < len) {                            // the whole chunk lies inside the buffer (gaps up to the next multiple of 8 exist)
      const int rem = len - (int)g;
      if constexpr (I16) {
        const i16x8 s = *reinterpret_cast<const i16x8*>(static_cast<const short*>(packed) + off + g);
#pragma unroll
        for (int i = 0; i < kChunk; ++i) v[i] = (i < rem) ? (float)s[i] * 0x1p-15f : 0.0f;
      } else {
        const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(packed) + off + g);
        const f32x4 lo = p[0], hi = p[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = (i < rem) ? lo[i] : 0.0f;
          v[4 + i] = (4 + i < rem) ? hi[i] : 0.0f;
        }
      }
    }
    f32x4 a, d;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = v[i], d[i] = v[4 + i];
    *reinterpret_cast<f32x4*>(win + c * kChunk) = a;
    *reinterpret_cast<f32x4*>(win + c * kChunk + 4) = d;
  }
  const int tab_len = L * P;                            // <= 2^16 * 2^10
  const bool tab_in_lds = tab_len <= kRsTabLds;
  if (tab_in_lds)
    for (int i = tid; i < tab_len; i += kRsThreads) taps[i] = tab[tb + i];
  __syncthreads();

  int tap[kRsPerThread], xb[kRsPerThread];
  float acc[kRsPerThread];
#pragma unroll
  for (int q = 0; q < kRsPerThread; ++q) {
    const int k = tid + q * kRsThreads;
    const unsigned t = (unsigned)r0 + (unsigned)(m0 + k < m_end ? k : 0) * (unsigned)M;     // (an output past the end redoes the first)
    const unsigned di = t / (unsigned)L;
    tap[q] = (int)(t - di * (unsigned)L) * P;
    xb[q] = lead + (int)di;
    acc[q] = 0.0f;
  }
  if (tab_in_lds)
    dot4(taps, win, tap, xb, P, acc);
  else
    dot4(tab + tb, win, tap, xb, P, acc);
#pragma unroll
  for (int q = 0; q < kRsPerThread; ++q) {
    const int m = m0 + tid + q * kRsThreads;
    if (m < m_hi) y[m] = m < m_end ? acc[q] : 0.0f;
  }
}

}  // namespace

extern "C" long long ds2_resample_out_samples(long long n, int L, int M) {
  if (n < 0 || n > (1LL << 31) || L < 1 || M < 1) return -1;
  return (n * L + M - 1) / M;
}

extern "C" int ds2_resample_tile_samples(void) { return kRsTile; }

extern "C" int ds2_wave_resample_f32(const void* packed, long long packed_elems, int dtype, const int* offsets_dev, const int* lengths_dev,
                                     const int* src_index_dev, const int* L_dev, const int* M_dev, const int* J_dev,
                                     const int* tab_base_dev, const float* tab, long long tab_elems, int B, int n_out_max, float* out,
                                     long long ld_out, void* stream) {
  DS2_REQUIRE(offsets_dev && lengths_dev && src_index_dev && L_dev && M_dev && J_dev && tab_base_dev && out, "ds2_wave_resample_f32: null pointer");
  DS2_REQUIRE(dtype == kTagI16 || dtype == kTagF32, "ds2_wave_resample_f32: dtype tag %d (0 = int16, 1 = fp32)", dtype);
  DS2_REQUIRE(B > 0 && B <= 65535 && n_out_max >= 0 && n_out_max <= (1 << 30) && ld_out >= n_out_max,
              "ds2_wave_resample_f32: bad dims (B=%d n_out_max=%d ld_out=%lld)", B, n_out_max, ld_out);
  DS2_REQUIRE(packed_elems >= 0 && packed_elems <= 0x7fffffffLL && packed_elems % kChunk == 0,
              "ds2_wave_resample_f32: packed_elems = %lld: a multiple of 8 in [0, 2^31)", packed_elems);
  DS2_REQUIRE(packed || packed_elems == 0, "ds2_wave_resample_f32: null packed buffer of %lld elements", packed_elems);
  DS2_REQUIRE(tab_elems >= 0 && tab_elems <= kRsMaxTabElems, "ds2_wave_resample_f32: tab_elems = %lld outside [0, 2^22]", tab_elems);
  DS2_REQUIRE(tab || tab_elems == 0, "ds2_wave_resample_f32: null table buffer of %lld elements", tab_elems);
  DS2_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)tab & 3) == 0,
              "ds2_wave_resample_f32: packed must be 16-byte aligned, out and tab 4-byte aligned");
  if (n_out_max == 0) return 0;
  const dim3 grid((unsigned)ceil_div(n_out_max, kRsTile), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == kTagI16)
    hipLaunchKernelGGL(wave_resample_kernel<true>, grid, dim3(kRsThreads), 0, s, packed, packed_elems, offsets_dev, lengths_dev,
                       src_index_dev, L_dev, M_dev, J_dev, tab_base_dev, tab, tab_elems, B, n_out_max, out, ld_out);
  else
    hipLaunchKernelGGL(wave_resample_kernel<false>, grid, dim3(kRsThreads), 0, s, packed, packed_elems, offsets_dev, lengths_dev,
                       src_index_dev, L_dev, M_dev, J_dev, tab_base_dev, tab, tab_elems, B, n_out_max, out, ld_out);
  DS2_LAUNCH_CHECK("wave_resample_kernel");
  return 0;
}
