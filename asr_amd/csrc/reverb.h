// Reverberation of the waveform batch (GpuSpectrogramFrontEnd(reverb=...), audio_conf.rir_dir): every utterance convolved with a room
// impulse response, truncated to the utterance's own length.  Contract: include/ds2hip.h (ds2_reverb_f32).
//
//     y[i] = sum_{k = 0 .. min(i, P - 1)} h[k] x[i - k],   i in [0, n)
//
// The one augmentation that is arithmetic-bound (B = 64, n = 160 000, P = 4 096: 4.2e10 multiply-adds), so the products run on the
// matrix cores in exact fp32: a FIR filter is a GEMM with a Toeplitz operand.  v_mfma_f32_16x16x4_f32 computes D (16 x 16) += A (16 x 4)
// B (4 x 16), bit for bit a k-ordered fmaf chain.  Here the 16 COLUMNS are 16 segments of kRvSeg consecutive outputs and the 16 ROWS are
// 16 consecutive outputs of each segment: with ob the first output of a block, d running over input offsets,
//     Y[m][seg] = sum_d T[m][d] X[d][seg],   T[m][d] = h[m - d] (0 outside [0, P)),   X[d][seg] = x[ob(seg) + d].
// Apart from the two triangular corners of T (15 of P + 15 columns) no product is wasted.
//
// Mapping: one workgroup (4 waves) per (row, tile of kRvTile = 4 x 16 x kRvSeg outputs); a wave owns 16 segments = 16 kRvSeg consecutive
// outputs as kRvBlocks accumulator blocks (the last block overlaps the one before it, kRvSeg not being a multiple of 16: its repeated
// rows are not stored).  The taps are walked in chunks of kRvChunk, ascending; per chunk the x window of the tile (tile + chunk samples:
// zeros left of sample 0 and from n on, so garbage beyond n never enters) and the chunk's taps (zero-padded by 16 on both sides: the
// triangular corners) are staged in LDS.  Per K step a lane reads ONE T value — 16 + m - d, a stride-1 read, equal addresses broadcast —
// which all kRvBlocks blocks reuse, and one X value per block at lane stride kRvSeg = 78 = 2 x 39 dwords: the 16 segments x 2 offsets of a
// 32-lane half fall into 32 different banks.  Within an output the order is fixed: chunks ascending, inside a chunk the taps descending,
// one fused multiply-add each; the zero products of the corners and of the padding add exact zeros.  So the bits of a row depend on
// (x, h) alone; no atomics, reruns are bit-identical.
// Included at the end of stft.hip, after resample.h: it shares nothing with them but the translation unit.
#pragma once
#include "common.h"

namespace {

constexpr int kRvThreads = 256;
constexpr int kRvWaves = kRvThreads / 64;
constexpr int kRvSeg = 78;                               // outputs per segment (MFMA column): 2 x odd, see above
constexpr int kRvBlocks = (kRvSeg + 15) / 16;            // 16-output blocks per segment, the last one starting at kRvSeg - 16
constexpr int kRvWaveTile = 16 * kRvSeg;
constexpr int kRvTile = kRvWaves * kRvWaveTile;          // outputs per workgroup
constexpr int kRvChunk = 1024;                           // taps per pass over the tile
constexpr int kRvMaxTaps = 16384;
constexpr int kRvWin = kRvTile + kRvChunk;               // x window of one chunk
constexpr int kRvTapLds = kRvChunk + 32;

static_assert(kRvSeg % 2 == 0 && (kRvSeg / 2) % 2 == 1 && kRvSeg >= 16, "segment stride: twice an odd number (LDS banks), at least one block");
static_assert(kRvChunk % 4 == 0 && kRvMaxTaps % kRvChunk == 0, "tap chunks are whole K steps");

// A row whose description is outside the contract is written as zeros: nothing is read outside audio's row or [0, rir_elems).
// The host wrapper rejects such descriptions before the launch (ops.reverb); this is the second line.
__global__ __launch_bounds__(kRvThreads) void reverb_kernel(const float* __restrict__ audio, long long ld_audio,
                                                            const int* __restrict__ n_samples, const float* __restrict__ rir,
                                                            long long rir_elems, const long long* __restrict__ rir_base,
                                                            const int* __restrict__ rir_taps, int n_max, float* __restrict__ out,
                                                            long long ld_out) {
  __shared__ float win[kRvWin];
  __shared__ float taps[kRvTapLds];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int i0 = blockIdx.x * kRvTile;
  if (i0 >= n_max) return;
  const int i_hi = min(i0 + kRvTile, n_max);
  const float* x = audio + (long long)b * ld_audio;
  float* y = out + (long long)b * ld_out;

  int n = n_samples[b];
  const int P = rir_taps[b];
  const long long base = rir_base[b];
  if (n < 0 || n > n_max || P < 0 || P > kRvMaxTaps || base < 0 || base + P > rir_elems) n = 0;
  if (i0 >= n) {                                        // padding, an empty or a rejected row
    for (int i = i0 + tid; i < i_hi; i += kRvThreads) y[i] = 0.0f;
    return;
  }
  if (P == 0) {                                         // not reverberated: the row, bit for bit
    for (int i = i0 + tid; i < i_hi; i += kRvThreads) y[i] = i < n ? x[i] : 0.0f;
    return;
  }

  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;          // A: row col, k quad.  B: k quad, column col.  C/D: column col, rows 4 quad + r
  const int w0 = wave * kRvWaveTile;                    // the wave's first output, relative to i0
  const bool wave_live = i0 + w0 < n;                   // (a wave wholly beyond n has only zeros to write)
  f32x4 acc[kRvBlocks];
#pragma unroll
  for (int j = 0; j < kRvBlocks; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const float* h = rir + base;
  for (int k0 = 0; k0 < P; k0 += kRvChunk) {
    const int pc = min(kRvChunk, P - k0);               // taps of this chunk
    const int steps = ((pc + 15 + 15) >> 4) << 2;       // K steps of 4, a multiple of 4: d in [-DL, 16), DL = 4 steps - 16 >= pc - 1
    const int DL = 4 * steps - 16;
    const int W = kRvTile + DL;                         // win[q] = x[g_lo + q]
    const int g_lo = i0 - k0 - DL;
    __syncthreads();                                    // (the previous chunk's reads are done)
    for (int q = tid; q < W; q += kRvThreads) {
      const int g = g_lo + q;
      win[q] = (g >= 0 && g < n) ? x[g] : 0.0f;
    }
    for (int q = tid; q < 4 * steps + 16; q += kRvThreads) {      // taps[16 + k] = h[k0 + k], zeros for k in [-16, 0) and [pc, 4 steps)
      const int k = q - 16;
      taps[q] = (k >= 0 && k < pc) ? h[k0 + k] : 0.0f;
    }
    __syncthreads();
    if (wave_live) {
      const float* tp = taps + 16 + col - quad + DL;    // T[m = col][d = -DL + 4 t + quad] = taps[16 + m - d]
      const float* xp = win + w0 + col * kRvSeg + quad; // X[d][seg = col] of block j = win[w0 + seg kRvSeg + bo_j + DL + d]
      for (int t = 0; t < steps; t += 4) {              // 4 K steps = 16 input offsets per trip: 4 T reads, 4 kRvBlocks X reads
        float a[4], xv[4][kRvBlocks];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a[u] = tp[-4 * (t + u)];
#pragma unroll
          for (int j = 0; j < kRvBlocks; ++j) xv[u][j] = xp[(j < kRvBlocks - 1 ? 16 * j : kRvSeg - 16) + 4 * (t + u)];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int j = 0; j < kRvBlocks; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], xv[u][j], acc[j], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kRvBlocks; ++j) {
    const int bo = j < kRvBlocks - 1 ? 16 * j : kRvSeg - 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = bo + 4 * quad + r;                  // position in the segment
      if (j == kRvBlocks - 1 && s < 16 * (kRvBlocks - 1)) continue;      // the overlap: block j - 1 has it
      const int i = i0 + w0 + col * kRvSeg + s;
      if (i < i_hi) y[i] = i < n ? acc[j][r] : 0.0f;
    }
  }
}

}  // namespace

extern "C" int ds2_reverb_max_taps(void) { return kRvMaxTaps; }
extern "C" int ds2_reverb_tile_samples(void) { return kRvTile; }
extern "C" int ds2_reverb_tap_chunk(void) { return kRvChunk; }

extern "C" int ds2_reverb_f32(const float* audio, long long ld_audio, const int* n_samples_dev, const float* rir, long long rir_elems,
                              const long long* rir_base_dev, const int* rir_taps_dev, int B, int n_max, float* out, long long ld_out,
                              void* stream) {
  DS2_REQUIRE(audio && n_samples_dev && rir_base_dev && rir_taps_dev && out, "ds2_reverb_f32: null pointer");
  DS2_REQUIRE(B > 0 && B <= 65535 && n_max >= 0 && n_max <= (1 << 30) && ld_out >= n_max && ld_audio >= n_max,
              "ds2_reverb_f32: bad dims (B=%d n_max=%d ld_audio=%lld ld_out=%lld)", B, n_max, ld_audio, ld_out);
  DS2_REQUIRE(rir_elems >= 0 && rir_elems <= 0x7fffffffLL, "ds2_reverb_f32: rir_elems = %lld outside [0, 2^31)", rir_elems);
  DS2_REQUIRE(rir || rir_elems == 0, "ds2_reverb_f32: null impulse-response bank of %lld elements", rir_elems);
  DS2_REQUIRE(((uintptr_t)audio & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)rir & 3) == 0 && ((uintptr_t)n_samples_dev & 3) == 0 &&
                  ((uintptr_t)rir_taps_dev & 3) == 0 && ((uintptr_t)rir_base_dev & 7) == 0,
              "ds2_reverb_f32: audio, out, rir, n_samples and rir_taps must be 4-byte aligned, rir_base 8-byte aligned");
  DS2_REQUIRE(out != audio, "ds2_reverb_f32: out must not alias audio");
  if (n_max == 0) return 0;
  const dim3 grid((unsigned)ceil_div(n_max, kRvTile), (unsigned)B);
  hipLaunchKernelGGL(reverb_kernel, grid, dim3(kRvThreads), 0, (hipStream_t)stream, audio, ld_audio, n_samples_dev, rir, rir_elems,
                     rir_base_dev, rir_taps_dev, n_max, out, ld_out);
  DS2_LAUNCH_CHECK("reverb_kernel");
  return 0;
}
