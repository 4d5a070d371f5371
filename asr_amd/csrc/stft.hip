// Spectrogram front-end on the GPU: the step before the train path.
// Replaces SpectrogramParser.parse_audio's arithmetic (asr_deepspeech/data/parsers/spectrogram_parser.py:45-60):
//     D = librosa.stft(y, n_fft, hop_length, win_length=n_fft, window)      (centred frames)
//     spect = log1p(|D|) ; optional (spect - mean) / std (unbiased, over the whole utterance)
// for a whole batch of waveforms at once, writing the (B,1,n_bins,T) zero-padded layout _collate_fn builds
// (functional.py:18-30).  librosa (0.11.0 in the reference's uv.lock) is a third-party dependency that is not in the
// reference tree; its published algorithm is restated: pad n_fft/2 on both sides (zeros = librosa >= 0.10 default, or
// reflect), frame t = padded[t*hop : t*hop + n_fft] * window, one-sided DFT, frames = 1 + n_samples / hop.
//
// Mapping: n_fft = 320 is not a power of two and tiny, so the DFT is a GEMM on the f32 matrix cores: all frames of all
// utterances are the rows of ONE (B*R, n_fft) operand with row pitch = hop — overlapping rows, no frame copy — times the
// window-folded basis (n_fft, 2*n_bins).  Around it: one padding pass, one LDS-tiled magnitude/log1p/transpose pass that
// also produces the per-utterance sums, and one normalisation pass.  HBM: ~2 x 82 MB at B=64 x 10 s; 13 GFLOP.
#include "common.h"

namespace {

// noise bank of the augmented front-end: utterance b mixes noise[base_b + (s_b + j) mod L_b] scaled by gain_b (0 = no noise)
struct AugNoise {
  const float* noise;
  const long long* base;
  const int* period;
  const int* start;
  const float* gain;
};

// ypad[b*R*hop + i] = padded waveform of utterance b (i in [0, R*hop)), zero beyond n_b + 2*half.
// Reflect padding follows np.pad(mode="reflect") (what librosa.stft calls) for every n >= 1: the index is folded into [0, 2(n-1)) and the
// upper half mirrored, so an utterance of n <= n_fft/2 samples is reflected as often as the pad needs.  For n > n_fft/2 one reflection
// lands inside the signal (-j <= half <= n-1, 2(n-1)-j >= n-1-half >= 0) and the fold picks that same sample: same bits as the
// one-reflection rule this replaced; zero padding does not pass through the fold at all.
// MIX: the padded signal is that of the mixed waveform x[j] + gain_b * noise_seg[j], read at the already reflected index j.
template <bool MIX>
__global__ __launch_bounds__(256) void stft_pad_kernel(const float* __restrict__ audio, long long ld_audio, const int* __restrict__ n_samples,
                                                       float* __restrict__ ypad, int Bn, long long row_len, int half, int reflect, long long total,
                                                       AugNoise nz) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    float v = 0.f;
    const long long b = i / row_len;
    if (b < Bn) {
      const int n = n_samples[b];
      long long j = i - b * row_len - half;            // index into the un-padded waveform
      if (j >= -(long long)half && j < (long long)n + half && n > 0) {
        if (j < 0 || j >= n) {
          if (!reflect) j = -1;
          else {
            const long long P = 2LL * (n - 1);         // numpy's reflect: mirror-periodic with period 2(n-1); n == 1: every index is sample 0
            j = P > 0 ? j % P : 0;
            if (j < 0) j += P;
            if (j >= n) j = P - j;
          }
        }
        if (j >= 0) {
          v = audio[b * ld_audio + j];
          if constexpr (MIX) {
            const float g = nz.gain[b];
            if (g != 0.f) {                            // (gain_b != 0 only for a validated noise segment, see aug_gain_kernel)
              const int L = nz.period[b];
              long long q = (long long)nz.start[b] + j;
              if (q >= L) q %= L;
              v += g * nz.noise[nz.base[b] + q];
            }
          }
        }
      }
    }
    ypad[i] = v;
  }
}

// SpecAugment masks of the augmented front-end: per utterance up to kMaxMasks [lo, hi) bin ranges and [lo, hi) frame ranges
constexpr int kMaxMasks = 8;
struct AugMasks {
  const int* freq;   // (B, nf, 2)
  const int* time;   // (B, nt, 2)
  int nf, nt;
};
// one utterance's ranges held in registers (unused slots are empty ranges); the loops are unrolled so the arrays never go to scratch
struct MaskRegs {
  int flo[kMaxMasks], fhi[kMaxMasks], tlo[kMaxMasks], thi[kMaxMasks];
  __device__ __forceinline__ void load(const AugMasks& m, int b) {
#pragma unroll
    for (int i = 0; i < kMaxMasks; ++i) {
      const bool f = i < m.nf, t = i < m.nt;
      flo[i] = f ? m.freq[((long long)b * m.nf + i) * 2] : 0;
      fhi[i] = f ? m.freq[((long long)b * m.nf + i) * 2 + 1] : 0;
      tlo[i] = t ? m.time[((long long)b * m.nt + i) * 2] : 0;
      thi[i] = t ? m.time[((long long)b * m.nt + i) * 2 + 1] : 0;
    }
  }
  __device__ __forceinline__ bool hit(int k, int t) const {
    bool z = false;
#pragma unroll
    for (int i = 0; i < kMaxMasks; ++i) z |= (k >= flo[i] && k < fhi[i]) || (t >= tlo[i] && t < thi[i]);
    return z;
  }
};

// C (B*R, 2*nb) [re, im interleaved per bin] -> out (B, nb, T) = log1p(sqrt(re^2 + im^2)) for t < frames_b else 0 ;
// part[b][blk][2] = (sum, sum of squares) over the valid elements of this block's tile.   block = 64 frames x 32 bins.
// MASK: elements inside a mask (t < frames_b) are stored as 0; the partial sums are those of the unmasked spectrogram.
template <bool MASK>
__global__ __launch_bounds__(256) void stft_post_kernel(const float* __restrict__ C, int ldc, int R, int nb, int T, int hop,
                                                        const int* __restrict__ n_samples, float* __restrict__ out, float* __restrict__ part,
                                                        AugMasks mk) {
  __shared__ float tile[64][33];
  __shared__ float red[2][4];
  const int b = blockIdx.z, t0 = blockIdx.x * 64, k0 = blockIdx.y * 32;
  const int n = n_samples[b];
  const int frames = n > 0 ? min(T, 1 + n / hop) : 0;
  const int tid = threadIdx.x;
  float s = 0.f, s2 = 0.f;
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int tl = pass * 8 + (tid >> 5), kl = tid & 31;
    const int t = t0 + tl, k = k0 + kl;
    float v = 0.f;
    if (t < frames && k < nb) {
      const float2 z = *reinterpret_cast<const float2*>(C + ((long long)b * R + t) * ldc + 2 * k);
      v = log1pf(sqrtf(z.x * z.x + z.y * z.y));
      s += v;
      s2 += v * v;
    }
    tile[tl][kl] = v;
  }
  __syncthreads();
  MaskRegs mr;
  if constexpr (MASK) mr.load(mk, b);
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int kl = pass * 4 + (tid >> 6), tl = tid & 63;
    const int t = t0 + tl, k = k0 + kl;
    if constexpr (MASK) {
      if (t < T && k < nb) out[((long long)b * nb + k) * T + t] = (t < frames && mr.hit(k, t)) ? 0.f : tile[tl][kl];
    } else {
      if (t < T && k < nb) out[((long long)b * nb + k) * T + t] = tile[tl][kl];
    }
  }
  s = wave_sum(s);
  s2 = wave_sum(s2);
  if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = s2; }
  __syncthreads();
  if (tid == 0) {
    const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    float* p = part + ((long long)b * gridDim.x * gridDim.y + blk) * 2;
    p[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    p[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// per utterance: mean and 1/std (unbiased) from the block partials, combined in fp64
__global__ void stft_stats_kernel(const float* __restrict__ part, int nblk, int nb, int T, int hop, const int* __restrict__ n_samples,
                                  float* __restrict__ stats) {
  const int b = blockIdx.x;
  __shared__ double sh[2][64];
  double s = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    s += (double)part[((long long)b * nblk + i) * 2];
    s2 += (double)part[((long long)b * nblk + i) * 2 + 1];
  }
  sh[0][threadIdx.x] = s;
  sh[1][threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0.0; s2 = 0.0;
    for (int i = 0; i < 64; ++i) { s += sh[0][i]; s2 += sh[1][i]; }
    const int n = n_samples[b];
    const double cnt = n > 0 ? (double)nb * (double)min(T, 1 + n / hop) : 0.0;
    const double mean = cnt > 0 ? s / cnt : 0.0;
    const double var = cnt > 1 ? fmax(s2 - cnt * mean * mean, 0.0) / (cnt - 1.0) : 0.0;
    stats[2 * b] = (float)mean;
    stats[2 * b + 1] = var > 0 ? (float)(1.0 / sqrt(var)) : 0.f;
  }
}

// out[b][k][t] = (out - mean_b) * rstd_b for t < frames_b (padding stays 0: _collate_fn pads AFTER normalisation)
// MASK: SpecAugment after normalisation — elements inside a mask are stored as 0 (the statistics are those of the unmasked spectrogram)
template <bool MASK>
__global__ __launch_bounds__(256) void stft_normalize_kernel(float* __restrict__ out, int nb, int T, int hop, const int* __restrict__ n_samples,
                                                             const float* __restrict__ stats, long long total, AugMasks mk) {
  MaskRegs mr;
  int cur = -1;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const int b = (int)(i / ((long long)nb * T));
    const int n = n_samples[b];
    const int frames = n > 0 ? min(T, 1 + n / hop) : 0;
    if constexpr (MASK) {
      if (t < frames) {
        if (b != cur) { mr.load(mk, b); cur = b; }   // a thread's stride crosses an utterance boundary rarely
        const int k = (int)((i / T) % nb);
        out[i] = mr.hit(k, t) ? 0.f : (out[i] - stats[2 * b]) * stats[2 * b + 1];
      }
    } else {
      if (t < frames) out[i] = (out[i] - stats[2 * b]) * stats[2 * b + 1];
    }
  }
}

// Noise-injection energy pass, stage 1: per (utterance b, block) fp32 partials of sum x^2 and sum noise_seg^2 over j in [0, n_b) —
// grid (kAugEnergyBlocks, B), block-strided, fixed order (no atomics).  Utterances without a valid noise segment write zeros.
constexpr int kAugEnergyBlocks = 32;
__device__ __forceinline__ bool aug_segment_ok(const AugNoise& nz, long long noise_len, int b, float level) {
  const long long base = nz.base[b];
  const int L = nz.period[b], s = nz.start[b];
  return level != 0.f && L > 0 && s >= 0 && s < L && base >= 0 && base + L <= noise_len;
}

__global__ __launch_bounds__(256) void aug_energy_kernel(const float* __restrict__ audio, long long ld_audio, const int* __restrict__ n_samples,
                                                         AugNoise nz, const float* __restrict__ level, long long noise_len, float* __restrict__ part) {
  __shared__ float red[2][4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = n_samples[b];
  float sx = 0.f, sn = 0.f;
  if (n > 0 && aug_segment_ok(nz, noise_len, b, level[b])) {
    const int L = nz.period[b];
    const long long s = nz.start[b];
    const float* x = audio + (long long)b * ld_audio;
    const float* w = nz.noise + nz.base[b];
    for (long long j = (long long)blockIdx.x * 256 + tid; j < n; j += (long long)gridDim.x * 256) {
      long long q = s + j;
      if (q >= L) q %= L;
      const float a = x[j], c = w[q];
      sx += a * a;
      sn += c * c;
    }
  }
  sx = wave_sum(sx);
  sn = wave_sum(sn);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sx; red[1][tid >> 6] = sn; }
  __syncthreads();
  if (tid == 0) {
    float* p = part + ((long long)b * gridDim.x + blockIdx.x) * 2;
    p[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    p[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// stage 2, one 64-thread block per utterance: partials combined in fp64 ->
// gain_b = level_b * rms(x) / rms(noise_seg) = level_b * sqrt(sum x^2 / sum noise_seg^2), 0 = unmixed (no noise, or a silent segment)
__global__ void aug_gain_kernel(const float* __restrict__ part, int nblk, const int* __restrict__ n_samples, AugNoise nz,
                                const float* __restrict__ level, long long noise_len, float* __restrict__ gain) {
  const int b = blockIdx.x;
  __shared__ double sh[2][64];
  double sx = 0.0, sn = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    sx += (double)part[((long long)b * nblk + i) * 2];
    sn += (double)part[((long long)b * nblk + i) * 2 + 1];
  }
  sh[0][threadIdx.x] = sx;
  sh[1][threadIdx.x] = sn;
  __syncthreads();
  if (threadIdx.x == 0) {
    sx = 0.0; sn = 0.0;
    for (int i = 0; i < 64; ++i) { sx += sh[0][i]; sn += sh[1][i]; }
    const float lv = level[b];
    const bool on = n_samples[b] > 0 && aug_segment_ok(nz, noise_len, b, lv) && sn > 0.0;
    gain[b] = on ? (float)((double)lv * sqrt(sx / sn)) : 0.f;
  }
}

inline int rows_per_utt(int T, int n_fft, int hop) { return T + ceil_div(n_fft, hop) - 1; }

}  // namespace

// frames an utterance of n samples produces (librosa centred STFT): 1 + n / hop
extern "C" int ds2_spectrogram_frames(int n_samples, int hop) { return n_samples > 0 ? 1 + n_samples / hop : 0; }

extern "C" size_t ds2_spectrogram_workspace_bytes(int B, int T, int n_fft, int hop) {
  const size_t R = (size_t)rows_per_utt(T, n_fft, hop);
  const size_t nb = (size_t)n_fft / 2 + 1;
  const size_t ypad = align_up(((size_t)B * R * hop + n_fft) * sizeof(float), 256);
  const size_t c = align_up((size_t)B * R * 2 * nb * sizeof(float), 256);
  const size_t part = align_up((size_t)B * ceil_div(T, 64) * ceil_div((int)nb, 32) * 2 * sizeof(float), 256);
  return ypad + c + part + align_up((size_t)B * 2 * sizeof(float), 256);
}

// + the noise energy partials (B, kAugEnergyBlocks, 2) and the per-utterance gains (B)
extern "C" size_t ds2_spectrogram_aug_workspace_bytes(int B, int T, int n_fft, int hop) {
  return ds2_spectrogram_workspace_bytes(B, T, n_fft, hop) + align_up((size_t)B * kAugEnergyBlocks * 2 * sizeof(float), 256) +
         align_up((size_t)B * sizeof(float), 256);
}

namespace {

// Both entry points.  aug == nullptr: the plain front-end (the <false> kernel instances, launched exactly as before the augmented variant
// existed).  Otherwise: noise energy + gain (when aug->level), the mix inside the pad pass, the masks inside the last pass.
struct AugArgs {
  AugNoise nz;
  const float* level;
  long long noise_len;
  AugMasks mk;
};

int spectrogram_impl(const float* audio, long long ld_audio, const int* n_samples_dev, int B, int T, int n_fft, int hop, const float* basis,
                     int pad_mode, int normalize, float* out, void* ws, const AugArgs* aug, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int R = rows_per_utt(T, n_fft, hop), nb = n_fft / 2 + 1;
  const long long row_len = (long long)R * hop;
  const long long ypad_n = (long long)B * row_len + n_fft;
  char* w = (char*)ws;
  float* ypad = (float*)w;                 w += align_up((size_t)ypad_n * sizeof(float), 256);
  float* C = (float*)w;                    w += align_up((size_t)B * R * 2 * nb * sizeof(float), 256);
  float* part = (float*)w;                 w += align_up((size_t)B * ceil_div(T, 64) * ceil_div(nb, 32) * 2 * sizeof(float), 256);
  float* stats = (float*)w;                w += align_up((size_t)B * 2 * sizeof(float), 256);
  float* epart = (float*)w;                w += align_up((size_t)B * kAugEnergyBlocks * 2 * sizeof(float), 256);
  float* gain = (float*)w;
  const bool mix = aug && aug->level;
  const bool mask = aug && (aug->mk.nf > 0 || aug->mk.nt > 0);
  AugNoise nz{};
  if (mix) {
    nz = aug->nz;
    nz.gain = gain;
    hipLaunchKernelGGL(aug_energy_kernel, dim3(kAugEnergyBlocks, B), dim3(256), 0, s, audio, ld_audio, n_samples_dev, nz, aug->level,
                       aug->noise_len, epart);
    DS2_LAUNCH_CHECK("aug_energy_kernel");
    hipLaunchKernelGGL(aug_gain_kernel, dim3(B), dim3(64), 0, s, (const float*)epart, kAugEnergyBlocks, n_samples_dev, nz, aug->level,
                       aug->noise_len, gain);
    DS2_LAUNCH_CHECK("aug_gain_kernel");
  }
  const AugMasks mk = mask ? aug->mk : AugMasks{};
  int blocks = (int)((ypad_n + 255) / 256);
  if (blocks > 16384) blocks = 16384;
  if (mix)
    hipLaunchKernelGGL(stft_pad_kernel<true>, dim3(blocks), dim3(256), 0, s, audio, ld_audio, n_samples_dev, ypad, B, row_len, n_fft / 2,
                       pad_mode, ypad_n, nz);
  else
    hipLaunchKernelGGL(stft_pad_kernel<false>, dim3(blocks), dim3(256), 0, s, audio, ld_audio, n_samples_dev, ypad, B, row_len, n_fft / 2,
                       pad_mode, ypad_n, nz);
  DS2_LAUNCH_CHECK("stft_pad_kernel");
  // every frame of every utterance is a row of ONE operand with pitch = hop (rows overlap): C = frames x basis
  int rc = ds2_gemm_f32(0, 0, B * R, 2 * nb, n_fft, ypad, hop, 0, basis, 2 * nb, 0, C, 2 * nb, 0, nullptr, 0, 1, 1, nullptr, 0, stream);
  if (rc) return rc;
  dim3 grid(ceil_div(T, 64), ceil_div(nb, 32), B);
  if (mask && !normalize)                                  // masks go into the LAST pass: here, or the normalisation below
    hipLaunchKernelGGL(stft_post_kernel<true>, grid, dim3(256), 0, s, (const float*)C, 2 * nb, R, nb, T, hop, n_samples_dev, out, part, mk);
  else
    hipLaunchKernelGGL(stft_post_kernel<false>, grid, dim3(256), 0, s, (const float*)C, 2 * nb, R, nb, T, hop, n_samples_dev, out, part, mk);
  DS2_LAUNCH_CHECK("stft_post_kernel");
  if (normalize) {
    hipLaunchKernelGGL(stft_stats_kernel, dim3(B), dim3(64), 0, s, (const float*)part, (int)(grid.x * grid.y), nb, T, hop, n_samples_dev, stats);
    DS2_LAUNCH_CHECK("stft_stats_kernel");
    const long long total = (long long)B * nb * T;
    int nblk = (int)((total + 255) / 256);
    if (nblk > 16384) nblk = 16384;
    if (mask)
      hipLaunchKernelGGL(stft_normalize_kernel<true>, dim3(nblk), dim3(256), 0, s, out, nb, T, hop, n_samples_dev, (const float*)stats, total, mk);
    else
      hipLaunchKernelGGL(stft_normalize_kernel<false>, dim3(nblk), dim3(256), 0, s, out, nb, T, hop, n_samples_dev, (const float*)stats, total, mk);
    DS2_LAUNCH_CHECK("stft_normalize_kernel");
  }
  return 0;
}

}  // namespace

//   audio      (B, ld_audio) fp32 waveforms on the device, n_samples_dev (B) int32 valid samples per row
//   basis      (n_fft, 2*n_bins) fp32, basis[k][2j] = w[k] cos(2 pi k j / n_fft), basis[k][2j+1] = -w[k] sin(2 pi k j / n_fft)
//   out        (B, n_bins, T) fp32 (= (B,1,n_bins,T)); T >= max frames; frames beyond each utterance's own are 0
//   pad_mode   0 = zeros (librosa >= 0.10 default), 1 = reflect ; normalize 0 | 1
extern "C" int ds2_spectrogram_f32(const float* audio, long long ld_audio, const int* n_samples_dev, int B, int T, int n_fft, int hop,
                                   const float* basis, int pad_mode, int normalize, float* out, void* ws, size_t ws_bytes, void* stream) {
  DS2_REQUIRE(audio && n_samples_dev && basis && out && ws, "ds2_spectrogram_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && n_fft >= 4 && (n_fft % 2) == 0 && hop > 0 && (hop % 4) == 0 && hop <= n_fft,
              "ds2_spectrogram_f32: bad dims (B=%d T=%d n_fft=%d hop=%d; hop must be a multiple of 4)", B, T, n_fft, hop);
  DS2_REQUIRE(ws_bytes >= ds2_spectrogram_workspace_bytes(B, T, n_fft, hop), "ds2_spectrogram_f32: workspace too small");
  return spectrogram_impl(audio, ld_audio, n_samples_dev, B, T, n_fft, hop, basis, pad_mode, normalize, out, ws, nullptr, stream);
}

// The augmented front-end (noise injection before the STFT, SpecAugment masks after the statistics); see include/ds2hip.h.
//   noise        (noise_len) fp32 device noise bank; noise_base (B) int64, noise_period (B) / noise_start (B) int32, noise_level (B) fp32:
//                utterance b mixes noise[noise_base[b] + (noise_start[b] + j) mod noise_period[b]]; level 0 = no noise.  The four arrays
//                are NULL together (no noise at all).
//   freq_masks   (B, n_freq_masks, 2) int32 [lo, hi) bin ranges, time_masks (B, n_time_masks, 2) int32 [lo, hi) frame ranges (NULL if 0)
extern "C" int ds2_spectrogram_aug_f32(const float* audio, long long ld_audio, const int* n_samples_dev, int B, int T, int n_fft, int hop,
                                       const float* basis, int pad_mode, int normalize, const float* noise, long long noise_len,
                                       const long long* noise_base, const int* noise_period, const int* noise_start, const float* noise_level,
                                       const int* freq_masks, int n_freq_masks, const int* time_masks, int n_time_masks, float* out, void* ws,
                                       size_t ws_bytes, void* stream) {
  DS2_REQUIRE(audio && n_samples_dev && basis && out && ws, "ds2_spectrogram_aug_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && n_fft >= 4 && (n_fft % 2) == 0 && hop > 0 && (hop % 4) == 0 && hop <= n_fft,
              "ds2_spectrogram_aug_f32: bad dims (B=%d T=%d n_fft=%d hop=%d; hop must be a multiple of 4)", B, T, n_fft, hop);
  DS2_REQUIRE(ws_bytes >= ds2_spectrogram_aug_workspace_bytes(B, T, n_fft, hop), "ds2_spectrogram_aug_f32: workspace too small");
  const bool any_noise = noise_base || noise_period || noise_start || noise_level;
  DS2_REQUIRE(!any_noise || (noise_base && noise_period && noise_start && noise_level && noise && noise_len > 0),
              "ds2_spectrogram_aug_f32: the noise bank (noise, noise_len > 0) and all four per-utterance noise arrays go together");
  DS2_REQUIRE(n_freq_masks >= 0 && n_freq_masks <= kMaxMasks && n_time_masks >= 0 && n_time_masks <= kMaxMasks,
              "ds2_spectrogram_aug_f32: %d frequency / %d time masks per utterance (at most %d of each)", n_freq_masks, n_time_masks, kMaxMasks);
  DS2_REQUIRE((n_freq_masks == 0 || freq_masks) && (n_time_masks == 0 || time_masks), "ds2_spectrogram_aug_f32: null mask array");
  AugArgs a{};
  a.nz = AugNoise{noise, noise_base, noise_period, noise_start, nullptr};
  a.level = any_noise ? noise_level : nullptr;
  a.noise_len = noise_len;
  a.mk = AugMasks{freq_masks, time_masks, n_freq_masks, n_time_masks};
  return spectrogram_impl(audio, ld_audio, n_samples_dev, B, T, n_fft, hop, basis, pad_mode, normalize, out, ws, &a, stream);
}

// ---- packed waveform feed: unpack -----------------------------------------------------------------------------------------------
// A ragged batch of waveforms -> the zero-padded (B, n_max) fp32 batch the kernels above (and tempo.hip's) read: the device half of the
// pipelined waveform feed (asr_amd.data, get_loader(front_end="gpu", prefetch=N)).  The host sends ONE packed buffer per batch — raw
// 16-bit PCM when every file is 16-bit mono, fp32 otherwise — and this pass does what the host did with B slice copies into a
// pageable torch.zeros(B, n_max): scale (int16 * 2^-15, exact: the bits of `astype(float32) / 32768`), permute rows, zero the padding.
//
// Mapping: one thread per 8 output samples of one row.  Every utterance starts at a multiple of 8 elements of a 16-byte-aligned
// buffer, so the 8 source samples are one 128-bit load (int16) or two (fp32); the row pitch of `out` is arbitrary (the front-end's
// batches have ld = n_max), so the two 128-bit stores are only 4-byte aligned, which global memory allows.  One pass, no LDS, no
// atomics: reruns are bit-identical.  The kernels above are untouched.
namespace {

typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));      // a 128-bit store at any 4-byte boundary

constexpr int kUnpackThreads = 256;
constexpr int kChunk = 8;
constexpr int kTagI16 = 0, kTagF32 = 1;                 // the dtype tag of the C ABI

// A row whose description is outside the contract is written as zeros: nothing is ever read outside [0, packed_elems).  The host
// wrapper rejects such descriptions before the launch (ops.wave_unpack); this is the second line.
template <bool I16>
__global__ __launch_bounds__(kUnpackThreads) void wave_unpack_kernel(const void* __restrict__ packed, long long packed_elems,
                                                                     const int* __restrict__ offsets, const int* __restrict__ lengths,
                                                                     const int* __restrict__ src_index, int B, int n_max,
                                                                     float* __restrict__ out, long long ld_out) {
  const int b = blockIdx.y;
  const int j0 = (blockIdx.x * kUnpackThreads + threadIdx.x) * kChunk;
  if (j0 >= n_max) return;
  const int src = src_index[b];
  int off = 0, len = 0;
  if (src >= 0 && src < B) {
    off = offsets[src], len = lengths[src];
    const long long end = (long long)off + (((long long)len + kChunk - 1) & ~(long long)(kChunk - 1));
    if (off < 0 || (off & (kChunk - 1)) || len < 0 || end > packed_elems) len = 0;
    len = min(len, n_max);
  }
  float v[kChunk];
#pragma unroll
  for (int i = 0; i < kChunk; ++i) v[i] = 0.0f;
  if (j0 < len) {                                      // the whole chunk lies inside the buffer (gaps up to the next multiple of 8 exist)
    if constexpr (I16) {
      const i16x8 s = *reinterpret_cast<const i16x8*>(static_cast<const short*>(packed) + off + j0);
#pragma unroll
      for (int i = 0; i < kChunk; ++i) v[i] = (j0 + i < len) ? (float)s[i] * 0x1p-15f : 0.0f;
    } else {
      const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(packed) + off + j0);
      const f32x4 lo = p[0], hi = p[1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = (j0 + i < len) ? lo[i] : 0.0f;
        v[4 + i] = (j0 + 4 + i < len) ? hi[i] : 0.0f;
      }
    }
  }
  float* y = out + (long long)b * ld_out + j0;
  if (j0 + kChunk <= n_max) {
    f32x4_u a, c;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = v[i], c[i] = v[4 + i];
    *reinterpret_cast<f32x4_u*>(y) = a;
    *reinterpret_cast<f32x4_u*>(y + 4) = c;
  } else {
#pragma unroll
    for (int i = 0; i < kChunk; ++i)
      if (j0 + i < n_max) y[i] = v[i];
  }
}

}  // namespace

extern "C" int ds2_wave_unpack_f32(const void* packed, long long packed_elems, int dtype, const int* offsets_dev, const int* lengths_dev,
                                   const int* src_index_dev, int B, int n_max, float* out, long long ld_out, void* stream) {
  DS2_REQUIRE(offsets_dev && lengths_dev && src_index_dev && out, "ds2_wave_unpack_f32: null pointer");
  DS2_REQUIRE(dtype == kTagI16 || dtype == kTagF32, "ds2_wave_unpack_f32: dtype tag %d (0 = int16, 1 = fp32)", dtype);
  DS2_REQUIRE(B > 0 && B <= 65535 && n_max >= 0 && n_max <= (1 << 30) && ld_out >= n_max, "ds2_wave_unpack_f32: bad dims (B=%d n_max=%d ld_out=%lld)", B, n_max, ld_out);
  DS2_REQUIRE(packed_elems >= 0 && packed_elems <= 0x7fffffffLL && packed_elems % kChunk == 0,
              "ds2_wave_unpack_f32: packed_elems = %lld: a multiple of 8 in [0, 2^31)", packed_elems);
  DS2_REQUIRE(packed || packed_elems == 0, "ds2_wave_unpack_f32: null packed buffer of %lld elements", packed_elems);
  DS2_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)out & 3) == 0, "ds2_wave_unpack_f32: packed must be 16-byte aligned, out 4-byte aligned");
  if (n_max == 0) return 0;
  const dim3 grid((unsigned)ceil_div(ceil_div(n_max, kChunk), kUnpackThreads), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == kTagI16)
    hipLaunchKernelGGL(wave_unpack_kernel<true>, grid, dim3(kUnpackThreads), 0, s, packed, packed_elems, offsets_dev, lengths_dev, src_index_dev,
                       B, n_max, out, ld_out);
  else
    hipLaunchKernelGGL(wave_unpack_kernel<false>, grid, dim3(kUnpackThreads), 0, s, packed, packed_elems, offsets_dev, lengths_dev, src_index_dev,
                       B, n_max, out, ld_out);
  DS2_LAUNCH_CHECK("wave_unpack_kernel");
  return 0;
}

// ---- packed waveform feed: unpack with a sample-rate conversion in it (ds2_wave_resample_f32) --------------------------------------
#define DS2_STFT_UNPACK_DEFS 1
#include "resample.h"

// ---- reverberation of the waveform batch (ds2_reverb_f32): built with the feed's other passes ------------------------------------------
#include "reverb.h"
