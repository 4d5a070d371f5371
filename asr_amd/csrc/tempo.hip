// Tempo and gain perturbation of a waveform batch on the GPU: the `speed_volume_perturb` switch of audio_conf.
// Replaces load_randomly_augmented_audio (asr_deepspeech/audio/functional.py:94-104), which starts one `sox ... tempo T gain G`
// process per utterance and reads a temporary WAV back.  sox is a third-party program that is not in the reference tree; what its
// `tempo` effect is published to do — WSOLA, waveform-similarity overlap-add — is restated as the contract in include/ds2hip.h
// (parity with sox itself is unpinned).
//
// Mapping: the only dependence between segments is d_{k-1} -> the tail that segment k is matched against, so the work splits in two:
//   tempo_chain_kernel   one workgroup per utterance walks k = 1 .. K-1.  Both windows a step reads, s[p_k .. p_k + R + O) and
//                        s[p_{k-1} + H .. + R + O), are known before the chain starts: the loads of step k+1 are issued before step k's
//                        R x O integer multiply-adds and land in the other half of a double-buffered LDS window while step k is
//                        reduced, so a step is LDS and ALU only.  Exact integer SSD, arg-min on the packed (SSD, d) key.
//   tempo_synth_kernel   one workgroup per (utterance, segment): cross-fade, copy, gain, clip, zeros up to the row pitch.
// No atomics: reruns are bit-identical.
#include <vector>
#include <math.h>
#include "common.h"

namespace {

constexpr int kChainThreads = 1024;
constexpr int kMaxWindow = 2048;                       // R + O, the samples of one search window
constexpr int kMaxLoads = 2 * kMaxWindow / kChainThreads;
constexpr int kDBits = 12;                             // the arg-min key is SSD << kDBits | d : R <= 4096, SSD <= O * 2^32 < 2^44
constexpr int kMaxSamples = 1 << 29;

struct TempoUtt {      // per utterance, made on the host
  double f;            // tempo factor
  int n, n_out, K;     // input samples, output samples, segments
  float G;             // linear gain
};

struct TempoSizes {
  int S, R, O, H;
};

__host__ __device__ inline int ms_to_samples(int sr, double ms) { return (int)((double)sr * ms / 1000.0 + 0.5); }

// p_k = floor(k * f * H + 0.5) in IEEE double, each operation rounded on its own (contraction into a fused multiply-add is switched
// off: it rounds once where the host rounds twice): the bits of the host's.
__device__ __forceinline__ int nominal_pos(int k, double f, int H) {
#pragma clang fp contract(off)
  const double kf = (double)k * f;
  const double kfh = kf * (double)H;
  return (int)floor(kfh + 0.5);
}

__device__ __forceinline__ float read_x(const float* x, int n, int i) { return (i >= 0 && i < n) ? x[i] : 0.0f; }

// the search signal: the 16-bit sample sox would have been handed (the scaling is exact in fp32; round half to even)
__device__ __forceinline__ int search_sample(float v) { return __float2int_rn(fminf(fmaxf(v * 32768.0f, -32768.0f), 32767.0f)); }

// offsets (B, ld_off) int32: d_0 = 0, d_k for 1 <= k < K_b, 0 for k >= K_b.
__global__ __launch_bounds__(kChainThreads) void tempo_chain_kernel(const float* __restrict__ audio, long long ld_audio,
                                                                    const TempoUtt* __restrict__ utt, TempoSizes sz,
                                                                    int* __restrict__ offsets, int ld_off) {
  __shared__ int win[2][2][kMaxWindow];                // [step parity][0: s[p_k + j] | 1: s[p_{k-1} + H + j]][j]
  __shared__ unsigned long long part[kMaxWindow];      // partial SSDs, [i-chunk][candidate]
  __shared__ unsigned long long red[kChainThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const TempoUtt u = utt[b];
  const float* x = audio + (long long)b * ld_audio;
  int* d_out = offsets + (long long)b * ld_off;
  const int R = sz.R, O = sz.O, H = sz.H, W = R + O, K = u.K;
  for (int k = tid; k < ld_off; k += kChainThreads)
    if (k == 0 || k >= K) d_out[k] = 0;
  if (K < 2) return;
  // candidates padded to whole waves so that an i-chunk is wave-uniform (the tail reads are LDS broadcasts); as many i-chunks as fit
  const int Rr = (R + 63) & ~63;
  const int chunks = Rr >= kChainThreads ? 1 : kChainThreads / Rr;
  const int chunk_len = (O + chunks - 1) / chunks;
  const int items = chunks * Rr;

  // The two windows of step k, one sample per (thread, slot).  The loads are unconditional (clamped address, the value selected when
  // it is used) and converted only in store_loads, so that nothing waits on them between issue and store.
  float regs[kMaxLoads];
  auto issue_loads = [&](int k) {
    const int pk = nominal_pos(k, u.f, H), pb = nominal_pos(k - 1, u.f, H) + H;
#pragma unroll
    for (int l = 0; l < kMaxLoads; ++l) {
      if (l * kChainThreads < 2 * W) {                 // block-uniform
        const int j = tid + l * kChainThreads;
        regs[l] = x[min(max(j < W ? pk + j : pb + (j - W), 0), u.n - 1)];
      }
    }
  };
  auto store_loads = [&](int k, int par) {
    const int pk = nominal_pos(k, u.f, H), pb = nominal_pos(k - 1, u.f, H) + H;
#pragma unroll
    for (int l = 0; l < kMaxLoads; ++l) {
      const int j = tid + l * kChainThreads;
      if (j < 2 * W) {
        const int pos = j < W ? pk + j : pb + (j - W);
        win[par][j < W ? 0 : 1][j < W ? j : j - W] = (pos >= 0 && pos < u.n) ? search_sample(regs[l]) : 0;
      }
    }
  };
  issue_loads(1);
  store_loads(1, 1);
  __syncthreads();
  // this thread's (candidate, i-chunk): with several chunks every thread has at most one, with one chunk the candidates are strided
  const int my_c = chunks == 1 ? tid : tid % Rr, my_ch = chunks == 1 ? 0 : tid / Rr;
  const int i0 = my_ch * chunk_len, i1 = min(O, i0 + chunk_len);
  int d_prev = 0;                                      // q_{k-1} - p_{k-1}
  int my_d = 0;                                        // d_k of the steps k = tid (mod kChainThreads): stored once per kChainThreads steps,
                                                       // a store per step would have the next step's loads queue behind it
  for (int k = 1; k < K; ++k) {
    const int par = k & 1;
    if (k + 1 < K) issue_loads(k + 1);                 // in flight during this step's arithmetic
    const int* cand = win[par][0];
    const int* tail = win[par][1] + d_prev;            // t[i] = s[q_{k-1} + H + i]
    for (int it = tid, c = my_c; it < items; it += kChainThreads, c += kChainThreads) {
      unsigned long long acc = 0;
      if (c < R) {
#pragma unroll 8
        for (int i = i0; i < i1; ++i) {
          const int df = cand[c + i] - tail[i];        // |df| <= 65535: df^2 < 2^32, the product of two 24-bit operands
          const unsigned a = (unsigned)(df < 0 ? -df : df);
          acc += __umul24(a, a);
        }
      }
      part[it] = acc;
    }
    __syncthreads();
    unsigned long long best = ~0ull;                   // min of SSD << kDBits | d : lowest SSD, then lowest d
    for (int c = tid; c < R; c += kChainThreads) {
      unsigned long long ssd = 0;
      for (int ch = 0; ch < chunks; ++ch) ssd += part[ch * Rr + c];
      const unsigned long long key = (ssd << kDBits) | (unsigned)c;
      best = key < best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kChainThreads / 64; ++w) best = red[w] < best ? red[w] : best;
    d_prev = (int)(best & ((1u << kDBits) - 1));
    if ((k & (kChainThreads - 1)) == tid) my_d = d_prev;
    if ((k & (kChainThreads - 1)) == kChainThreads - 1 || k == K - 1) {
      const int kk = (k & ~(kChainThreads - 1)) + tid;
      if (kk >= 1 && kk <= k) d_out[kk] = my_d;
    }
    if (k + 1 < K) store_loads(k + 1, par ^ 1);
    __syncthreads();                                   // the next window is in LDS; part / red may be written again
  }
}

// out (B, ld_out): y[0, n_out) of every utterance, exact zeros in [n_out, ld_out); n_out_dev (B) int32.
__global__ __launch_bounds__(256) void tempo_synth_kernel(const float* __restrict__ audio, long long ld_audio,
                                                          const TempoUtt* __restrict__ utt, TempoSizes sz,
                                                          const int* __restrict__ offsets, int ld_off, float* __restrict__ out,
                                                          long long ld_out, int* __restrict__ n_out_dev) {
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const TempoUtt u = utt[b];
  const float* x = audio + (long long)b * ld_audio;
  float* y = out + (long long)b * ld_out;
  const int O = sz.O, H = sz.H;
  if (k == 0 && tid == 0) n_out_dev[b] = u.n_out;
  int q = 0, q_prev = 0;
  if (k < u.K) {
    q = nominal_pos(k, u.f, H) + offsets[(long long)b * ld_off + k];
    if (k > 0) q_prev = nominal_pos(k - 1, u.f, H) + offsets[(long long)b * ld_off + k - 1];
  }
  const float fO = (float)O;
  for (int i = tid; i < H; i += 256) {
    const long long j = (long long)k * H + i;
    if (j >= ld_out) break;
    float v = 0.0f;
    if (j < u.n_out) {
      v = read_x(x, u.n, q + i);
      if (k > 0 && i < O) {                            // linear cross-fade from what segment k-1 would have played next
        const float a = read_x(x, u.n, q_prev + H + i);
        const float w = ((float)i + 0.5f) / fO;
        const float df = v - a;
        v = df == 0.0f ? a : a + w * df;
      }
      v = fminf(fmaxf(u.G * v, -1.0f), 1.0f);
    }
    y[j] = v;
  }
}

int tempo_sizes(int sr, double seg_ms, double search_ms, double overlap_ms, TempoSizes* out) {
  DS2_REQUIRE(sr > 0 && seg_ms > 0 && search_ms > 0 && overlap_ms > 0 && seg_ms < 1e6 && search_ms < 1e6 && overlap_ms < 1e6 &&
                  (double)sr * seg_ms < 1e12,
              "ds2_tempo: bad sample rate / times (sr=%d segment=%g search=%g overlap=%g ms)", sr, seg_ms, search_ms, overlap_ms);
  TempoSizes z;
  z.S = ms_to_samples(sr, seg_ms), z.R = ms_to_samples(sr, search_ms), z.O = ms_to_samples(sr, overlap_ms);
  z.H = z.S - z.O;
  DS2_REQUIRE(z.S > 2 * z.O && z.R >= 1 && z.O >= 1, "ds2_tempo: segment %d, search %d, overlap %d samples: need S > 2 O, R >= 1, O >= 1",
              z.S, z.R, z.O);
  DS2_REQUIRE(z.R + z.O <= kMaxWindow, "ds2_tempo: search + overlap = %d samples, at most %d", z.R + z.O, kMaxWindow);
  *out = z;
  return 0;
}

}  // namespace

extern "C" int ds2_tempo_sizes(int sample_rate, double segment_ms, double search_ms, double overlap_ms, int* S, int* R, int* O) {
  TempoSizes z;
  if (int rc = tempo_sizes(sample_rate, segment_ms, search_ms, overlap_ms, &z)) return rc;
  if (S) *S = z.S;
  if (R) *R = z.R;
  if (O) *O = z.O;
  return 0;
}

extern "C" int ds2_tempo_out_samples(int n, double f) {
  if (!(n >= 0 && n <= kMaxSamples && f >= 0.5 && f <= 2.0)) return -1;
  return (int)floor((double)n / f + 0.5);
}

extern "C" size_t ds2_tempo_workspace_bytes(int B) { return B > 0 ? align_up((size_t)B * sizeof(TempoUtt), 256) : 0; }

extern "C" int ds2_tempo_gain_f32(const float* audio, long long ld_audio, const int* n_samples, const double* tempo, const float* gain,
                                  int B, int sample_rate, double segment_ms, double search_ms, double overlap_ms, float* out,
                                  long long ld_out, int* n_out_dev, int* offsets_out, int ld_offsets, void* ws, size_t ws_bytes,
                                  void* stream) {
  DS2_REQUIRE(audio && n_samples && tempo && gain && out && n_out_dev && offsets_out && ws, "ds2_tempo_gain_f32: null pointer");
  DS2_REQUIRE(B > 0 && B <= 65535 && ld_audio > 0 && ld_out > 0 && ld_offsets > 0, "ds2_tempo_gain_f32: bad dims (B=%d ld_audio=%lld ld_out=%lld ld_offsets=%d)",
              B, ld_audio, ld_out, ld_offsets);
  DS2_REQUIRE(ws_bytes >= ds2_tempo_workspace_bytes(B), "ds2_tempo_gain_f32: workspace too small");
  TempoSizes z;
  if (int rc = tempo_sizes(sample_rate, segment_ms, search_ms, overlap_ms, &z)) return rc;
  std::vector<TempoUtt> utt(B);
  for (int b = 0; b < B; ++b) {
    const int n_out = ds2_tempo_out_samples(n_samples[b], tempo[b]);
    DS2_REQUIRE(n_out >= 0, "ds2_tempo_gain_f32: utterance %d: n = %d samples (0 .. 2^29), tempo = %g (0.5 .. 2)", b, n_samples[b], tempo[b]);
    DS2_REQUIRE(n_samples[b] <= ld_audio && n_out <= ld_out, "ds2_tempo_gain_f32: utterance %d: %d samples in a row of %lld, %d out in a row of %lld",
                b, n_samples[b], ld_audio, n_out, ld_out);
    DS2_REQUIRE(gain[b] >= 0.0f && gain[b] < INFINITY, "ds2_tempo_gain_f32: utterance %d: linear gain %g", b, (double)gain[b]);
    utt[b].f = tempo[b], utt[b].n = n_samples[b], utt[b].n_out = n_out, utt[b].K = ceil_div(n_out, z.H), utt[b].G = gain[b];
    DS2_REQUIRE(utt[b].K <= ld_offsets, "ds2_tempo_gain_f32: utterance %d has %d segments, offsets_out holds %d per row", b, utt[b].K, ld_offsets);
  }
  const long long synth_blocks = (ld_out + z.H - 1) / z.H;
  DS2_REQUIRE(synth_blocks <= 0x7fffffffLL, "ds2_tempo_gain_f32: ld_out too large");
  hipStream_t s = (hipStream_t)stream;
  // pageable source: the runtime has consumed it when the call returns
  DS2_HIP(hipMemcpyAsync(ws, utt.data(), (size_t)B * sizeof(TempoUtt), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(tempo_chain_kernel, dim3(B), dim3(kChainThreads), 0, s, audio, ld_audio, (const TempoUtt*)ws, z, offsets_out, ld_offsets);
  DS2_LAUNCH_CHECK("tempo_chain_kernel");
  hipLaunchKernelGGL(tempo_synth_kernel, dim3((unsigned)synth_blocks, B), dim3(256), 0, s, audio, ld_audio, (const TempoUtt*)ws, z,
                     (const int*)offsets_out, ld_offsets, out, ld_out, n_out_dev);
  DS2_LAUNCH_CHECK("tempo_synth_kernel");
  return 0;
}
