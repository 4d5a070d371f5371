// Pause segmentation of CTC posteriors and the packing of the segments into a decode batch (ds2_ctc_segment_f32,
// ds2_ctc_segment_gather_f32; contracts in include/ds2hip.h, restated by tests/ctc_segment_oracle.py).  Compiled inside decode.hip's
// translation unit.  Integer work on the blank column: nothing here rounds.
//
// Bits kernel: one lane per frame reads x[b][t][blank] and the wave's ballot is one 64-bit word per 64 frames (bit i = frame 64 w + i
// is silent; frames at or beyond T_b are not), four words per workgroup, B * ceil(T / 64) words in all: an hour at B = 1 is 2 813 waves.
// Segment kernel: one workgroup of 256 threads per utterance, on the words alone.
//   1. runs: a thread takes a word; the first frames of the silent runs are v & ~(v << 1 | carry in), the last frames
//      v & ~(v >> 1 | carry in), and the k-th first frame belongs with the k-th last frame: two lists, filled by prefix counts.
//   2. pauses: the runs that are long enough or touch an end, compacted by a prefix count.
//   3. regions: with P pauses the candidates are the P + 1 gaps before, between and behind them (only the first and the last can be
//      empty); a thread takes a gap, pads it from its two pauses and counts its segments: 1, or for a padded region above max_len what
//      the forced cuts give.  Those are rare: the wave that holds such a region walks it with a wave-wide arg-max per cut and leaves the
//      cuts in the workspace, at the region's own frames, which no other region shares.  A prefix count of the segment counts places
//      every region's segments.
// Gather kernel: a workgroup copies 1 024 consecutive floats of a row of out, as 32-bit words; reads are contiguous where ld_t == C.
#pragma once
#ifndef DS2_CTC_SEGMENT_TU
#error "ctc_segment.h is a part of decode.hip"
#endif

namespace {

constexpr int SEG_THREADS = 256;

struct SegArgs {
  const float* x;
  long long ld_b, ld_t;
  int T, W, blank;
  const int* in_lens;
  float thr;
  int min_gap, pad, max_len, max_segs;
  int *seg_start, *seg_end, *seg_flags, *n_segs;
  unsigned long long* words;   // workspace: [B][W]
  int* lists;                  // workspace: [B][4 * (T / 2 + 1) + T]: run starts, run ends, pause starts, pause ends, forced cuts
};

__global__ __launch_bounds__(256) void ctc_segment_bits_kernel(SegArgs a) {
  const int wpb = (a.W + 3) >> 2;                                // workgroups per utterance
  const int b = blockIdx.x / wpb;
  const int w = (blockIdx.x - b * wpb) * 4 + (threadIdx.x >> 6);
  if (w >= a.W) return;
  const int lane = threadIdx.x & 63;
  const int Tb = a.in_lens ? min(max(a.in_lens[b], 0), a.T) : a.T;
  const int t = w * 64 + lane;
  bool silent = false;
  if (t < Tb) silent = a.x[(long long)b * a.ld_b + (long long)t * a.ld_t + a.blank] >= a.thr;
  const unsigned long long m = __ballot(silent);
  if (lane == 0) a.words[(long long)b * a.W + w] = m;
}

// exclusive prefix sum over the workgroup's 256 threads; total: the sum of all of them.  part: 4 ints of LDS.
__device__ __forceinline__ int seg_block_scan(int v, int* part, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) part[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = part[q];
    base += q < wave ? p : 0;
    sum += p;
  }
  __syncthreads();                                               // part is free again
  total = sum;
  return base + inc - v;
}

// The forced cuts of the padded region [s, e), e - s > max_len, by one whole wavefront: the cuts go to cuts[0 ..), their count returns.
// Every frame read lies in [s, e).
__device__ int seg_forced_cuts(const float* xb, long long ld_t, int s, int e, int max_len, int* cuts) {
  const int lane = threadIdx.x & 63;
  const int half = max_len / 2 + (max_len & 1);
  int cur = s, n = 0;
  while (e - cur > max_len) {
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int c = cur + half + lane; c <= cur + max_len; c += 64) {   // ascending c within a lane: a tie keeps the smaller c
      float v = xb[(long long)c * ld_t];
      v = v == v ? v : -INFINITY;                                    // (NaN: unspecified by the contract; an ordered value keeps the lanes agreed)
      if (v > bv || bc == 0x7fffffff) { bv = v; bc = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    if (lane == 0) cuts[n] = bc;
    ++n;
    cur = bc;                                                        // bc >= cur + half > cur: the walk ends
  }
  return n;
}

__global__ __launch_bounds__(SEG_THREADS) void ctc_segment_kernel(SegArgs a) {
  __shared__ int part[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x;
  const int Tb = a.in_lens ? min(max(a.in_lens[b], 0), a.T) : a.T;
  const int W = a.W, R = a.T / 2 + 1;
  const unsigned long long* words = a.words + (long long)b * W;
  int* runA = a.lists + (long long)b * (4LL * R + a.T);
  int *runB = runA + R, *pA = runB + R, *pB = pA + R, *cuts = pB + R;
  // 1. the silent runs
  int nA = 0, nB = 0;
  for (int w0 = 0; w0 < W; w0 += SEG_THREADS) {
    const int w = w0 + tid;
    unsigned long long first = 0, last = 0;
    if (w < W) {
      const unsigned long long v = words[w];
      const unsigned long long prev = w > 0 ? words[w - 1] >> 63 : 0ull;
      const unsigned long long next = w + 1 < W ? words[w + 1] & 1ull : 0ull;
      first = v & ~((v << 1) | prev);
      last = v & ~((v >> 1) | (next << 63));
    }
    int total;                                                       // at most 32 of each per word: 16 bits hold a tile's sum
    const int ex = seg_block_scan(__popcll(first) | (__popcll(last) << 16), part, total);
    int ia = nA + (ex & 0xffff), ib = nB + (ex >> 16);
    for (; first; first &= first - 1) runA[ia++] = w * 64 + __builtin_ctzll(first);
    for (; last; last &= last - 1) runB[ib++] = w * 64 + __builtin_ctzll(last) + 1;
    nA += total & 0xffff;
    nB += total >> 16;
  }
  __syncthreads();
  // 2. the pauses among them
  int P = 0;
  for (int k0 = 0; k0 < nA; k0 += SEG_THREADS) {
    const int k = k0 + tid;
    int ra = 0, rb = 0;
    bool is_pause = false;
    if (k < nA) {
      ra = runA[k];
      rb = runB[k];
      is_pause = rb - ra >= a.min_gap || ra == 0 || rb == Tb;
    }
    int total;
    const int ex = seg_block_scan(is_pause ? 1 : 0, part, total);
    if (is_pause) {
      pA[P + ex] = ra;
      pB[P + ex] = rb;
    }
    P += total;
  }
  __syncthreads();
  // 3. the regions, their padding, their segments
  const float* xb = a.x + (long long)b * a.ld_b + a.blank;
  const long long orow = (long long)b * a.max_segs;
  int n_out = 0;
  for (int g0 = 0; g0 <= P; g0 += SEG_THREADS) {
    const int g = g0 + tid;
    int s = 0, e = 0, cnt = 0;
    if (g <= P) {
      int lo = 0, hi = Tb;
      if (g > 0) {
        const int fa = pA[g - 1], fb = pB[g - 1];
        s = fb;
        lo = fa == 0 ? 0 : fa + (fb - fa) / 2;
      }
      e = Tb;
      if (g < P) {
        const int ba = pA[g], bb = pB[g];
        e = ba;
        hi = bb == Tb ? Tb : ba + (bb - ba) / 2;
      }
      if (s < e) {
        s = max(s - a.pad, lo);
        e = min(e + a.pad, hi);                                      // (pad <= T: the entry clamps it)
        cnt = 1;
      }
    }
    const bool is_long = cnt > 0 && e - s > a.max_len;
    for (unsigned long long m = __ballot(is_long); m; m &= m - 1) {  // the whole wave walks each long region of its 64
      const int src = __builtin_ctzll(m);
      const int ls = __shfl(s, src, 64), le = __shfl(e, src, 64);
      const int n = seg_forced_cuts(xb, a.ld_t, ls, le, a.max_len, cuts + ls);
      if (lane == src) cnt = n + 1;
    }
    int total;
    const int ex = seg_block_scan(cnt, part, total);                 // (its barrier also publishes the cuts)
    long long i = (long long)n_out + ex;
    if (cnt == 1) {
      if (i < a.max_segs) {
        a.seg_start[orow + i] = s;
        a.seg_end[orow + i] = e;
        a.seg_flags[orow + i] = 0;
      }
    } else if (cnt > 1) {
      int cur = s;
      for (int q = 0; q < cnt && i < a.max_segs; ++q, ++i) {
        const int nxt = q + 1 < cnt ? cuts[s + q] : e;
        a.seg_start[orow + i] = cur;
        a.seg_end[orow + i] = nxt;
        a.seg_flags[orow + i] = (q > 0 ? 1 : 0) | (q + 1 < cnt ? 2 : 0);
        cur = nxt;
      }
    }
    n_out += total;
  }
  for (int i = min(n_out, a.max_segs) + tid; i < a.max_segs; i += SEG_THREADS) {
    a.seg_start[orow + i] = -1;
    a.seg_end[orow + i] = -1;
    a.seg_flags[orow + i] = 0;
  }
  if (tid == 0) a.n_segs[b] = n_out;
}

constexpr int GATHER_CHUNK = 1024;                                   // floats of one out row per workgroup

__global__ __launch_bounds__(256) void ctc_segment_gather_kernel(const unsigned* __restrict__ x, long long ld_b, long long ld_t, int B, int T,
                                                                 int C, const int* __restrict__ seg_b, const int* __restrict__ seg_start,
                                                                 const int* __restrict__ seg_len, int T_max, int chunks,
                                                                 unsigned* __restrict__ out, int* __restrict__ out_sizes) {
  const int s = blockIdx.x / chunks, chunk = blockIdx.x - s * chunks;
  const int sb = seg_b[s], st = seg_start[s];
  int len = seg_len[s];
  if (sb < 0 || sb >= B || st < 0 || len < 0 || (long long)st + len > T || len > T_max) len = 0;
  if (chunk == 0 && threadIdx.x == 0) out_sizes[s] = len;
  const long long row = (long long)T_max * C, live = (long long)len * C;
  const unsigned* src = x + (len > 0 ? (long long)sb * ld_b + (long long)st * ld_t : 0);
  unsigned* dst = out + (long long)s * row;
#pragma unroll
  for (int q = 0; q < GATHER_CHUNK / 256; ++q) {
    const long long i = (long long)chunk * GATHER_CHUNK + q * 256 + threadIdx.x;
    if (i >= row) break;
    unsigned v = 0;
    if (i < live) {
      const long long t = i / C;
      v = src[t * ld_t + (i - t * C)];
    }
    dst[i] = v;
  }
}

}  // namespace

extern "C" size_t ds2_ctc_segment_workspace_bytes(int B, int T) {
  if (B <= 0 || T <= 0) return 0;
  const size_t W = ((size_t)T + 63) / 64, R = (size_t)T / 2 + 1;
  return (size_t)B * (8 * W + 4 * (4 * R + (size_t)T));
}

extern "C" int ds2_ctc_segment_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, const int* in_lens_dev, int blank,
                                   float thr, int min_gap, int pad, int max_len, int max_segs, int* seg_start, int* seg_end, int* seg_flags,
                                   int* n_segs, void* ws, size_t ws_bytes, void* stream) {
  DS2_REQUIRE(x && seg_start && seg_end && seg_flags && n_segs, "ds2_ctc_segment_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && C > 0 && ld_b > 0 && ld_t > 0, "ds2_ctc_segment_f32: bad dims (B=%d T=%d C=%d)", B, T, C);
  DS2_REQUIRE(blank >= 0 && blank < C, "ds2_ctc_segment_f32: blank must lie in [0, C), got %d", blank);
  DS2_REQUIRE(min_gap >= 1, "ds2_ctc_segment_f32: min_gap must be at least 1, got %d", min_gap);
  DS2_REQUIRE(pad >= 0, "ds2_ctc_segment_f32: pad must not be negative, got %d", pad);
  DS2_REQUIRE(max_len >= 2, "ds2_ctc_segment_f32: max_len must be at least 2, got %d", max_len);
  DS2_REQUIRE(max_segs >= 1, "ds2_ctc_segment_f32: max_segs must be at least 1, got %d", max_segs);
  const int W = (int)(((long long)T + 63) / 64);
  const long long bits_grid = (long long)B * ((W + 3) / 4);
  DS2_REQUIRE(bits_grid <= 0x7fffffffLL, "ds2_ctc_segment_f32: B * T too large for one launch (B=%d T=%d)", B, T);
  DS2_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= ds2_ctc_segment_workspace_bytes(B, T),
              "ds2_ctc_segment_f32: workspace too small (or not 8-byte aligned)");
  unsigned long long* words = (unsigned long long*)ws;
  SegArgs a{x, ld_b, ld_t, T, W, blank, in_lens_dev, thr, min_gap, pad < T ? pad : T, max_len, max_segs, seg_start, seg_end, seg_flags, n_segs,
            words, (int*)(words + (size_t)B * (size_t)W)};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ctc_segment_bits_kernel, dim3((unsigned)bits_grid), dim3(256), 0, s, a);
  DS2_LAUNCH_CHECK("ctc_segment_bits_kernel");
  hipLaunchKernelGGL(ctc_segment_kernel, dim3((unsigned)B), dim3(SEG_THREADS), 0, s, a);
  DS2_LAUNCH_CHECK("ctc_segment_kernel");
  return 0;
}

extern "C" int ds2_ctc_segment_gather_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, const int* seg_b_dev,
                                          const int* seg_start_dev, const int* seg_len_dev, int S, int T_max, float* out, int* out_sizes,
                                          void* stream) {
  DS2_REQUIRE(x && seg_b_dev && seg_start_dev && seg_len_dev && out && out_sizes, "ds2_ctc_segment_gather_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && C > 0 && ld_b > 0 && ld_t > 0, "ds2_ctc_segment_gather_f32: bad dims (B=%d T=%d C=%d)", B, T, C);
  DS2_REQUIRE(S > 0 && T_max > 0, "ds2_ctc_segment_gather_f32: S and T_max must be positive (S=%d T_max=%d)", S, T_max);
  const long long chunks = ((long long)T_max * C + GATHER_CHUNK - 1) / GATHER_CHUNK;
  DS2_REQUIRE(chunks * S <= 0x7fffffffLL, "ds2_ctc_segment_gather_f32: S * T_max * C too large for one launch");
  hipLaunchKernelGGL(ctc_segment_gather_kernel, dim3((unsigned)(chunks * S)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)x, ld_b,
                     ld_t, B, T, C, seg_b_dev, seg_start_dev, seg_len_dev, T_max, (int)chunks, (unsigned*)out, out_sizes);
  DS2_LAUNCH_CHECK("ctc_segment_gather_kernel");
  return 0;
}
