// Streaming keyword search (ds2_ctc_kws_stream_feed_f32, contract in include/ds2hip.h): the search of ctc_kws.h fed a chunk of frames at
// a time, with detections reported as soon as they can no longer change.  Compiled inside ctc.hip's translation unit, after ctc_kws.h.
//
// Lattice: ctc_kws_wave_kernel<IS_LOG, KwsStreamArgs>, the one-call kernel with the two hooks below.  What the lattice carries from one
// frame to the next is four registers per lane (E, O, sE, sO); stream_load reads them and the frames consumed so far (a state of zero
// bytes: the kernel's own initial values), stream_save writes them back and reduces the horizon over the lanes: the smallest start among
// the states whose value is at or above the threshold.  Emission terms are <= 0, so a state below the threshold stays below it for
// ever, and every candidate of a later feed starts at the horizon or after it.
// Intake, settle and pick: ctc_kws_stream_pick_kernel, one wavefront per (utterance, keyword), on the pending list in the state.
//   intake   the chunk's frames at or above the threshold are appended by ballot and prefix count, ascending t (the list is ascending
//            already: every earlier t is below this chunk's first frame);
//   settle   c starts at max(tail, horizon) and is lowered to the smallest start among the candidates it cuts (start < c <= t) until it
//            cuts none; every round is one scan of the list and takes c to a start of the list, so there are at most as many rounds
//            as candidates.  With max_lag, c is then raised to n - max_lag and what it cuts is dropped;
//   pick     the rounds of ctc_kws_pick_kernel on the list, first among the candidates with t < c (final), then among the rest
//            (tentative).  A kill is the complement of the candidate's start (starts are >= 0), which the compaction undoes for the
//            tentative candidates: they stay pending, and the winner that killed one may itself lose to a later frame;
//   compact  the candidates with t >= c move to the front, in order.
// A lane scans and marks the entries i = l (mod 64) only; the intake, which writes entries from other lanes, is fenced from the scans.
// Every index into the state is clamped to the sizes the launch was given, whatever the blob holds.
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_kws_stream.h is a part of ctc.hip"
#endif

namespace {

constexpr int KWS_MAX_PENDING = 65536;
// one (utterance, keyword) of the state, in int32 words: the header, the four registers of the 64 lanes, the pending list (t | start | score)
enum { KWS_ST_N, KWS_ST_TAIL, KWS_ST_NPEND, KWS_ST_FORCED, KWS_ST_DROPPED, KWS_ST_H, KWS_ST_CHUNK, KWS_ST_LANES = 8, KWS_ST_PEND = 8 + 4 * 64 };

__host__ __device__ inline size_t kws_stream_words(int pending) { return (size_t)KWS_ST_PEND + 3 * (size_t)pending; }

struct KwsStreamArgs : KwsArgs {
  int* state;
  int pending, max_lag, finish;
  int *hit_final, *tail, *frames, *forced, *dropped;   // hit_final [B][K][max_hits], the rest [B][K]

  __device__ int* blob() const { return state + (size_t)blockIdx.x * kws_stream_words(pending); }

  __device__ int stream_load(int l, float& E, float& O, int& sE, int& sO) const {
    const int* st = blob();
    const int n0 = max(__builtin_amdgcn_readfirstlane(st[KWS_ST_N]), 0);
    if (n0 > 0) {
      E = __int_as_float(st[KWS_ST_LANES + l]);
      O = __int_as_float(st[KWS_ST_LANES + 64 + l]);
      sE = st[KWS_ST_LANES + 128 + l];
      sO = st[KWS_ST_LANES + 192 + l];
    }
    return n0;
  }

  __device__ void stream_save(int l, int k, int n0, int Tadv, float E, float O, int sE, int sO) const {
    int* st = blob();
    if (Tadv > 0) {
      st[KWS_ST_LANES + l] = __float_as_int(E);
      st[KWS_ST_LANES + 64 + l] = __float_as_int(O);
      st[KWS_ST_LANES + 128 + l] = sE;
      st[KWS_ST_LANES + 192 + l] = sO;
    }
    const float th = thr[k];
    const int n = n0 + Tadv;
    int h = n;
    if (E > NEG_INF && E >= th) h = min(h, sE);
    if (O > NEG_INF && O >= th) h = min(h, sO);
    for (int o = 32; o > 0; o >>= 1) h = min(h, __shfl_xor(h, o));
    if (l == 0) {
      st[KWS_ST_N] = n;
      st[KWS_ST_H] = h;
      st[KWS_ST_CHUNK] = Tadv;
    }
  }
};

__device__ __forceinline__ int kws_wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(64) void ctc_kws_stream_pick_kernel(KwsStreamArgs a) {
  const int l = threadIdx.x;
  const int k = blockIdx.x % a.K;
  int* st = a.blob();
  int* pt = st + KWS_ST_PEND;
  int* ps = pt + a.pending;
  float* pv = (float*)(ps + a.pending);
  const float thr = a.thr[k];
  const int n = max(st[KWS_ST_N], 0);
  const int chunk = a.T > 0 ? min(max(st[KWS_ST_CHUNK], 0), min(a.T, n)) : 0;   // (T == 0: the lattice kernel did not run)
  const int h = min(max(st[KWS_ST_H], 0), n);
  int tail = min(max(st[KWS_ST_TAIL], 0), n), np = min(max(st[KWS_ST_NPEND], 0), a.pending);
  int forced = st[KWS_ST_FORCED], dropped = st[KWS_ST_DROPPED];

  // intake: the chunk's frames n - chunk .. n - 1
  const long long row = (long long)blockIdx.x * a.T;
  const int n0 = n - chunk;
  for (int i0 = 0; i0 < chunk; i0 += 64) {
    const int i = i0 + l;
    float v = NEG_INF;
    int s = -1;
    bool c = false;
    if (i < chunk) {
      v = a.fscore[row + i];
      s = a.fstart[row + i];
      c = v > NEG_INF && v >= thr;
    }
    const bool late = c && s < tail;                             // its path began before a forced cut
    c = c && !late;
    const unsigned long long m = __ballot(c);
    const int pos = np + __popcll(m & ((1ull << l) - 1ull));
    if (c && pos < a.pending) {
      pt[pos] = n0 + i;
      ps[pos] = s;
      pv[pos] = v;
    }
    const int cnt = __popcll(m), fit = min(cnt, a.pending - np);
    dropped += __popcll(__ballot(late)) + cnt - fit;
    np += fit;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");         // the list is read by other lanes than wrote it
  __builtin_amdgcn_wave_barrier();

  // settle
  int c = n;
  if (!a.finish) {
    c = max(tail, h);
    for (;;) {
      int m = 0x7fffffff;
      for (int i = l; i < np; i += 64) {
        const int s = ps[i];
        if (s < c && c <= pt[i]) m = min(m, s);
      }
      m = kws_wave_min(m);
      if (m == 0x7fffffff) break;
      c = m;                                                     // (m < c: the loop ends)
    }
  }
  if (a.max_lag >= 0 && n - c > a.max_lag) {                     // a forced cut: what it cuts is dropped
    c = n - a.max_lag;
    ++forced;
    for (int i0 = 0; i0 < np; i0 += 64) {
      const int i = i0 + l;
      const bool cut = i < np && ps[i] < c && c <= pt[i];
      if (cut) pt[i] = -1;
      dropped += __popcll(__ballot(cut));
    }
  }

  // pick: phase 0 the candidates with t < c, phase 1 the rest
  const long long hrow = (long long)blockIdx.x * a.max_hits;
  int nh = 0, wt = -1, ws = 0, phase = 0;                        // [ws, wt]: the span of the previous winner (wt < 0: none yet)
  bool over = false;
  for (;;) {
    float bv = NEG_INF;
    int bt = 0x7fffffff, bs = -1;
    for (int i = l; i < np; i += 64) {                           // (a lane reads and kills its own entries only)
      const int t = pt[i], s = ps[i];
      if (t < 0 || s < 0) continue;
      if (wt >= 0 && s <= wt && ws <= t) {
        ps[i] = ~s;
        continue;
      }
      if ((t < c) != (phase == 0)) continue;
      const float v = pv[i];
      if (v > bv) { bv = v; bt = t; bs = s; }                    // ascending t within a lane: a tie keeps the smaller t
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int ot = __shfl_xor(bt, o), os = __shfl_xor(bs, o);
      if (ov > bv || (ov == bv && ot < bt)) { bv = ov; bt = ot; bs = os; }
    }
    if (bt == 0x7fffffff) {                                      // no live candidate on this side of c
      if (phase == 1) break;
      phase = 1;
      continue;
    }
    if (nh == a.max_hits) {                                      // a live candidate beyond the last slot
      over = true;
      break;
    }
    if (l == 0) {
      a.hit_start[hrow + nh] = bs;
      a.hit_end[hrow + nh] = bt + 1;
      a.hit_score[hrow + nh] = bv;
      a.hit_final[hrow + nh] = phase == 0;
    }
    ++nh;
    wt = bt;
    ws = bs;
  }
  for (int i = nh + l; i < a.max_hits; i += 64) {
    a.hit_start[hrow + i] = -1;
    a.hit_end[hrow + i] = -1;
    a.hit_score[hrow + i] = NEG_INF;
    a.hit_final[hrow + i] = 0;
  }

  // compact: the candidates with t >= c stay, their kills undone
  int m = 0;
  for (int i0 = 0; i0 < np; i0 += 64) {
    const int i = i0 + l;
    int t = -1, s = 0;
    float v = 0.f;
    if (i < np) {
      t = pt[i];
      s = ps[i];
      v = pv[i];
    }
    const bool keep = t >= c;                                    // (a dropped candidate has t = -1 < c)
    const unsigned long long mk = __ballot(keep);
    if (keep) {                                                  // (m + the prefix count <= i: behind every entry still to be read)
      const int pos = m + __popcll(mk & ((1ull << l) - 1ull));
      pt[pos] = t;
      ps[pos] = s < 0 ? ~s : s;
      pv[pos] = v;
    }
    m += __popcll(mk);
  }
  if (l == 0) {
    st[KWS_ST_TAIL] = c;
    st[KWS_ST_NPEND] = m;
    st[KWS_ST_FORCED] = forced;
    st[KWS_ST_DROPPED] = dropped;
    a.n_hits[blockIdx.x] = over ? a.max_hits + 1 : nh;
    a.tail[blockIdx.x] = c;
    a.frames[blockIdx.x] = n;
    a.forced[blockIdx.x] = forced;
    a.dropped[blockIdx.x] = dropped;
  }
}

}  // namespace

extern "C" size_t ds2_ctc_kws_stream_state_bytes(int B, int K, int pending) {
  if (B <= 0 || K <= 0 || (long long)B * K > 0x7fffffffLL || pending < 1 || pending > KWS_MAX_PENDING) return 0;
  return (size_t)B * (size_t)K * kws_stream_words(pending) * sizeof(int);
}

extern "C" size_t ds2_ctc_kws_stream_workspace_bytes(int B, int T, int K, int frames_out) {
  if (B <= 0 || T < 0 || K <= 0) return 0;
  return ((size_t)B * (size_t)T + (frames_out ? 0 : 2 * (size_t)B * (size_t)K * (size_t)T)) * sizeof(float);
}

extern "C" int ds2_ctc_kws_stream_feed_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                                           const int* in_lens_dev, const int* kw_labels_dev, const int* kw_off_dev, const int* kw_lens_dev,
                                           int K, int max_kw_len, const float* thr_dev, int max_hits, int max_lag, int finish, int pending,
                                           long long frames_bound, void* state, size_t state_bytes, float* frame_score, int* frame_start,
                                           int* hit_start, int* hit_end, float* hit_score, int* hit_final, int* n_hits, int* tail,
                                           int* frames, int* forced, int* dropped, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "ds2_ctc_kws_stream_feed_f32";
  DS2_REQUIRE(state && kw_off_dev && kw_lens_dev && thr_dev && hit_start && hit_end && hit_score && hit_final && n_hits && tail && frames &&
              forced && dropped && (T == 0 || x), "%s: null pointer", who);
  DS2_REQUIRE((frame_score == nullptr) == (frame_start == nullptr), "%s: frame_score and frame_start are given together or not at all", who);
  DS2_REQUIRE(B > 0 && T >= 0 && C > 0 && K > 0 && (T == 0 || (ld_b > 0 && ld_t > 0)) && (long long)B * K <= 0x7fffffffLL,
              "%s: bad dims (B=%d T=%d C=%d K=%d)", who, B, T, C, K);
  DS2_REQUIRE(max_kw_len >= 0 && max_kw_len <= KWS_MAX_LEN, "%s: max_kw_len must lie in [0, %d] (one wavefront, two states per lane), got %d",
              who, KWS_MAX_LEN, max_kw_len);
  DS2_REQUIRE(max_kw_len == 0 || kw_labels_dev, "%s: null keyword labels", who);
  DS2_REQUIRE(is_log == 0 || is_log == 1, "%s: is_log must be 0 or 1", who);
  DS2_REQUIRE(finish == 0 || finish == 1, "%s: finish must be 0 or 1", who);
  DS2_REQUIRE(max_hits >= 1 && max_hits <= KWS_MAX_HITS, "%s: max_hits must lie in [1, %d], got %d", who, KWS_MAX_HITS, max_hits);
  DS2_REQUIRE(pending >= 1 && pending <= KWS_MAX_PENDING, "%s: pending must lie in [1, %d], got %d", who, KWS_MAX_PENDING, pending);
  DS2_REQUIRE(state_bytes >= ds2_ctc_kws_stream_state_bytes(B, K, pending), "%s: state too small: %zu bytes, %zu needed", who, state_bytes,
              ds2_ctc_kws_stream_state_bytes(B, K, pending));
  DS2_REQUIRE(frames_bound >= 0 && frames_bound + T <= 0x7fffffffLL, "%s: %lld frames so far + %d now pass 2^31 - 1", who, frames_bound, T);
  const size_t need = ds2_ctc_kws_stream_workspace_bytes(B, T, K, frame_score != nullptr);
  DS2_REQUIRE(need == 0 || (ws && ws_bytes >= need), "%s: workspace too small: %zu bytes, %zu needed", who, ws_bytes, need);
  KwsStreamArgs a{};
  a.x = x; a.ld_b = ld_b; a.ld_t = ld_t; a.T = T; a.C = C; a.K = K;
  a.in_lens = in_lens_dev; a.kw_labels = kw_labels_dev; a.kw_off = kw_off_dev; a.kw_lens = kw_lens_dev; a.maxU = max_kw_len;
  a.thr = thr_dev; a.max_hits = max_hits;
  float* g = (float*)ws;
  a.g = g;
  a.fscore = frame_score ? frame_score : g + (size_t)B * (size_t)T;
  a.fstart = frame_start ? frame_start : (int*)(g + (size_t)B * (size_t)T + (size_t)B * (size_t)K * (size_t)T);
  a.hit_start = hit_start; a.hit_end = hit_end; a.hit_score = hit_score; a.n_hits = n_hits; a.cand = nullptr;
  a.state = (int*)state; a.pending = pending; a.max_lag = max_lag < 0 ? -1 : max_lag; a.finish = finish;
  a.hit_final = hit_final; a.tail = tail; a.frames = frames; a.forced = forced; a.dropped = dropped;
  const dim3 grid((unsigned)(B * K));
  hipStream_t s = (hipStream_t)stream;
  if (T > 0) {
    if (int rc = align_star_row_launch(x, ld_b, ld_t, B, T, C, is_log, in_lens_dev, 0.f, g, stream)) return rc;
    if (is_log) hipLaunchKernelGGL((ctc_kws_wave_kernel<1, KwsStreamArgs>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((ctc_kws_wave_kernel<0, KwsStreamArgs>), grid, dim3(64), 0, s, a);
    DS2_LAUNCH_CHECK("ctc_kws_wave_kernel<STREAM>");
  }
  hipLaunchKernelGGL(ctc_kws_stream_pick_kernel, grid, dim3(64), 0, s, a);
  DS2_LAUNCH_CHECK("ctc_kws_stream_pick_kernel");
  return 0;
}
