// Streaming CTC prefix beam search: ctc_beam_kernel (ctc_beam.h) stopped after any frame, stored and resumed with the same bits.
// Everything the search carries from one frame to the next is plain data per beam (pb, pnb, tot, node, len, last, the two hashes, the
// LM arm's ctx / bow / node / lmb, the hotword arm's automaton node) and the number of live beams; nothing in a frame's arithmetic
// depends on T.  A streaming launch (one workgroup per utterance, as the one-call kernel) therefore does:
//   load     the state blob's beams into beam buffer 0 (a blob of zero bytes: the one-call kernel's initialisation instead);
//   frames   the unchanged per-frame loop over this call's frames; only the frame index of a new node is t0 + t;
//   save     the current buffers, nb and t0 + n back to the blob, BEFORE the end-of-utterance stage, which then works on LDS alone;
//   read-out (n_out > 0) the end-of-utterance stage and the first n_out slots in the one-call format, in rows of the caller's width;
//   stable   the length of the (label, offset) prefix common to every live beam.
// The state adds no LDS: the blob is copied straight into and out of the buffers the kernel has, and the stable prefix borrows one
// int of the header.
//
// Stable prefix: every beam of every later call descends from a beam alive now, so what all live beams share can never change, in
// labels or in offsets.  A node is made once per (prefix, frame), so two chains spell the same (label, offset) pairs exactly when they
// end in the same node: one thread per live beam walks its back-pointers up to the depth of the shortest beam, then all step to the
// parent together until every thread holds the same node.  The previous length stays in the state; it is a floor (every live beam
// descends from beams that shared it), so a call walks the unstable suffix, not the stream.  With no live beam the value is kept.
//
// Node storage is the caller's, laid out for `cap` rows of K nodes per utterance (parent | label | frame, cap * K each); node ids do not
// depend on cap, so the host grows it between calls by copying each utterance's three arrays into a larger buffer.  A frame writes the
// row of its index until a commit (ctc_beam_commit.h) compacts the rows to the live tree: then frame t0 + t writes row row_base + t0 + t
// - frame_base, and a read-out starts at the pair committed_len (all zero in a stream that never commits).
#pragma once
#ifndef DS2_CTC_BEAM_TU
#error "ctc_beam_stream.h defines the ds2_ctc_beam_stream_* entry points: it is compiled once, as part of decode.hip, after ctc_beam.h"
#endif

namespace {

__host__ __device__ inline size_t stream_lm_bytes(int K) { return Layout::align_up(lm_beams_bytes(K), 16); }
// bytes of one utterance's blob; LmBeams are kept by the LM arm and by the hotword arm, whose lmb rides there without an LM
__host__ __device__ inline size_t stream_stride(int K, bool lm, bool hot) {
  return sizeof(StreamHeader) + Layout::buffer_bytes(K) + (lm || hot ? stream_lm_bytes(K) : 0) + (hot ? hot_state_bytes(K) : 0);
}

// nbytes (a multiple of 4) from src to dst, one of them LDS, by the whole workgroup: 16-byte vectors where both sides allow, else dwords
__device__ inline void stream_copy(void* dst, const void* src, size_t nbytes) {
  if ((((size_t)dst | (size_t)src | nbytes) & 15) == 0) {
    uint4* d = (uint4*)dst;
    const uint4* s = (const uint4*)src;
    for (size_t i = threadIdx.x; i < nbytes / 16; i += BEAM_THREADS) d[i] = s[i];
  } else {
    unsigned* d = (unsigned*)dst;
    const unsigned* s = (const unsigned*)src;
    for (size_t i = threadIdx.x; i < nbytes / 4; i += BEAM_THREADS) d[i] = s[i];
  }
}

__device__ inline void stream_load(const StreamArgs& st, int b, const Layout& L, char* smem, Header* hd, bool lm, const LmBeams& l0, int* h0) {
  const char* p = st.state + (size_t)b * st.stride;
  const size_t bb = Layout::buffer_bytes(L.K);
  stream_copy(smem + L.beams, p + sizeof(StreamHeader), bb);
  if (lm) stream_copy(l0.ctx, p + sizeof(StreamHeader) + bb, lm_beams_bytes(L.K));
  if (h0) stream_copy(h0, p + sizeof(StreamHeader) + bb + stream_lm_bytes(L.K), hot_state_bytes(L.K));
  if (threadIdx.x == 0) hd->nb = min(max(((const StreamHeader*)p)->nb, 0), L.K);
}

__device__ inline void stream_save(const StreamArgs& st, int b, const Layout& L, char* smem, const Header* hd, int cur, int frames, bool lm,
                                   const LmBeams& l0, const LmBeams& l1, const int* hf) {
  char* p = st.state + (size_t)b * st.stride;
  const size_t bb = Layout::buffer_bytes(L.K);
  stream_copy(p + sizeof(StreamHeader), smem + L.beams + cur * bb, bb);
  if (lm) stream_copy(p + sizeof(StreamHeader) + bb, (cur ? l1 : l0).ctx, lm_beams_bytes(L.K));
  if (hf) stream_copy(p + sizeof(StreamHeader) + bb + stream_lm_bytes(L.K), hf, hot_state_bytes(L.K));
  if (threadIdx.x == 0) {
    StreamHeader* sh = (StreamHeader*)p;
    sh->opened = 1;
    sh->t0 = frames;
    sh->nb = hd->nb;
    st.frames[b] = frames;
  }
}

__device__ inline void stream_stable(const StreamArgs& st, int b, Header* hd, const Beams& f, int nb, const int* n_parent) {
  StreamHeader* sh = (StreamHeader*)(st.state + (size_t)b * st.stride);
  const int tid = threadIdx.x, floor_len = sh->stable_len;
  int sl = floor_len;
  if (nb > 0) {   // nb <= K <= BEAM_THREADS: one thread per live beam
    const bool live = tid < nb;
    int x = live ? f.node[tid] : -1, d = live ? f.len[tid] : 0x7fffffff;
    __syncthreads();
    if (tid == 0) hd->pad2 = 0x7fffffff;
    __syncthreads();
    if (live) atomicMin(&hd->pad2, d);
    __syncthreads();
    const int dmin = hd->pad2;
    for (; live && d > dmin; --d) x = n_parent[x];
    d = dmin;   // the same in every thread from here: the barriers below are met by all
    while (d > floor_len) {
      __syncthreads();
      if (tid == 0) hd->pad2 = x;
      __syncthreads();
      if (__syncthreads_and(!live || x == hd->pad2)) break;
      if (live) x = n_parent[x];
      --d;
    }
    sl = d;
    if (tid == 0) {
      sh->stable_len = d;
      sh->stable_node = x;
    }
  }
  if (tid == 0) st.stable_len[b] = sl;
}

}  // namespace

extern "C" size_t ds2_ctc_beam_stream_state_bytes(int B, int beam_width, int lm, int hot) {
  if (B <= 0 || beam_width <= 0 || beam_width > BEAM_MAX_K) return 0;
  return (size_t)B * stream_stride(beam_width, lm != 0, hot != 0);
}

extern "C" size_t ds2_ctc_beam_stream_nodes_bytes(int B, int cap_frames, int beam_width) {
  return ds2_ctc_beam_workspace_bytes(B, cap_frames, beam_width);
}

// The two feed entries.  A stream that never committed counts its node rows in frames (cap_frames, frames_bound) and a read-out row holds
// every frame; a committed stream (ctc_beam_commit.h) counts rows (cap_frames and frames_bound are then cap_rows and rows_bound) and a
// read-out row holds the uncommitted labels, of which the host knows the bound labels_bound (< 0: the uncommitted entry).
static int stream_feed(const char* who, const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                       int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev, size_t lm_bytes, int lm_order, int lm_mode,
                       int space, float alpha, float beta, const void* hot_dev, const void* hot_host, size_t hot_bytes, void* state,
                       size_t state_bytes, void* nodes, size_t nodes_bytes, int cap_frames, int frames_bound, int labels_bound, int n_out, int W,
                       int* labels, int* offsets, int* lens, float* scores, int* stable_len, int* frames, void* stream) {
  const bool committed = labels_bound >= 0;
  DS2_REQUIRE(state && nodes && stable_len && frames && (T == 0 || probs) && (n_out <= 0 || (labels && offsets && lens && scores)),
              "%s: null pointer", who);
  DS2_REQUIRE(T >= 0 && frames_bound >= 0 && cap_frames >= 1, "%s: bad dims (T=%d, %d %s so far, node capacity %d %s)", who, T,
              frames_bound, committed ? "rows" : "frames", cap_frames, committed ? "rows" : "frames");
  DS2_REQUIRE(T > 0 || n_out > 0, "%s: no frames and no read-out (T = 0 and n_out = 0): nothing to do", who);
  DS2_REQUIRE((long long)frames_bound + T <= cap_frames, "%s: node buffer too small: capacity %d frames, %d so far + %d now", who, cap_frames,
              frames_bound, T);
  DS2_REQUIRE(nodes_bytes >= ds2_ctc_beam_stream_nodes_bytes(B, cap_frames, beam_width) || B <= 0 || beam_width <= 0,
              "%s: node buffer too small: %zu bytes, a capacity of %d frames needs %zu", who, nodes_bytes, cap_frames,
              ds2_ctc_beam_stream_nodes_bytes(B, cap_frames, beam_width));
  // the checks every decode entry makes, on the stream's own terms: the node buffer is the workspace, of cap_frames frames
  int* const out_or = (int*)state;   // (stands in for outputs a call without read-out does not have)
  if (int rc = beam_check(who, T ? probs : (const float*)state, hot_dev ? hot_dev : (lm_dev ? lm_dev : state), B, cap_frames, C, blank,
                          beam_width, cutoff_top_n, cutoff_prob, n_out > 0 ? labels : out_or, n_out > 0 ? offsets : out_or,
                          n_out > 0 ? lens : out_or, n_out > 0 ? scores : (float*)state, nodes, nodes_bytes)) return rc;
  const int K = beam_width;
  DS2_REQUIRE(n_out >= 0 && n_out <= K, "%s: n_out %d outside 0..beam_width (%d)", who, n_out, K);
  if (committed)
    DS2_REQUIRE(n_out == 0 || (long long)W >= (long long)labels_bound + T, "%s: rows of W = %d labels cannot hold %d uncommitted labels + %d frames now",
                who, W, labels_bound, T);
  else
    DS2_REQUIRE(n_out == 0 || W >= frames_bound + T, "%s: rows of W = %d labels cannot hold %d frames so far + %d now", who, W, frames_bound, T);
  const bool hot = hot_dev != nullptr, lm = lm_dev != nullptr;
  DS2_REQUIRE(state_bytes >= ds2_ctc_beam_stream_state_bytes(B, K, lm, hot), "%s: state too small: %zu bytes, %zu needed", who, state_bytes,
              ds2_ctc_beam_stream_state_bytes(B, K, lm, hot));
  BeamPlan p;
  if (int rc = beam_plan(p, who, C, blank, K, cutoff_top_n, lm_dev, lm_bytes, lm_order, lm_mode, space, alpha, beta, hot_dev, hot_host, hot_bytes))
    return rc;
  const StreamArgs sa{(char*)state, stream_stride(K, lm, hot), cap_frames, n_out, n_out > 0 ? W : 0, stable_len, frames};
  return beam_dispatch(p, BeamCall{probs, ld_b, ld_t, B, T, C, sizes_dev, blank, cutoff_top_n, cutoff_prob, labels, offsets, lens, scores,
                                   (int*)nodes, stream}, &sa);
}

extern "C" int ds2_ctc_beam_stream_feed_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev,
                                            int blank, int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev,
                                            size_t lm_bytes, int lm_order, int lm_mode, int space, float alpha, float beta,
                                            const void* hot_dev, const void* hot_host, size_t hot_bytes, void* state, size_t state_bytes,
                                            void* nodes, size_t nodes_bytes, int cap_frames, int frames_bound, int n_out, int W,
                                            int* labels, int* offsets, int* lens, float* scores, int* stable_len, int* frames,
                                            void* stream) {
  return stream_feed("ds2_ctc_beam_stream_feed_f32", probs, ld_b, ld_t, B, T, C, sizes_dev, blank, beam_width, cutoff_top_n, cutoff_prob, lm_dev,
                     lm_bytes, lm_order, lm_mode, space, alpha, beta, hot_dev, hot_host, hot_bytes, state, state_bytes, nodes, nodes_bytes,
                     cap_frames, frames_bound, -1, n_out, W, labels, offsets, lens, scores, stable_len, frames, stream);
}

extern "C" int ds2_ctc_beam_stream_feed_committed_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C,
                                                      const int* sizes_dev, int blank, int beam_width, int cutoff_top_n, float cutoff_prob,
                                                      const void* lm_dev, size_t lm_bytes, int lm_order, int lm_mode, int space, float alpha,
                                                      float beta, const void* hot_dev, const void* hot_host, size_t hot_bytes, void* state,
                                                      size_t state_bytes, void* nodes, size_t nodes_bytes, int cap_rows, int rows_bound,
                                                      int labels_bound, int n_out, int W, int* labels, int* offsets, int* lens, float* scores,
                                                      int* stable_len, int* frames, void* stream) {
  const char* who = "ds2_ctc_beam_stream_feed_committed_f32";
  DS2_REQUIRE(labels_bound >= 0, "%s: labels_bound %d is negative", who, labels_bound);
  return stream_feed(who, probs, ld_b, ld_t, B, T, C, sizes_dev, blank, beam_width, cutoff_top_n, cutoff_prob, lm_dev, lm_bytes, lm_order, lm_mode,
                     space, alpha, beta, hot_dev, hot_host, hot_bytes, state, state_bytes, nodes, nodes_bytes, cap_rows, rows_bound, labels_bound,
                     n_out, W, labels, offsets, lens, scores, stable_len, frames, stream);
}
