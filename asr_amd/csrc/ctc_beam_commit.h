// Commit and compaction of a streaming beam search's back-pointers (ctc_beam_stream.h): what keeps an open stream's memory bounded.
// Every later beam descends from a beam alive now, so the (label, offset) pairs all live beams share are final: they can leave the device,
// and of the node storage only the LIVE TREE is still needed, the nodes on the chains from the live beams down to the stable node.  One
// launch, one workgroup per utterance:
//   cut      (where cut_frame[b] >= 0) the forced cut: the first slot of the saved state decides the text before frame cut_frame[b]; beams
//            that do not share those m pairs are dropped, the survivors move to the front with every per-beam field, and the stable
//            prefix becomes those m pairs.  The only step that changes what the search computes;
//   commit   the pairs between committed_len and min(stable_len, committed_len + Wc) are written, in text order, to the caller's rows;
//            the node of the last committed pair is the ROOT of what stays (the stable node, unless the rows were too narrow);
//   mark     one thread per live beam walks its chain down to the root and sets a bit per node (a walk stops at a marked node: whoever
//            marked it goes on to the root); the bitmap over the rows in use is in LDS where it fits, else in the workspace;
//   scan     a node's new id is the rank of its bit: an exclusive prefix of the words' popcounts plus a masked popcount.  Ranks keep the
//            order of the ids, so a parent stays below its children;
//   move     parent (renumbered; the root's is -1), label and frame go to the DESTINATION storage, a distinct buffer that may be larger:
//            growth and compaction are one copy.  The beams' nodes and the header's stable node are renumbered, row_base becomes
//            ceil(M / K) and frame_base the frames consumed: the next frame writes the first row after the live tree.
// Why the search's bits do not change: the candidate order (CandLess, ctc_beam.h) walks two chains of equal length only until they meet,
// and all live beams descend from the root, so they meet at it or above it; stream_stable never walks below its floor stable_len; the
// prefix hashes are carried per beam; the LM and hotword states hold no ids of this tree.
#pragma once
#ifndef DS2_CTC_BEAM_TU
#error "ctc_beam_commit.h defines ds2_ctc_beam_stream_commit: it is compiled once, as part of decode.hip, after ctc_beam_stream.h"
#endif

namespace {

constexpr size_t COMMIT_LDS_BYTES = 48 * 1024;   // bitmap (8 B) and prefix (4 B) per 64 nodes: up to 4096 words = 262144 nodes in LDS

__host__ __device__ inline size_t commit_words(int cap_rows, int K) { return ((size_t)cap_rows * K + 63) / 64; }

struct CommitArgs {
  char* state;
  size_t stride;
  const int* src;   // (B, 3, cap_src * K)
  int* dst;         // (B, 3, cap_dst * K)
  int cap_src, cap_dst, K, Wc, lm, hot;
  const int* cut_frame;   // (B) or null
  int *labels, *offsets;  // (B, Wc)
  int *info, *dropped;    // (B, 4), (B) or null
  u64* ws;                // null: the bitmap fits LDS
  size_t ws_words;        // words per utterance in ws
};

// the beams of a state blob, in place (the layout of stream_save)
struct BlobBeams {
  float *pb, *pnb, *tot;
  int *node, *len, *last;
  u64 *h, *ph;
  int* lm_ctx;
  float* lm_bow;
  int* lm_node;
  float* lm_lmb;
  int* hot;
};

__device__ inline BlobBeams blob_beams(char* p, int K) {
  BlobBeams s;
  char* q = p + sizeof(StreamHeader);
  s.pb = (float*)q;
  s.pnb = s.pb + K;
  s.tot = s.pnb + K;
  s.node = (int*)(s.tot + K);
  s.len = s.node + K;
  s.last = s.len + K;
  s.h = (u64*)(q + Layout::align_up(6 * 4 * (size_t)K, 16));
  s.ph = s.h + K;
  char* l = q + Layout::buffer_bytes(K);
  s.lm_ctx = (int*)l;
  s.lm_bow = (float*)(s.lm_ctx + LM_CTX * K);
  s.lm_node = (int*)(s.lm_bow + LM_CTX * K);
  s.lm_lmb = (float*)(s.lm_node + K);
  s.hot = (int*)(l + stream_lm_bytes(K));
  return s;
}

__device__ inline int commit_rank(const u64* bits, const unsigned* pre, int id) {
  return (int)pre[id >> 6] + __popcll(bits[id >> 6] & ((1ull << (id & 63)) - 1));
}

__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_commit_kernel(CommitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int sh_i[8];          // 0: m / root, 1: target node, 2: kept beams, 3: longest beam, 4: scan carry
  __shared__ int wave_sum[BEAM_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = a.K;
  char* blob = a.state + (size_t)b * a.stride;
  StreamHeader* sh = (StreamHeader*)blob;
  int* info = a.info + 4 * b;
  if (sh->opened == 0) {   // never fed: nothing to commit, nothing to move (uniform: the whole workgroup leaves)
    if (tid == 0) {
      info[0] = info[1] = info[2] = info[3] = 0;
      if (a.dropped) a.dropped[b] = 0;
    }
    return;
  }
  const long long SK = (long long)a.cap_src * K, DK = (long long)a.cap_dst * K;
  const int* s_parent = a.src + (long long)b * 3 * SK;
  const int* s_label = s_parent + SK;
  const int* s_frame = s_label + SK;
  int* d_parent = a.dst + (long long)b * 3 * DK;
  int* d_label = d_parent + DK;
  int* d_frame = d_label + DK;
  const BlobBeams bm = blob_beams(blob, K);
  int nb = min(max(sh->nb, 0), K);
  const int t0 = sh->t0, done = sh->committed_len;
  const int rows = min(max(sh->row_base + t0 - sh->frame_base, 0), a.cap_src);   // rows in use
  int stable_len = sh->stable_len, stable_node = sh->stable_node, n_drop = 0;
  if (nb == 0) {   // a dead stream keeps no node: the next frames (which the search skips) count from row 0
    if (tid == 0) {
      sh->row_base = 0;
      sh->frame_base = t0;
      info[0] = info[1] = info[2] = 0;
      info[3] = sh->commit_frame;
      if (a.dropped) a.dropped[b] = 0;
    }
    return;
  }

  // 1. forced cut
  const int cut = a.cut_frame ? a.cut_frame[b] : -1;
  if (cut >= 0) {
    if (tid == 0) {   // m: the first slot's pairs before the cut; only a depth above the stable prefix matters
      int x = bm.node[0], d = bm.len[0];
      while (d > stable_len && s_frame[x] >= cut) {
        x = s_parent[x];
        --d;
      }
      sh_i[0] = d;
      sh_i[1] = x;
    }
    __syncthreads();
    const int m = sh_i[0], target = sh_i[1];
    if (m > stable_len) {   // (uniform)
      bool keep = false;
      if (tid < nb && bm.len[tid] >= m) {
        int x = bm.node[tid];
        for (int d = bm.len[tid]; d > m; --d) x = s_parent[x];
        keep = x == target;
      }
      // survivors move to the front in order: every thread reads its beam, all wait, then each writes its new slot (never above its own)
      const u64 mask = __ballot(keep);
      if (lane == 0) wave_sum[wave] = __popcll(mask);
      __syncthreads();
      int rank = __popcll(mask & ((1ull << lane) - 1)), kept = 0;
      for (int w = 0; w < BEAM_THREADS / 64; ++w) {
        if (w < wave) rank += wave_sum[w];
        kept += wave_sum[w];
      }
      float pb = 0.f, pnb = 0.f, tot = 0.f, lmb = 0.f, bow[LM_CTX];
      int node = 0, len = 0, last = 0, lnode = 0, hs = 0, ctx[LM_CTX];
      u64 h = 0, ph = 0;
      if (keep) {
        pb = bm.pb[tid], pnb = bm.pnb[tid], tot = bm.tot[tid];
        node = bm.node[tid], len = bm.len[tid], last = bm.last[tid];
        h = bm.h[tid], ph = bm.ph[tid];
        if (a.lm) {
#pragma unroll
          for (int i = 0; i < LM_CTX; ++i) {
            ctx[i] = bm.lm_ctx[tid * LM_CTX + i];
            bow[i] = bm.lm_bow[tid * LM_CTX + i];
          }
          lnode = bm.lm_node[tid], lmb = bm.lm_lmb[tid];
        }
        if (a.hot) hs = bm.hot[tid];
      }
      __syncthreads();
      if (keep) {
        bm.pb[rank] = pb, bm.pnb[rank] = pnb, bm.tot[rank] = tot;
        bm.node[rank] = node, bm.len[rank] = len, bm.last[rank] = last;
        bm.h[rank] = h, bm.ph[rank] = ph;
        if (a.lm) {
#pragma unroll
          for (int i = 0; i < LM_CTX; ++i) {
            bm.lm_ctx[rank * LM_CTX + i] = ctx[i];
            bm.lm_bow[rank * LM_CTX + i] = bow[i];
          }
          bm.lm_node[rank] = lnode, bm.lm_lmb[rank] = lmb;
        }
        if (a.hot) bm.hot[rank] = hs;
      }
      n_drop = nb - kept;
      nb = kept;          // (>= 1: the first slot keeps itself)
      stable_len = m;
      stable_node = target;
    }
    __syncthreads();
  }

  // 2. commit: the root is the node of the last pair that leaves
  const int upto = min(stable_len, done + max(a.Wc, 0));
  if (tid == 0) {
    int x = stable_len > 0 ? stable_node : -1;
    for (int d = stable_len; d > upto; --d) x = s_parent[x];
    sh_i[0] = x;   // the root (-1 with nothing committed, ever)
    for (int d = upto; d > done; --d) {
      a.labels[(long long)b * a.Wc + d - done - 1] = s_label[x];
      a.offsets[(long long)b * a.Wc + d - done - 1] = s_frame[x];
      x = s_parent[x];
    }
    sh_i[3] = 0;
  }
  const int nwords = (int)(((long long)rows * K + 63) / 64);
  u64* bits = a.ws ? a.ws + (size_t)b * a.ws_words * 2 : (u64*)smem;
  unsigned* pre = a.ws ? (unsigned*)(bits + a.ws_words) : (unsigned*)(smem + 8 * (size_t)commit_words(a.cap_src, K));
  for (int w = tid; w < nwords; w += BEAM_THREADS) bits[w] = 0;
  __syncthreads();
  const int root = sh_i[0];
  const int floor_d = max(upto, 1);   // the depth of the last node a walk marks

  // 3. mark
  if (tid < nb) {
    int x = bm.node[tid];
    atomicMax(&sh_i[3], bm.len[tid]);
    for (int d = bm.len[tid]; d >= floor_d && (unsigned)x < (unsigned)(rows * K); --d) {   // (a foreign state must not mark past the bitmap)
      const u64 bit = 1ull << (x & 63);
      if (atomicOr((unsigned long long*)&bits[x >> 6], bit) & bit) break;
      x = s_parent[x];
    }
  }
  __syncthreads();

  // 4. scan: every thread a run of words, a block scan of the runs' sums
  const int run = (nwords + BEAM_THREADS - 1) / BEAM_THREADS, w0 = min(tid * run, nwords), w1 = min(w0 + run, nwords);
  int mine = 0;
  for (int w = w0; w < w1; ++w) mine += __popcll(bits[w]);
  const int incl = wave_incl_scan_i(mine, lane);
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int before = incl - mine, M = 0;
  for (int w = 0; w < BEAM_THREADS / 64; ++w) {
    if (w < wave) before += wave_sum[w];
    M += wave_sum[w];
  }
  for (int w = w0; w < w1; ++w) {
    pre[w] = (unsigned)before;
    before += __popcll(bits[w]);
  }
  __syncthreads();

  // 5. move (M <= rows * K <= cap_src * K <= cap_dst * K: the entry has checked the capacities)
  for (int w = tid; w < nwords; w += BEAM_THREADS) {
    u64 v = bits[w];
    int id_new = (int)pre[w];
    while (v) {
      const int id = (w << 6) + __ffsll((long long)v) - 1;
      v &= v - 1;
      const int p = s_parent[id];
      d_parent[id_new] = (id == root || p < 0) ? -1 : commit_rank(bits, pre, p);
      d_label[id_new] = s_label[id];
      d_frame[id_new] = s_frame[id];
      ++id_new;
    }
  }
  if (tid < nb && bm.node[tid] >= 0) bm.node[tid] = commit_rank(bits, pre, bm.node[tid]);
  if (tid == 0) {
    sh->nb = nb;
    sh->stable_len = stable_len;
    sh->stable_node = stable_len > 0 ? commit_rank(bits, pre, stable_node) : stable_node;
    sh->row_base = (M + K - 1) / K;
    sh->frame_base = t0;
    if (upto > done) sh->commit_frame = s_frame[root];
    sh->committed_len = upto;
    info[0] = upto - done;
    info[1] = M;
    info[2] = sh_i[3] - upto;
    info[3] = sh->commit_frame;
    if (a.dropped) a.dropped[b] = n_drop;
  }
}

}  // namespace

// bytes of the workspace ds2_ctc_beam_stream_commit needs for a source of cap_rows rows: 0 where the bitmap fits LDS
extern "C" size_t ds2_ctc_beam_stream_commit_workspace_bytes(int B, int cap_rows, int beam_width) {
  if (B <= 0 || cap_rows <= 0 || beam_width <= 0 || beam_width > BEAM_MAX_K || cap_rows > BEAM_MAX_T) return 0;
  const size_t words = commit_words(cap_rows, beam_width);
  if (12 * words <= COMMIT_LDS_BYTES) return 0;
  return (size_t)B * 2 * words * sizeof(u64);   // bitmap words, then the prefix in the space of as many words
}

extern "C" int ds2_ctc_beam_stream_commit(void* state, size_t state_bytes, int B, int beam_width, int lm, int hot, const void* nodes,
                                          size_t nodes_bytes, int cap_rows, void* nodes_out, size_t nodes_out_bytes, int cap_rows_out,
                                          const int* cut_frame, int Wc, int* labels, int* offsets, int* info, int* dropped, void* ws,
                                          size_t ws_bytes, void* stream) {
  const char* who = "ds2_ctc_beam_stream_commit";
  DS2_REQUIRE(state && nodes && nodes_out && info && (Wc <= 0 || (labels && offsets)), "%s: null pointer", who);
  DS2_REQUIRE(B > 0 && beam_width >= 1 && beam_width <= BEAM_MAX_K && Wc >= 0, "%s: bad dims (B=%d beam_width=%d Wc=%d; beam_width <= %d)", who, B,
              beam_width, Wc, BEAM_MAX_K);
  DS2_REQUIRE(cap_rows >= 1 && cap_rows <= BEAM_MAX_T && cap_rows_out <= BEAM_MAX_T, "%s: node capacities %d -> %d rows outside 1..%d", who,
              cap_rows, cap_rows_out, BEAM_MAX_T);
  DS2_REQUIRE(cap_rows_out >= cap_rows, "%s: destination too small: %d rows for a source of %d (the live tree may be all of it)", who,
              cap_rows_out, cap_rows);
  const size_t src_need = ds2_ctc_beam_stream_nodes_bytes(B, cap_rows, beam_width), dst_need = ds2_ctc_beam_stream_nodes_bytes(B, cap_rows_out, beam_width);
  DS2_REQUIRE(nodes_bytes >= src_need, "%s: node buffer too small: %zu bytes, a capacity of %d rows needs %zu", who, nodes_bytes, cap_rows, src_need);
  DS2_REQUIRE(nodes_out_bytes >= dst_need, "%s: destination too small: %zu bytes, a capacity of %d rows needs %zu", who, nodes_out_bytes,
              cap_rows_out, dst_need);
  const char *s0 = (const char*)nodes, *d0 = (const char*)nodes_out;
  DS2_REQUIRE(s0 + src_need <= d0 || d0 + dst_need <= s0, "%s: the destination aliases the source: compaction moves nodes between distinct buffers",
              who);
  DS2_REQUIRE(state_bytes >= ds2_ctc_beam_stream_state_bytes(B, beam_width, lm, hot), "%s: state too small: %zu bytes, %zu needed", who, state_bytes,
              ds2_ctc_beam_stream_state_bytes(B, beam_width, lm, hot));
  const size_t need = ds2_ctc_beam_stream_commit_workspace_bytes(B, cap_rows, beam_width), words = commit_words(cap_rows, beam_width);
  DS2_REQUIRE(need == 0 || (ws && ws_bytes >= need), "%s: workspace too small: %zu bytes, %zu needed", who, ws_bytes, need);
  CommitArgs a{(char*)state, stream_stride(beam_width, lm != 0, hot != 0), (const int*)nodes, (int*)nodes_out, cap_rows, cap_rows_out,
               beam_width, Wc, lm != 0 || hot != 0, hot != 0, cut_frame, labels, offsets, info, dropped, need ? (u64*)ws : nullptr, words};
  hipLaunchKernelGGL(ctc_beam_commit_kernel, dim3(B), dim3(BEAM_THREADS), need ? 0 : 12 * words, (hipStream_t)stream, a);
  DS2_LAUNCH_CHECK("ctc_beam_commit_kernel");
  return 0;
}
