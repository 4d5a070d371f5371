// CTC forced alignment of imperfect transcripts (ds2_ctc_align_star_f32, ds2_ctc_align_star_tiled_f32, contract in include/ds2hip.h):
// a wildcard label (the value C) and per-utterance optional first / last tokens.  Compiled inside ctc.hip's translation unit, after
// ctc_align.h and ctc_align_tiled.h, whose lattice kernels it instantiates with STAR = true (the plain entries keep STAR = false: no
// select, no flag, the kernels they always had).  What is new here is the pre-pass and the two entries:
//   the wildcard row g[b][t] = max_c e[t][c] + star_penalty, one pass over x for the valid frames.  A row of C classes is read by a
//   group of 8 .. 64 adjacent lanes (the smallest power of two with at most four loads per lane, so that C = 29 keeps 32 rows per
//   workgroup in flight and C = 3000 has whole wavefronts striding the row), the lanes' maxima meet by butterfly shuffles inside the
//   group, and lane 0 of the group does the ONE add and the store.  With probabilities the max is taken on x and align_emit of it is
//   the log (log is monotonic: the same value as the max of the logs, for one log2 per row instead of C).
// g lives in the workspace behind the arrays of the plain entry, so both workspace sizes are the plain ones + 4 B T (+ 8 B for the
// tiled entry's four end values instead of two).
#pragma once
#ifndef DS2_CTC_ALIGN_TU
#error "ctc_align_star.h is a part of ctc.hip"
#endif

namespace {

struct StarRowArgs {
  const float* x;
  long long ld_b, ld_t;
  int B, T, C;
  const int* in_lens;
  float* g;              // [B][T]; frames t >= T_b are not written (nothing reads them)
  float penalty;
  int lg;                // log2 of the lanes per row
};

template <int IS_LOG>
__global__ __launch_bounds__(256) void ctc_align_star_row_kernel(StarRowArgs r) {
  const int q = threadIdx.x & ((1 << r.lg) - 1), rpb = 256 >> r.lg;
  const long long rows = (long long)r.B * r.T;
  for (long long r0 = (long long)blockIdx.x * rpb; r0 < rows; r0 += (long long)gridDim.x * rpb) {   // (uniform trip count per workgroup)
    const long long row = r0 + (threadIdx.x >> r.lg);
    bool valid = row < rows;
    const int b = valid ? (int)(row / r.T) : 0;
    const int t = valid ? (int)(row - (long long)b * r.T) : 0;
    const int Tb = r.in_lens ? min(r.in_lens[b], r.T) : r.T;
    valid = valid && t < Tb;
    float m = NEG_INF;
    if (valid) {
      const float* xr = r.x + (long long)b * r.ld_b + (long long)t * r.ld_t;
#pragma unroll 4
      for (int c = q; c < r.C; c += 1 << r.lg) {
        const float v = xr[c];
        m = v > m ? v : m;
      }
    }
    for (int o = (1 << r.lg) >> 1; o > 0; o >>= 1) {           // every lane takes part: the groups are aligned inside the wavefront
      const float v = __shfl_xor(m, o);
      m = v > m ? v : m;
    }
    if (valid && q == 0) {
#pragma clang fp contract(off)
      const float e = align_emit<IS_LOG>(m);
      r.g[row] = e + r.penalty;
    }
  }
}

int align_star_row_launch(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* in_lens, float penalty,
                          float* g, void* stream) {
  StarRowArgs r;
  r.x = x; r.ld_b = ld_b; r.ld_t = ld_t; r.B = B; r.T = T; r.C = C; r.in_lens = in_lens; r.g = g; r.penalty = penalty;
  r.lg = 3;
  while (r.lg < 6 && (4 << r.lg) < C) ++r.lg;
  const long long rpb = 256 >> r.lg, blocks = ((long long)B * T + rpb - 1) / rpb;
  const dim3 grid((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)));
  if (is_log) hipLaunchKernelGGL(ctc_align_star_row_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, r);
  else hipLaunchKernelGGL(ctc_align_star_row_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, r);
  DS2_LAUNCH_CHECK("ctc_align_star_row_kernel");
  return 0;
}

inline bool align_star_penalty_ok(float p) { return p <= 0.f && p >= -3.402823466e+38f; }   // (NaN fails the first test)

}  // namespace

extern "C" int ds2_ctc_align_star_row_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                                          const int* in_lens_dev, float star_penalty, float* g, void* stream) {
  DS2_REQUIRE(x && g, "ds2_ctc_align_star_row_f32: null pointer");
  DS2_REQUIRE(B > 0 && T > 0 && C > 0 && ld_b > 0 && ld_t > 0, "ds2_ctc_align_star_row_f32: bad dims (B=%d T=%d C=%d)", B, T, C);
  DS2_REQUIRE(is_log == 0 || is_log == 1, "ds2_ctc_align_star_row_f32: is_log must be 0 or 1");
  DS2_REQUIRE(align_star_penalty_ok(star_penalty), "ds2_ctc_align_star_row_f32: star_penalty must be finite and <= 0, got %g",
              (double)star_penalty);
  return align_star_row_launch(x, ld_b, ld_t, B, T, C, is_log, in_lens_dev, star_penalty, g, stream);
}

extern "C" size_t ds2_ctc_align_star_workspace_bytes(int B, int T, int max_target_len) {
  const size_t plain = ds2_ctc_align_workspace_bytes(B, T, max_target_len);
  return plain ? plain + (size_t)B * (size_t)T * sizeof(float) : 0;
}

extern "C" int ds2_ctc_align_star_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* targets_dev,
                                      const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len,
                                      int variant, float star_penalty, const int* flags_dev, float* score, int* states, int* tok_start,
                                      int* tok_end, float* tok_logp, void* ws, size_t ws_bytes, void* stream) {
  AlignArgs a;
  if (int rc = align_entry_args("ds2_ctc_align_star_f32", a, x, ld_b, ld_t, B, T, C, is_log, targets_dev, tgt_off_dev, in_lens_dev,
                                tgt_lens_dev, max_target_len, score, states, tok_start, tok_end, tok_logp)) return rc;
  DS2_REQUIRE(variant >= 0 && variant <= 2, "ds2_ctc_align_star_f32: variant must be 0, 1 or 2");
  DS2_REQUIRE(align_star_penalty_ok(star_penalty), "ds2_ctc_align_star_f32: star_penalty must be finite and <= 0, got %g",
              (double)star_penalty);
  const int Smax = 2 * max_target_len + 1;
  DS2_REQUIRE(variant != 1 || Smax <= 128, "ds2_ctc_align_star_f32: variant 1 (one wavefront) needs 2 * max_target_len + 1 <= 128, got %d",
              Smax);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_align_star_workspace_bytes(B, T, max_target_len), "ds2_ctc_align_star_f32: workspace too small");
  float* g = (float*)((char*)ws + ds2_ctc_align_workspace_bytes(B, T, max_target_len));
  if (int rc = align_star_row_launch(x, ld_b, ld_t, B, T, C, is_log, in_lens_dev, star_penalty, g, stream)) return rc;
  a.bp = (unsigned*)ws;
  a.g = g; a.flags = flags_dev;
  return align_launch<true>("ds2_ctc_align_star_f32", a, B, is_log, variant, max_target_len, stream);
}

extern "C" size_t ds2_ctc_align_star_tiled_workspace_bytes(int B, int T, int max_target_len, int tile_frames, int tile_pairs) {
  if (B <= 0 || T <= 0 || max_target_len < 0 || !align_tiled_shape(tile_frames, tile_pairs)) return 0;
  const AlignTiledLayout L = align_tiled_layout(B, T, max_target_len, tile_frames, tile_pairs, true);
  return (L.bp_words + L.col_words + L.carry_words + L.fin_words + (size_t)B * (size_t)T) * sizeof(float);
}

extern "C" int ds2_ctc_align_star_tiled_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                                            const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                                            int max_target_len, int tile_frames, int tile_pairs, float star_penalty, const int* flags_dev,
                                            float* score, int* states, int* tok_start, int* tok_end, float* tok_logp, void* ws,
                                            size_t ws_bytes, void* stream) {
  AlignArgs a;
  if (int rc = align_entry_args("ds2_ctc_align_star_tiled_f32", a, x, ld_b, ld_t, B, T, C, is_log, targets_dev, tgt_off_dev, in_lens_dev,
                                tgt_lens_dev, max_target_len, score, states, tok_start, tok_end, tok_logp)) return rc;
  DS2_REQUIRE(align_tiled_shape(tile_frames, tile_pairs),
              "ds2_ctc_align_star_tiled_f32: tile_frames must be a positive multiple of 8 and tile_pairs a positive multiple of 64 up to "
              "1024 (or 0 for the default), got %d x %d", tile_frames, tile_pairs);
  DS2_REQUIRE(align_star_penalty_ok(star_penalty), "ds2_ctc_align_star_tiled_f32: star_penalty must be finite and <= 0, got %g",
              (double)star_penalty);
  DS2_REQUIRE(ws && ws_bytes >= ds2_ctc_align_star_tiled_workspace_bytes(B, T, max_target_len, tile_frames, tile_pairs),
              "ds2_ctc_align_star_tiled_f32: workspace too small");
  const AlignTiledLayout L = align_tiled_layout(B, T, max_target_len, tile_frames, tile_pairs, true);
  float* g = (float*)ws + (L.bp_words + L.col_words + L.carry_words + L.fin_words);
  if (int rc = align_star_row_launch(x, ld_b, ld_t, B, T, C, is_log, in_lens_dev, star_penalty, g, stream)) return rc;
  a.g = g; a.flags = flags_dev;
  return align_tiled_launch<true>("ds2_ctc_align_star_tiled_f32", a, B, is_log, max_target_len, tile_frames, tile_pairs, (float*)ws, stream);
}
