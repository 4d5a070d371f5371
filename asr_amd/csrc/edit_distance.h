// Batched Levenshtein distance (unit costs) over int32 symbol sequences: the WER / CER scoring of DeepSpeech.evaluate().  Replaces
// Decoder.wer / Decoder.cer's per-utterance host DP (the reference calls the `Levenshtein` C package, decoders/decoder.py:26-58);
// the host maps words and characters to int32 ids (asr_amd/decoders), so the kernel knows nothing about labels or text.
//
// Method: Myers' bit-vector algorithm in its blocked form (Myers 1999, "A fast bit-vector algorithm for approximate string matching
// based on dynamic programming", §4; Hyyroe 2003 for the edit-distance reading).  The shorter side a (m symbols) runs along the rows
// in strips of 64, one row per lane; the longer side b (n symbols) along the columns.  A strip's state is the 64-bit pair (Pv, Mv) of
// vertical deltas D[i][j] - D[i-1][j] = +1 / -1; one column step turns (Pv, Mv, Eq, hin) into the next state and hout, the
// horizontal delta D[i_last][j] - D[i_last][j-1] of the strip's last row.  Eq bit i = (a[64s + i] == b[j]) is one compare + ballot.
// The step is a few 64-bit ops on values uniform across the wave (SALU), so a wave needs no barrier and no cross-lane shifts.
//  - strip 0 starts from hin = +1 in every column (D[0][j] = j), every strip from Pv = all ones, Mv = 0 (D[i][0] = i);
//  - strip s > 0 takes hin from strip s-1's hout of the same column: one int8 per column in the problem's workspace row,
//    read and overwritten in place (each lane owns one column of a 64-column chunk), L2-resident at these sizes;
//  - bits above the last row of a partial strip never reach lower bits (carries and shifts only go up): hout is read at bit r-1;
//  - D[m][n] = m + sum_j hout_last(j).
// Exact integer arithmetic: the result is the DP's value, bit for bit.  Cost ceil(m/64) * n dependent column steps per problem;
// one wave per problem, four problems per workgroup, every problem of the batch in one launch.
#pragma once
#ifndef DS2_EDIT_DISTANCE_TU
#error "edit_distance.h defines the ds2_edit_distance_* entry points: it is compiled once, as part of decode.hip"
#endif
#include "common.h"

namespace {

constexpr int ED_WAVES = 4;   // problems per workgroup

__global__ __launch_bounds__(64 * ED_WAVES) void edit_distance_kernel(const int* __restrict__ seq, long long n_seq,
                                                                       const long long* __restrict__ a_off, const int* __restrict__ a_len,
                                                                       const long long* __restrict__ b_off, const int* __restrict__ b_len,
                                                                       int P, signed char* __restrict__ ws, long long ws_stride,
                                                                       int* __restrict__ dist) {
  // wave-uniform problem index: the compiler then keeps lengths, loop bounds and the bit-vector step in SGPRs (SALU)
  const int p = blockIdx.x * ED_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= P) return;
  const int lane = threadIdx.x & 63;
  long long ao = a_off[p], bo = b_off[p];
  int m = a_len[p], n = b_len[p];
  // a problem outside the symbol buffer (or too long for the workspace row below) is not computed: its distance is -1
  const bool bad = m < 0 || n < 0 || ao < 0 || bo < 0 || ao > n_seq - m || bo > n_seq - n;
  if (m > n) {
    const long long to = ao; ao = bo; bo = to;
    const int t = m; m = n; n = t;
  }
  if (bad || (m > 64 && (long long)n > ws_stride)) {
    if (lane == 0) dist[p] = -1;
    return;
  }
  if (m == 0) {
    if (lane == 0) dist[p] = n;
    return;
  }
  const int* A = seq + ao;
  const int* Bs = seq + bo;
  signed char* hrow = ws + (long long)p * ws_stride;
  const int strips = (m + 63) >> 6;
  long long total = 0;
  for (int s = 0; s < strips; ++s) {
    const int r = min(64, m - 64 * s);
    const bool row_ok = lane < r;
    const int a_sym = row_ok ? A[64 * s + lane] : 0;
    const unsigned long long top = 1ull << (r - 1);
    const bool last = s == strips - 1;
    unsigned long long Pv = ~0ull, Mv = 0ull;
    for (long long c = 0; c < n; c += 64) {
      const int cols = (int)min(64ll, (long long)n - c);
      const bool col_ok = lane < cols;
      const int b_sym = col_ok ? Bs[c + lane] : 0;
      const int hin_v = s == 0 ? 1 : (col_ok ? (int)hrow[c + lane] : 0);
      unsigned long long hp = 0ull, hm = 0ull;   // bit jj: hout of column c + jj is +1 / -1
      for (int jj = 0; jj < cols; ++jj) {
        const int bj = __builtin_amdgcn_readlane(b_sym, jj);
        const int hin = __builtin_amdgcn_readlane(hin_v, jj);
        const unsigned long long hneg = hin < 0, hpos = hin > 0;
        const unsigned long long Eq = __ballot(row_ok && a_sym == bj);
        const unsigned long long Xv = Eq | Mv;
        const unsigned long long Eh = Eq | hneg;
        const unsigned long long Xh = (((Eh & Pv) + Pv) ^ Pv) | Eh;
        const unsigned long long Ph = Mv | ~(Xh | Pv);
        const unsigned long long Mh = Pv & Xh;
        hp |= (unsigned long long)((Ph & top) != 0) << jj;
        hm |= (unsigned long long)((Mh & top) != 0) << jj;
        const unsigned long long Phs = (Ph << 1) | hpos, Mhs = (Mh << 1) | hneg;
        Pv = Mhs | ~(Xv | Phs);
        Mv = Phs & Xv;
      }
      if (last) {
        total += (long long)__popcll(hp) - (long long)__popcll(hm);
      } else if (col_ok) {
        hrow[c + lane] = (signed char)((int)((hp >> lane) & 1ull) - (int)((hm >> lane) & 1ull));
      }
    }
  }
  if (lane == 0) dist[p] = (int)(m + total);
}

}  // namespace

extern "C" size_t ds2_edit_distance_workspace_bytes(int P, long long max_len) {
  if (P <= 0 || max_len <= 64) return 0;
  return (size_t)P * align_up((size_t)max_len, 64);
}

extern "C" int ds2_edit_distance_i32(const int* seq, long long n_seq, const long long* a_off, const int* a_len, const long long* b_off,
                                     const int* b_len, int P, long long max_len, int* dist, void* ws, size_t ws_bytes, void* stream) {
  DS2_REQUIRE(P >= 0 && n_seq >= 0 && max_len >= 0, "ds2_edit_distance_i32: bad dims (P=%d n_seq=%lld max_len=%lld)", P, n_seq, max_len);
  if (P == 0) return 0;
  DS2_REQUIRE(a_off && a_len && b_off && b_len && dist, "ds2_edit_distance_i32: null pointer");
  DS2_REQUIRE(seq || n_seq == 0, "ds2_edit_distance_i32: null symbol buffer");
  const size_t need = ds2_edit_distance_workspace_bytes(P, max_len);
  DS2_REQUIRE(need == 0 || (ws && ws_bytes >= need), "ds2_edit_distance_i32: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  const long long stride = need ? (long long)align_up((size_t)max_len, 64) : 0;
  const unsigned grid = (unsigned)(((long long)P + ED_WAVES - 1) / ED_WAVES);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(grid), dim3(64 * ED_WAVES), 0, (hipStream_t)stream, seq, n_seq, a_off, a_len, b_off, b_len,
                     P, (signed char*)ws, stride, dist);
  DS2_LAUNCH_CHECK("edit_distance_kernel");
  return 0;
}
