// Batched edit ALIGNMENT (unit costs) over int32 symbol sequences: which symbols of a hypothesis a and a reference b are hits,
// substitutions, deletions and insertions, and which index pairs with which.  The breakdown behind a WER / CER (Decoder.align_batch,
// decoders.ErrorReport); the problem layout is edit_distance.h's.  The contract (the DP, the tie rule of the traceback, the outputs)
// is stated in include/ds2hip.h and restated by tests/edit_align_oracle.py.
//
// Method.  Forward pass: edit_distance.h's blocked Myers / Hyyroe column step, the shorter side on the rows in strips of 64, one wave
// per problem.  The pair (Pv, Mv) after column j holds the vertical deltas D[i][j] - D[i-1][j] of that column, which the distance
// kernel throws away; here every column's pair is kept per strip (16 bytes, 2 bits per DP cell), written by one coalesced 16-byte
// store per lane and 64 columns.  Any D value is then a masked popcount:
//   D[64 s + r][j] = base_s(j) + popc(Pv_s(j) & low(r)) - popc(Mv_s(j) & low(r)),   base_s(j) = j + sum over t < s of popc(Pv_t(j)) - popc(Mv_t(j))
// (the strips below s are full, so their popcounts are whole words; column 0 is Pv = all ones, Mv = 0 and is not stored).
// Traceback: the same wave, in the same launch, walks from (m, n) to (0, 0).  It holds a window of 64 columns in its lanes (the pair
// of the current strip, base_s and the column's symbol; one coalesced load per lane, and 2 s more for base_s), so a step is a handful
// of v_readlane and 64-bit scalar operations with no memory access; a window is reloaded when the walk leaves it to the left or
// enters the strip above.  Each map entry is decided exactly once: lane (index & 63) keeps it until the walk leaves that block of 64
// indices, then one coalesced store writes the block.  No address is written twice.
// When the sides were swapped (the hypothesis is the longer one and runs along the columns), the second and third option of the tie
// rule trade places: a step that leaves a symbol of b unpaired is then a step UP, and it is tried before the step LEFT.
// Exact integer work: counts and maps are the rule's, entry for entry.  Cost: the distance kernel's ceil(m/64) * n column steps, plus
// at most m + n traceback steps, plus the stores.
#pragma once
#ifndef DS2_EDIT_ALIGN_TU
#error "edit_align.h defines the ds2_edit_align_* entry points: it is compiled once, as part of decode.hip"
#endif
#include "common.h"

namespace {

constexpr int EA_WAVES = 4;   // problems per workgroup

__device__ __forceinline__ unsigned long long ea_readlane64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// one block of 64 map entries, [base, base + 64) cut to len: lane l holds entry base + l
__device__ __forceinline__ void ea_flush(int* __restrict__ map, int base, int len, int lane, int v) {
  if (base + lane < len) map[base + lane] = v;
}

__global__ __launch_bounds__(64 * EA_WAVES) void edit_align_kernel(const int* __restrict__ seq, long long n_seq,
                                                                    const long long* __restrict__ a_off, const int* __restrict__ a_len,
                                                                    const long long* __restrict__ b_off, const int* __restrict__ b_len,
                                                                    int P, long long max_len, ulonglong2* __restrict__ cols,
                                                                    signed char* __restrict__ hws, long long h_stride,
                                                                    int* __restrict__ counts, int* __restrict__ a_map, int* __restrict__ b_map) {
  // wave-uniform problem index: lengths, loop bounds, the bit-vector step and the whole traceback state stay in SGPRs (SALU)
  const int p = blockIdx.x * EA_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p >= P) return;
  const int lane = threadIdx.x & 63;
  long long ao = a_off[p], bo = b_off[p];
  int m = a_len[p], n = b_len[p];
  int* amap = a_map + (long long)p * max_len;
  int* bmap = b_map + (long long)p * max_len;
  const bool bad = m < 0 || n < 0 || ao < 0 || bo < 0 || ao > n_seq - m || bo > n_seq - n || m > max_len || n > max_len;
  // entries at or beyond a side's length (all of them for a rejected problem) are -1; the entries below are written further down
  for (long long k = (long long)(bad ? 0 : m) + lane; k < max_len; k += 64) amap[k] = -1;
  for (long long k = (long long)(bad ? 0 : n) + lane; k < max_len; k += 64) bmap[k] = -1;
  if (bad) {
    if (lane < 4) counts[4 * (long long)p + lane] = -1;
    return;
  }
  // rows: the shorter side (m symbols); columns: the longer (n).  swapped: the hypothesis a runs along the columns
  const bool swapped = m > n;
  int* rmap = amap;
  int* cmap = bmap;
  if (swapped) {
    const long long to = ao; ao = bo; bo = to;
    const int t = m; m = n; n = t;
    rmap = bmap; cmap = amap;
  }
  const int* A = seq + ao;
  const int* Bs = seq + bo;
  const int strips = (m + 63) >> 6;
  const long long L = max_len;
  ulonglong2* W = cols + (long long)p * ((max_len + 63) >> 6) * L;   // W[s * L + j - 1]: (Pv, Mv) of strip s after column j
  signed char* hrow = hws + (long long)p * h_stride;

  // ---- forward pass: edit_distance.h's column step, every column's (Pv, Mv) kept
  for (int s = 0; s < strips; ++s) {
    const int r = min(64, m - 64 * s);
    const bool row_ok = lane < r;
    const int a_sym = row_ok ? A[64 * s + lane] : 0;
    const unsigned long long top = 1ull << (r - 1);
    const bool last = s == strips - 1;
    unsigned long long Pv = ~0ull, Mv = 0ull;
    for (int c = 0; c < n; c += 64) {
      const int ncol = min(64, n - c);
      const bool col_ok = lane < ncol;
      const int b_sym = col_ok ? Bs[c + lane] : 0;
      const int hin_v = s == 0 ? 1 : (col_ok ? (int)hrow[c + lane] : 0);
      unsigned long long hp = 0ull, hm = 0ull;   // bit jj: hout of column c + jj is +1 / -1
      unsigned long long pv_l = 0ull, mv_l = 0ull;   // lane jj: the pair after column c + jj + 1
      for (int jj = 0; jj < ncol; ++jj) {
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
        pv_l = lane == jj ? Pv : pv_l;
        mv_l = lane == jj ? Mv : mv_l;
      }
      if (col_ok) {
        W[(long long)s * L + c + lane] = make_ulonglong2(pv_l, mv_l);
        if (!last) hrow[c + lane] = (signed char)((int)((hp >> lane) & 1ull) - (int)((hm >> lane) & 1ull));
      }
    }
  }
  // the traceback reads, from other lanes, what this wave stored above
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  // ---- traceback from (m, n): all state wave-uniform
  int i = m, j = n;
  int hits = 0, subs = 0, row_only = 0, col_only = 0;
  int rv = -1, cv = -1;        // lane l: the map entry of row / column index (block of 64) + l, decided so far
  int s = -1, cbase = 0;       // the window: strip s, lane l holds column cbase + l
  unsigned long long Pw = 0ull, Mw = 0ull;
  int base_w = 0, bsym_w = 0, asym_w = 0;
  while (i > 0 && j > 0) {
    const int sn = (i - 1) >> 6;
    if (sn != s || j - 1 < cbase) {
      if (sn != s) asym_w = 64 * sn + lane < m ? A[64 * sn + lane] : 0;
      s = sn;
      cbase = max(j - 63, 0);
      const int col = cbase + lane;
      const bool st = col >= 1 && col <= j;       // a stored column (column 0 is the DP's first: Pv all ones, Mv none)
      Pw = ~0ull; Mw = 0ull; base_w = 64 * s; bsym_w = 0;
      if (st) {
        const ulonglong2 w = W[(long long)s * L + col - 1];
        Pw = w.x; Mw = w.y;
        bsym_w = Bs[col - 1];
        base_w = col;
        for (int t = 0; t < s; ++t) {
          const ulonglong2 u = W[(long long)t * L + col - 1];
          base_w += __popcll(u.x) - __popcll(u.y);
        }
      }
    }
    const int r = i - 64 * s;                      // 1 .. 64: the row inside the strip
    const int lj = j - cbase;                      // >= 1: the lanes of columns j and j - 1
    const unsigned long long Pj = ea_readlane64(Pw, lj), Mj = ea_readlane64(Mw, lj);
    const unsigned long long Pq = ea_readlane64(Pw, lj - 1), Mq = ea_readlane64(Mw, lj - 1);
    const int bj = __builtin_amdgcn_readlane(base_w, lj), bq = __builtin_amdgcn_readlane(base_w, lj - 1);
    const int neq = __builtin_amdgcn_readlane(asym_w, r - 1) != __builtin_amdgcn_readlane(bsym_w, lj);
    const unsigned long long mask = ~0ull >> (64 - r), maskm = mask >> 1;
    const int d_ij = bj + __popcll(Pj & mask) - __popcll(Mj & mask);         // D[i][j]
    const int d_left = bq + __popcll(Pq & mask) - __popcll(Mq & mask);       // D[i][j-1]
    const int d_diag = bq + __popcll(Pq & maskm) - __popcll(Mq & maskm);     // D[i-1][j-1]
    const bool diag = d_diag + neq == d_ij;
    const bool left = d_left + 1 == d_ij;
    const bool up = (Pj >> (r - 1)) & 1ull;                                   // D[i-1][j] + 1 == D[i][j]
    // the step that leaves a symbol of b unpaired comes second: LEFT with b on the columns, UP with b on the rows
    const bool go_left = !diag && (swapped ? !up : left);
    const bool go_up = !diag && !go_left;
    if (diag) {
      rv = lane == ((i - 1) & 63) ? j - 1 : rv;
      cv = lane == ((j - 1) & 63) ? i - 1 : cv;
      hits += !neq; subs += neq;
    }
    row_only += go_up; col_only += go_left;
    if (!go_left) {
      --i;
      if ((i & 63) == 0) { ea_flush(rmap, i, m, lane, rv); rv = -1; }
    }
    if (!go_up) {
      --j;
      if ((j & 63) == 0) { ea_flush(cmap, j, n, lane, cv); cv = -1; }
    }
  }
  // one side is used up: what is left of the other is unpaired.  The block the walk stopped in holds its decided entries, -1 elsewhere
  if (i > 0) {
    const int blk = ((i - 1) >> 6) << 6;
    ea_flush(rmap, blk, m, lane, rv);
    for (int k = lane; k < blk; k += 64) rmap[k] = -1;
    row_only += i;
  }
  if (j > 0) {
    const int blk = ((j - 1) >> 6) << 6;
    ea_flush(cmap, blk, n, lane, cv);
    for (int k = lane; k < blk; k += 64) cmap[k] = -1;
    col_only += j;
  }
  // an unpaired symbol of b is a deletion, one of a an insertion
  const int dels = swapped ? row_only : col_only, ins = swapped ? col_only : row_only;
  if (lane < 4) counts[4 * (long long)p + lane] = lane == 0 ? hits : lane == 1 ? subs : lane == 2 ? dels : ins;
}

}  // namespace

extern "C" size_t ds2_edit_distance_workspace_bytes(int P, long long max_len);

extern "C" size_t ds2_edit_align_workspace_bytes(int P, long long max_len) {
  if (P <= 0 || max_len <= 0) return 0;
  return (size_t)P * (size_t)((max_len + 63) / 64) * (size_t)max_len * 16 + ds2_edit_distance_workspace_bytes(P, max_len);
}

extern "C" int ds2_edit_align_i32(const int* seq, long long n_seq, const long long* a_off, const int* a_len, const long long* b_off,
                                  const int* b_len, int P, long long max_len, int* counts, int* a_map, int* b_map, void* ws,
                                  size_t ws_bytes, void* stream) {
  DS2_REQUIRE(P >= 0 && n_seq >= 0 && max_len >= 0, "ds2_edit_align_i32: bad dims (P=%d n_seq=%lld max_len=%lld)", P, n_seq, max_len);
  DS2_REQUIRE(max_len <= 0x7fffffffll, "ds2_edit_align_i32: max_len %lld does not fit the int32 lengths", max_len);
  if (P == 0) return 0;
  DS2_REQUIRE(a_off && a_len && b_off && b_len && counts, "ds2_edit_align_i32: null pointer");
  DS2_REQUIRE((a_map && b_map) || max_len == 0, "ds2_edit_align_i32: null map");
  DS2_REQUIRE(seq || n_seq == 0, "ds2_edit_align_i32: null symbol buffer");
  const size_t need = ds2_edit_align_workspace_bytes(P, max_len);
  DS2_REQUIRE(need == 0 || (ws && ws_bytes >= need), "ds2_edit_align_i32: workspace too small (%zu < %zu bytes)", ws_bytes, need);
  DS2_REQUIRE(need == 0 || ((size_t)ws & 15) == 0, "ds2_edit_align_i32: workspace must be 16-byte aligned");
  const size_t col_bytes = (size_t)P * (size_t)((max_len + 63) / 64) * (size_t)max_len * 16;
  const long long h_stride = max_len > 64 ? (long long)align_up((size_t)max_len, 64) : 0;
  const unsigned grid = (unsigned)(((long long)P + EA_WAVES - 1) / EA_WAVES);
  hipLaunchKernelGGL(edit_align_kernel, dim3(grid), dim3(64 * EA_WAVES), 0, (hipStream_t)stream, seq, n_seq, a_off, a_len, b_off, b_len,
                     P, max_len, (ulonglong2*)ws, (signed char*)ws + col_bytes, h_stride, counts, a_map, b_map);
  DS2_LAUNCH_CHECK("edit_align_kernel");
  return 0;
}
