// Sizes of the recurrence's workspaces: plain host arithmetic (no HIP), stated ONCE.  A persistent launcher takes its exchange bytes from the
// function of its kernel family below, ds2_rnn_*_workspace_bytes take the largest over the families a shape can reach, and the launch tail
// (persist_arm, rnn.hip) refuses a fill that would not fit the workspace it was given — so a family cannot overwrite memory behind a
// workspace because one side restated a size differently.
#pragma once
#include <stddef.h>
#include <algorithm>

namespace rnn_sizes {

constexpr size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }

// operand mode: of a WORKSPACE query, the entry's `bf16` argument (0 fp32, 1 bf16, 2 fp32 mode with the split kernels first and the fp32
// kernels as fallback); of a KERNEL FAMILY's exchange, the operands of the instance (2 = split: a hi and a lo bf16 plane per buffer)
enum { OP_F32 = 0, OP_BF16 = 1, OP_SPLIT = 2 };
constexpr size_t planes(int op) { return op == OP_SPLIT ? 2 : 1; }
constexpr size_t kchunk_of(int op) { return op == OP_F32 ? 16 : 32; }

constexpr size_t CENSUS_BYTES = 64;                       // 8 per-XCD slot counters, the arrival counter, one "unexpected XCC id" flag

// shapes the K-split backward / the 10-unit-slice forward exist for (G = 3 / 4 only: ksplit_avail / u10_avail in rnn.hip)
inline bool ksplit_shape_ok(int H) { return H >= 256 && (H % 256) == 0 && H <= 1280; }
// whole 32-unit chunks, whole 10-unit slices, at most one workgroup per CU for both directions of one batch tile, at most five chunks per wave
inline bool u10_shape_ok(int H) { return H >= 160 && (H % 160) == 0 && H <= 1280; }

// bytes of ONE packed exchange buffer of the all-gather recurrences ([2 dirs][tiles][chunks][1 KiB]) over a kdim-wide operand
inline size_t xbuf_bytes(int B, int kdim, size_t kchunk) { return (size_t)2 * (cdiv(B, 32) * 2) * cdiv(kdim, kchunk) * 1024; }
// bytes of the two exchange slots of the K-split backward: [2 slots][2 dirs x batch tiles][gs consumers][8 waves][gs producers][128 B]
inline size_t ksplit_xbuf_bytes(int B, int H) { const size_t gs = (size_t)H / 32; return (size_t)2 * 2 * cdiv(B, 16) * gs * gs * 1024; }

// ---- exchange bytes per persistent kernel family (without the census words behind them)
// forward all-gather (rnn_fwd_persistent_kernel): four round-robin buffers of h
inline size_t fwd_allgather_xbytes(int B, int H, int op) { return 4 * planes(op) * xbuf_bytes(B, H, kchunk_of(op)); }
// forward, 10-unit slices (rnn_fwd_u10_kernel): the split kernel's four buffers of two planes
inline size_t fwd_u10_xbytes(int B, int H) { return fwd_allgather_xbytes(B, H, OP_SPLIT); }
// backward all-gather (rnn_bwd_persistent_kernel): four round-robin buffers of the G*H-wide dGh
inline size_t bwd_allgather_xbytes(int gates, int B, int H, int op) { return 4 * planes(op) * xbuf_bytes(B, gates * H, kchunk_of(op)); }
// backward K-split (rnn_bwd_ksplit_kernel): two slots of partial dh, per plane
inline size_t bwd_ksplit_xbytes(int B, int H, int op) { return planes(op) * ksplit_xbuf_bytes(B, H); }

// the step kernels' two ping-pong buffers, in bytes (1 chunk = 1 KiB in both precisions)
inline size_t step_bytes(int B, int kdim, int op) { return (size_t)2 * 2 * (cdiv(B, 32) * 2) * cdiv(kdim, kchunk_of(op)) * 1024; }
// the backward recurrence's carry in front of its exchange buffers: (4, B, H) fp32
inline size_t bwd_carry_bytes(int B, int H) { return (size_t)4 * B * H * sizeof(float); }

// mode 2 tries the split kernels first and falls back to the fp32 ones: the workspace serves both
inline size_t fwd_workspace_bytes(int B, int H, int mode) {
  size_t pers = fwd_allgather_xbytes(B, H, mode == OP_BF16 ? OP_BF16 : OP_F32);
  if (mode == OP_SPLIT) pers = std::max(pers, fwd_allgather_xbytes(B, H, OP_SPLIT));
  if (mode == OP_SPLIT && u10_shape_ok(H)) pers = std::max(pers, fwd_u10_xbytes(B, H));
  return std::max(step_bytes(B, H, mode == OP_BF16 ? OP_BF16 : OP_F32), pers + CENSUS_BYTES);
}
inline size_t bwd_workspace_bytes(int gates, int B, int H, int mode) {
  size_t pers = bwd_allgather_xbytes(gates, B, H, mode == OP_BF16 ? OP_BF16 : OP_F32);
  if (mode == OP_SPLIT) pers = std::max(pers, bwd_allgather_xbytes(gates, B, H, OP_SPLIT));
  if ((mode == OP_BF16 || mode == OP_SPLIT) && gates != 1 && ksplit_shape_ok(H)) pers = std::max(pers, bwd_ksplit_xbytes(B, H, mode));
  return bwd_carry_bytes(B, H) + std::max(step_bytes(B, gates * H, mode == OP_BF16 ? OP_BF16 : OP_F32), pers + CENSUS_BYTES);
}

}  // namespace rnn_sizes
