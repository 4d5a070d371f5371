/* libds2hip — C ABI of the MI355X-native (gfx950) DeepSpeech2 train-step kernels.
 *
 * Drop-in boundary for the hot path of zakuro-ai/asr (`asr_deepspeech`).  The reference has no FFI
 * of its own (it is pure Python over torch ops); each entry point below replaces the torch/ATen op
 * sequence at the cited reference call site (paths relative to the reference tree).  The Python
 * host layer `asr_amd/` binds these with ctypes (see INTEGRATION.md for the stub a maintainer of
 * the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`; the library never
 *     allocates, frees or retains memory: caller owns inputs, outputs, saved tensors, workspaces.
 *   - `stream` is a hipStream_t (as void*); all work is enqueued asynchronously on it.
 *   - return 0 on success, negative on error; `ds2_last_error()` returns a thread-local message.
 *   - threading: the library keeps NO mutable global state besides that thread-local message.  Everything the recurrence entry points
 *     remember between calls (which kernel family the last call took, the cooldown after a starved persistent launch, the enable
 *     switches, the debug selectors, where the starvation record and the poison word live) is in a caller-owned `ds2_rnn_ctx`
 *     (below); one context per thread / stream that launches recurrences, calls on different contexts are independent.  Environment
 *     switches (DS2_*) are tuning / A-B overrides read once and never written.
 *   - all tensors fp32, row-major, contiguous unless a pitch (`ld*`) is given.
 *   - lengths (`lens_dev`) are int32 per-sample valid OUTPUT frame counts (after the conv stack,
 *     modules/deepspeech.py:275-288), sorted descending as the reference requires (blocks.py:87).
 */
#ifndef DS2HIP_H
#define DS2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ds2_version(void);
const char* ds2_last_error(void);
int ds2_device_info(int* cu_count, int* wave_size, char* arch, int arch_len);
int ds2_ablation_build(void);

/* ---- caller-owned state of the recurrence entry points (modules/blocks.py:84-93 is stateless in the reference: aten::gru / aten::lstm) ----
 * The caller allocates the struct (any memory it owns), zeroes it and calls ds2_rnn_ctx_init with
 *   status_dev   device memory, 8 ints, zero-initialised: the starvation record of persistent launches made through this context
 *   poison_host / poison_dev   optional (both NULL, or both set): host and device address of ONE pinned, mapped int that
 *                ds2_rnn_poison_if_starved raises — lets a caller that never synchronises notice a starved launch with a host read.
 * The library never allocates any of it and holds no reference beyond the call it is passed to.  ctx == NULL is accepted by the launch
 * entry points: the recurrence then runs on the one-launch-per-step kernels (no persistent launch: nothing to remember, nothing to record). */
typedef struct ds2_rnn_ctx {
  int size;                 /* sizeof(ds2_rnn_ctx) of the build that initialised it (ABI check) */
  int persist_fwd, persist_bwd;   /* which recurrences may run as ONE persistent launch (ds2_rnn_persistent_enable) */
  int cooldown;             /* recurrence calls left on the one-launch-per-step kernels after a starved launch (0 armed, < 0 never re-arm) */
  int rearm_calls;          /* length of that cooldown (default 64 calls; 0 = never re-arm); DS2_RNN_REARM_CALLS at init */
  int starved_total;        /* launches through this context that starved (reporting) */
  int last_path;            /* out: bits describing what the last forward / backward call launched (ds2_rnn_last_path) */
  int last_bwd_kind;        /* out: 0 step kernels, 1 all-gather persistent, 2 K-split persistent */
  int debug_flags;          /* kernel-family selectors (ds2_debug_flags) */
  int reserved[7];
  int* status_dev;
  int* poison_host;
  int* poison_dev;
} ds2_rnn_ctx;
int ds2_rnn_ctx_init(ds2_rnn_ctx* ctx, int* status_dev, int* poison_host, int* poison_dev);
/* hipMemsetAsync through the C ABI.  Workspace pre-arming: the recurrence entries that take a trailing `ws_armed` skip a persistent launch's
 * own fill of the exchange buffers — which otherwise sits between the projection GEMM and the launch that needs every CU — when it is 1: the
 * caller promises that it has filled THIS call's whole workspace with 0xff bytes earlier in the stream.  The promise belongs to the one call
 * it is passed to (an argument, not state of the context: two threads driving one context cannot hand it to each other's calls). */
int ds2_memset_async(void* dst, int value, size_t bytes, void* stream);
/* Kernel-family selectors of the recurrence (every selection computes the full result; used by the parity tests and A/B scripts):
 * 8 / 16 alternative tile shapes of the wide step kernels, 64 one launch per time step instead of the persistent kernels, 128 the
 * all-gather persistent backward kernel instead of the K-split one.  Returns the previous value; 0 = production.  Bits 1 / 2 (skip the
 * recurrent product / the gate epilogue, scripts/ablate_rnn.py) are honoured only by a library built with -DDS2_ABLATE
 * (ds2_ablation_build() == 1); the shipped library masks them off. */
int ds2_debug_flags(ds2_rnn_ctx* ctx, int flags);

/* ---- dense GEMM on the f32 matrix cores -------------------------------------------------------
 * C[M,N] (+)= op(A) op(B) (+ bias[N]);  transA: A stored (K,M);  transB: B stored (N,K).
 * Replaces aten::addmm/mm inside aten::gru / aten::lstm (input projections, modules/blocks.py:76-78,88),
 * nn.Linear (modules/deepspeech.py:105) and their autograd backward (dX, dW).
 * batch > 1: strided batches; splitk > 1: deterministic split-K through `workspace`. */
size_t ds2_gemm_f32_workspace_bytes(int M, int N, int batch, int splitk);
int ds2_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, int lda, long long strideA, const float* B, int ldb,
                 long long strideB, float* C, int ldc, long long strideC, const float* bias, int accumulate, int batch, int splitk,
                 void* workspace, size_t workspace_bytes, void* stream);

/* bf16-operand / fp32-accumulate GEMM (v_mfma_f32_32x32x16_bf16), "NT" form only: C[M,N] (+)= A[M,K] B[N,K]^T (+bias).
 * Used for the RNN input projections and their dX / dW when the model runs with precision="bf16" (BASELINE configs[2],[4]);
 * the cast passes produce the K-contiguous bf16 operands (dst pitch % 8 == 0, pad columns zero-filled). */
size_t ds2_gemm_bf16_workspace_bytes(int M, int N, int batch, int splitk);
int ds2_gemm_bf16_nt(int M, int N, int K, const void* A, int lda, long long strideA, const void* B, int ldb, long long strideB, float* C,
                     int ldc, long long strideC, const float* bias, int accumulate, int batch, int splitk, void* workspace,
                     size_t workspace_bytes, void* stream);
/* C[M,N] **bf16** = A[M,K] B[N,K]^T + bias (fp32 accumulation and bias add, ONE rounding at the store; ldc in bf16 elements, N, ldc % 8 == 0):
 * the x-projections of a recurrent layer in the bf16 training mode (aten::addmm inside aten::gru / lstm, blocks.py:76-78, 88), read once by
 * ds2_rnn_fwd_x.  Returns 1 — nothing launched, call ds2_gemm_bf16_nt — where the four-wave kernel does not apply (K % 64 != 0, fewer
 * 256 x 256 tiles than CUs, alignment); 0 = launched; < 0 = error. */
int ds2_gemm_bf16_nt_obf16(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc, const float* bias, void* stream);
/* n contiguous bf16 -> fp32 (n % 8 == 0, 16-byte aligned bases). */
int ds2_cast_f32_from_bf16(const void* src, float* dst, long long n, void* stream);
/* "TN" form: C[M,N] (+)= A[K,M]^T B[K,N], both operands bf16 row-major with the reduction index on the rows (pitches lda / ldb).
 * The weight-gradient product of the recurrent layers (dW = dGx^T [Xn | h], K = T*B) without a transposed copy of any operand.
 * M, N, lda, ldb, strides multiples of 8; batch > 1: independent products at the given element strides (may be negative). */
int ds2_gemm_bf16_tn(int M, int N, int K, const void* A, int lda, long long strideA, const void* B, int ldb, long long strideB, float* C,
                     int ldc, long long strideC, int accumulate, int batch, int splitk, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Grouped TN products in ONE launch of a kernel sized to run BESIDE a persistent backward recurrence (4 waves of <= 128 registers, at most
 * one workgroup per CU): all weight-gradient products of one recurrent layer — dW_hh of both directions, a GRU's n-gate rows, dW_ih
 * (asr_deepspeech/modules/blocks.py:76-78,88 under autograd) — as one flat list of 128 x 128 tiles walked by one workgroup per CU; every
 * tile is a full reduction over K_p (no split-K, no workspace).  Same operand rules as ds2_gemm_bf16_tn; up to 8 problems. */
typedef struct ds2_tn_problem {
  const void* A; const void* B; float* C;
  int M, N, K, lda, ldb, ldc;
} ds2_tn_problem;
int ds2_gemm_bf16_tn_group(int nprob, const ds2_tn_problem* problems, int max_workgroups, void* stream);
/* The same problem list through the 256 x 256 TN kernel with ONE split-K factor for all of them: one GEMM launch whose work items are
 * (problem, K slice, tile) — a layer's 192 weight-gradient tiles x 4 slices are 768 equal items = three full rounds of the chip, where
 * three separate launches each had their own ramp and tail and up to 8 slabs per tile — and one reduce launch.  workspace: the partial slabs
 * of the split products, nothing else (ds2_gemm_bf16_tn_splitk_group_workspace_bytes: an upper bound).
 * Consecutive problems that name the SAME C are TERMS of one product and are summed (the fp32 mode's hi.hi + hi.lo + lo.hi on views of
 * split operands, ds2_split_bf16): up to 16 entries per launch. */
size_t ds2_gemm_bf16_tn_splitk_group_workspace_bytes(int nprob, const ds2_tn_problem* problems, int splitk);
int ds2_gemm_bf16_tn_splitk_group(int nprob, const ds2_tn_problem* problems, int splitk, void* workspace, size_t workspace_bytes, void* stream);
/* ds2_gemm_bf16_tn_splitk_group with an epilogue on product ep_index, applied by the reduce launch: C = (A^T B) diag(scale) + rowv (x) shift
 * (scale / shift: N floats, 16-byte aligned; rowv: M floats) — dW_ih of a projection whose BatchNorm1d was folded into it (ds2_wih_fold_bf16).
 * Returns 1, nothing launched, when that product would have a single slab: use the plain entry + ds2_scale_rank1_f32. */
int ds2_gemm_bf16_tn_splitk_group_ep(int nprob, const ds2_tn_problem* probs, int splitk, int ep_index, const float* ep_scale, const float* ep_rowv,
                                     const float* ep_shift, void* workspace, size_t workspace_bytes, void* stream);
int ds2_cast_bf16(const float* src, int ld_src, void* dst, int ld_dst, int R, int Cc, void* stream);
/* fp32 mode (precision="fp32", BASELINE configs[1],[3]), large GEMMs: every fp32 operand is SPLIT into two bf16 terms, x = hi + lo with
 * hi = bf16(x), lo = bf16(x - hi) (x is represented to 2^-18 relative), and a product is taken as a_hi b_hi + a_hi b_lo + a_lo b_hi on the bf16
 * matrix cores with fp32 accumulation (the dropped lo.lo term is 2^-18 of the product; the result is within ~1e-5 of the fp32 product,
 * two orders inside north_star's 1e-3) — torch.nn.functional.linear / autograd's mm (blocks.py:76-78,88) at ~5x the fp32-MFMA roof.
 * dst (R, ld_dst) bf16 = blocks of pad8(C) columns each: order 0 [hi | hi | lo] (A operand), 1 [hi | lo | hi] (B operand: one NT product
 * over a reduction index 3 pad8(C) long IS the three-term product), 2 [hi | lo] (TN products take row-pitched views of the blocks). */
int ds2_split_bf16(const float* src, int ld_src, void* dst, int ld_dst, int R, int Cc, int order, void* stream);
int ds2_cast_transpose_bf16(const float* src, int ld_src, void* dst, int ld_dst, int R, int Cc, void* stream);
/* both copies from ONE read of src: dst_r (R, ld_r) = bf16(src) (NULL: skipped), dst_t (C, ld_t) = bf16(src)^T, pads zero
 * (ld_r % 8 == 0, C <= ld_r <= C rounded up to a multiple of 64; ld_t % 8 == 0, ld_t >= R); colsum (C) optional: column sums of src from the same read
 * (the bias gradient db_ih = sum_rows dGx), then ws >= ds2_cast_bf16_both_workspace_bytes(R, C) */
size_t ds2_cast_bf16_both_workspace_bytes(int R, int Cc);
int ds2_cast_bf16_both(const float* src, int ld_src, void* dst_r, int ld_r, void* dst_t, int ld_t, int R, int Cc, float* colsum, void* ws,
                       size_t ws_bytes, void* stream);
/* bf16 (R, C) row-major (pitch ld_src % 8 == 0) -> bf16 (C, ld_t) transposed, pads zero; colsum (C) fp32 optional: column sums from
 * the same read (ws >= ds2_cast_bf16_both_workspace_bytes(R, C)). */
int ds2_transpose_bf16(const void* src, int ld_src, void* dst_t, int ld_t, int R, int Cc, float* colsum, void* ws, size_t ws_bytes,
                       void* stream);

/* ---- BatchNorm1d over (T*B, H) rows, padding rows included -----------------------------------
 * modules/blocks.py:75,85-86 (SequenceWise(BatchNorm1d)) and modules/deepspeech.py:104 (fc block).
 * stats: biased variance for normalisation; running stats updated with momentum and the unbiased
 * variance when run_mean/run_var are non-null (torch.nn.BatchNorm1d training semantics). */
size_t ds2_colreduce_workspace_bytes(int M, int H);
int ds2_colstats_f32(const float* X, int ldx, int M, int H, float* mean, float* var, float* run_mean, float* run_var, float momentum,
                     void* ws, size_t ws_bytes, void* stream);
/* Y = Xa + Xb (sum of the two RNN directions, modules/blocks.py:92) fused with the statistics of Y */
int ds2_add_colstats_f32(const float* Xa, int lda, const float* Xb, int ldb, float* Y, int ldy, int M, int H, float* mean, float* var,
                         float* run_mean, float* run_var, float momentum, void* ws, size_t ws_bytes, void* stream);
int ds2_colsum_f32(const float* X, int ldx, int M, int H, float* sum, float* sumsq, void* ws, size_t ws_bytes, void* stream);
int ds2_bn1d_apply_f32(const float* X, int ldx, float* Y, int ldy, int M, int H, const float* mean, const float* var,
                       const float* gamma, const float* beta, float eps, void* stream);
/* same, Y written as bf16 (M, ldy), ldy % 8 == 0, pad columns zero: feeds the bf16 input-projection GEMM without a cast pass */
int ds2_bn1d_apply_bf16(const float* X, int ldx, void* Y, int ldy, int M, int H, const float* mean, const float* var, const float* gamma,
                        const float* beta, float eps, void* stream);
/* (dX may be NULL: only the column sums dgamma / dbeta are produced — see ds2_rnn_bwd_bn) */
int ds2_bn1d_bwd_f32(const float* dY, int lddy, const float* X, int ldx, float* dX, int lddx, int M, int H, const float* mean,
                     const float* var, const float* gamma, float eps, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                     void* stream);

/* ---- BatchNorm1d folded into the input projection of the recurrent layer behind it (bf16 training mode, round 6) --------------------------
 * blocks.py:85-86 (SequenceWise(BatchNorm1d)) + :92 (direction sum of the layer in front) + aten::addmm inside aten::gru / lstm (:88).
 * y = Xa + Xb is never written.  ds2_center_colstats writes the CENTRED sum yc = y - m0 as the bf16 GEMM operand (M, ldyc; pad columns
 * zero), m0 = the column means of y taken from hsum (2, ntiles, H: ds2_rnn_fwd_x), and returns the batch statistics of y (mean, biased var:
 * what nn.BatchNorm1d computes; running statistics updated with momentum and the unbiased variance) plus delta = mean - m0, the mean of yc.
 * ds2_wih_fold_bf16 then folds the normalisation into the projection:  BN(y) W^T + b = yc (W diag(s))^T + (b + W c),
 * s = gamma rsqrt(var + eps), c = beta - delta s: W2 = bf16(W diag(s)) (R rows, pitch ldw2), bias2 = b + W c in fp32, colscale = s, colshift = c.
 * Backward: the weight gradient of the folded projection is dW = (dGx^T yc) diag(s) + db (x) c (ds2_scale_rank1_f32 on the TN product);
 * the BatchNorm backward formulas hold on (yc, delta, var) unchanged — ds2_bn1d_bwd_xbf16 / ds2_rnn_bwd_bn_xbf16 take the bf16 operand.
 * workspace of ds2_center_colstats: ds2_colreduce_workspace_bytes(M, H) + H * sizeof(float). */
int ds2_center_colstats(const float* Xa, int lda, const float* Xb, int ldb, const float* hsum, int ntiles, void* Yc_bf16, int ldyc, int M, int H,
                        float* mean, float* var, float* delta, float* run_mean, float* run_var, float momentum, void* ws, size_t ws_bytes,
                        void* stream);
int ds2_wih_fold_bf16(const float* W, int ldw, const float* bias, int R, int I, const float* var, const float* gamma, const float* beta,
                      const float* delta, float eps, void* W2_bf16, int ldw2, float* bias2, float* colscale, float* colshift, void* stream);
/* C[r][c] = C[r][c] * scale[c] + rowv[r] * shift[c], (R, N) fp32 in place (N, ldc % 4 == 0, 16-byte aligned) */
int ds2_scale_rank1_f32(float* C, int ldc, int R, int N, const float* scale, const float* rowv, const float* shift, void* stream);
/* ds2_bn1d_bwd_f32 with the BatchNorm input as bf16 (pitch ldx % 4 == 0; dX, when given, needs H % 4 == 0); `mean` = the mean of X itself */
int ds2_bn1d_bwd_xbf16(const float* dY, int lddy, const void* X_bf16, int ldx, float* dX, int lddx, int M, int H, const float* mean, const float* var,
                       const float* gamma, float eps, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm2d + Hardtanh(0,20) + MaskConv time mask on (B,C,D,T) ----------------------------
 * modules/deepspeech.py:62-63,65-66 under modules/blocks.py:48-55 (mask after EVERY sub-module). */
size_t ds2_chanreduce_workspace_bytes(int C);
int ds2_bn2d_stats_f32(const float* Y, int B, int C, int D, int T, float* mean, float* var, float* run_mean, float* run_var,
                       float momentum, void* ws, size_t ws_bytes, void* stream);
int ds2_bn2d_act_fwd_f32(const float* Y, float* A, int B, int C, int D, int T, const int* lens_dev, const float* mean,
                         const float* var, const float* gamma, const float* beta, float eps, void* stream);
int ds2_bn2d_act_bwd_f32(const float* Y, const float* dA, float* dY, int B, int C, int D, int T, const int* lens_dev, const float* mean,
                         const float* var, const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, void* ws,
                         size_t ws_bytes, void* stream);

/* bf16 mode: the same two blocks with the layout casts that follow them fused into the pass (deepspeech.py:62-66 + the operand
 * preparation of conv2 forward / dgrad / wgrad): each result may be written as fp32 (B,32,D,T), as zero-padded bf16 rows
 * (B,32,D,Tp), Tp = ds2_conv_padded_pitch(T), and as channels-last bf16 (B,D,T,32) — NULL skips a form.  The backward form also
 * returns dbias (32) = per-channel sums of dY, the gradient of the bias of the convolution in front (deepspeech.py:61,64). */
int ds2_bn2d_act_fwd_fused(const float* Y, int B, int D, int T, const int* lens_dev, const float* mean, const float* var,
                           const float* gamma, const float* beta, float eps, float* a_f32, void* a_pad, void* a_nhwc, void* stream);
/* second conv stage, bf16 mode: the same block fused with the (B,32*D,T) -> (T*B, 32*D) collapse (deepspeech.py:135-137) and the cast to
 * the first recurrent layer's bf16 GEMM operand; x_f32 (pitch 32*D) and x_bf16 (pitch ld_bf >= 32*D, a multiple of 8; the columns behind
 * 32*D are written as zeros) may each be NULL */
int ds2_bn2d_act_collapse(const float* Y, int B, int D, int T, const int* lens_dev, const float* mean, const float* var,
                          const float* gamma, const float* beta, float eps, float* x_f32, void* x_bf16, int ld_bf, void* stream);
size_t ds2_bn2d_act_bwd_fused_workspace_bytes(int B, int D, int T);
int ds2_bn2d_act_bwd_fused(const float* Y, const float* dA, int B, int D, int T, const int* lens_dev, const float* mean,
                           const float* var, const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta,
                           float* dbias, float* dy_f32, void* dy_pad, void* dy_nhwc, void* ws, size_t ws_bytes, void* stream);
/* dir 0: (B,F,T) -> (T,B,F) = view+transpose+contiguous of modules/deepspeech.py:135-137; dir 1: inverse */
int ds2_transpose_bft_f32(const float* src, float* dst, int B, int F, int T, int dir, void* stream);
int ds2_transpose2d_f32(const float* src, int ld_src, long long stride_src, float* dst, int ld_dst, long long stride_dst, int R, int Cc,
                        int batch, void* stream);

/* ---- conv front-end (MFMA implicit GEMM) -------------------------------------------------------
 * conv1 = nn.Conv2d(1,32,(41,11),(2,2),(20,5)) modules/deepspeech.py:61; conv2 = nn.Conv2d(32,32,(21,11),(2,1),(10,5)) :64;
 * forward epilogues add the bias and apply the MaskConv mask (modules/blocks.py:50-55). */
void ds2_conv_dims(int F, int Tin, int* D1, int* D2, int* T);
size_t ds2_conv_packed_floats(int which /*0: conv1 fwd, 1: conv2 fwd, 2: conv2 dgrad*/);
int ds2_conv_pack_f32(const float* w1, const float* w2, float* wpk1, float* wpk2, float* wpk2d, void* stream);
int ds2_conv1_fwd_f32(const float* x, const float* wpk1, const float* bias, const int* lens_dev, float* y1, int B, int F, int Tin,
                      void* stream);
int ds2_conv2_fwd_f32(const float* a1, const float* wpk2, const float* bias, const int* lens_dev, float* y2, int B, int D1, int T,
                      void* stream);
int ds2_conv2_dgrad_f32(const float* dy2, const float* wpk2d, float* da1, int B, int D1, int T, void* stream);
size_t ds2_conv_wgrad_workspace_bytes(int which /*0: conv1, 1: conv2*/, int B, int F);
int ds2_conv1_wgrad_f32(const float* x, const float* dy1, const int* lens_dev, float* dW1, int B, int F, int Tin, int accumulate, void* ws,
                        size_t ws_bytes, void* stream);
int ds2_conv2_wgrad_f32(const float* a1, const float* dy2, const int* lens_dev, float* dW2, int B, int D1, int T, int accumulate, void* ws,
                        size_t ws_bytes, void* stream);

/* conv2 forward / data-gradient with bf16 MFMA operands (precision="bf16"): activations channels-last (B,D,T,32) bf16
 * (ds2_nhwc_bf16_f32 converts from the (B,32,D,T) fp32 layout), weights re-packed by ds2_conv2_pack_bf16; fp32 output. */
size_t ds2_conv2_bf16_packed_bytes(int which /*0: forward, 1: dgrad even rows, 2: dgrad odd rows*/);
int ds2_conv2_pack_bf16(const float* w2, void* wf, void* wd0, void* wd1, void* stream);
int ds2_nhwc_bf16_f32(const float* src, void* dst, int B, int D, int T, void* stream);
int ds2_conv2_fwd_bf16(const void* a1_nhwc, const void* wf, const float* bias, const int* lens_dev, float* y2, int B, int D1, int T,
                       void* stream);
int ds2_conv2_fwd_bf16_stat_blocks(int B, int D1, int T);
int ds2_conv2_fwd_bf16_stats(const void* a1_nhwc, const void* wf, const float* bias, const int* lens_dev, float* y2, int B, int D1, int T,
                             float* stat_part, void* stream);
size_t ds2_chanstats_from_partials_workspace_bytes(void);
int ds2_chanstats_from_partials(const float* part, int nblk, int C, double count, float* mean, float* var, float* run_mean, float* run_var,
                                float momentum, void* ws, size_t ws_bytes, void* stream);
int ds2_conv2_dgrad_bf16(const void* dy2_nhwc, const void* wd0, const void* wd1, float* da1, int B, int D1, int T, void* stream);

/* conv2 weight gradient with bf16 MFMA operands: zero-padded bf16 copies (R, Tp) of the (B,32,D,T) tensors, Tp = ds2_conv_padded_pitch(T) */
int ds2_conv_padded_pitch(int T);
int ds2_padcast_bf16(const float* src, void* dst, long long R, int T, void* stream);
size_t ds2_conv2_wgrad_bf16_workspace_bytes(int B, int D1);
int ds2_conv2_wgrad_bf16(const void* a1p, const void* dy2p, const int* lens_dev, float* dW2, int B, int D1, int T, void* ws, size_t ws_bytes,
                         void* stream);
/* The same weight gradient from the CHANNELS-LAST bf16 operands the conv2 forward / data-gradient kernels already take (a1 (B,D1,T,32),
 * dy2 (B,D2,T,32)): no padded copies, operands go global -> LDS by DMA and the kernel-tap shift is a row offset of the time-major LDS image
 * (Conv2d weight gradient under loss.backward(), modules/deepspeech.py:64 / trainers/deepspeech_trainer.py:87).  Workspace: as above. */
int ds2_conv2_wgrad_nhwc_bf16(const void* a1_nhwc, const void* dy2_nhwc, const int* lens_dev, float* dW2, int B, int D1, int T, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- bidirectional GRU / LSTM / tanh-RNN recurrence ----------------------------------------------
 * pack_padded_sequence -> aten::gru / aten::lstm / aten::rnn_tanh -> pad_packed_sequence, modules/blocks.py:87-89, h0 = 0,
 * gate order r,z,n (GRU) / i,f,g,o (LSTM); gates = 3 | 4 | 1 (nn.RNN, tanh: h_t = tanh(x W_ih^T + b_ih + h W_hh^T + b_hh)).
 * gates = 1: h is the whole saved-for-backward state — aux may be NULL and is never touched, gates_bf16 is ignored (no record), the forward
 * leaves gx as it is (the x-projections) and the backward writes dGx = d(pre-activation) into gx or dgx_bf16 (gx may be NULL when
 * dgx_bf16 is given).  The K-split backward and the ten-unit-slice forward have no gates = 1 instance (the K-split footprint reports 0).
 * See asr_amd/csrc/rnn.hip for buffer roles. */
size_t ds2_rnn_packed_bytes(int gates, int H, int which /*0: forward operand, 1: backward operand*/, int bf16);
/* re-pack W_hh = [weight_hh_l0 ; weight_hh_l0_reverse] (2,G*H,H) fp32 into MFMA-fragment order, fp32 or bf16 fragments
 * (once per optimizer step).  bf16 = 2 (here, in ds2_rnn_packed_bytes, ds2_rnn_fwd_workspace_bytes and ds2_rnn_fwd*): the fp32 mode with the
 * SPLIT persistent forward recurrence — h_t and W_hh each as two bf16 planes, x = bf16(x) + bf16(x - bf16(x)), product = hi.hi + lo.hi + hi.lo on
 * the bf16 matrix cores with fp32 accumulation (fp32-grade: ~1e-6 of the fp32 kernels, far inside north_star's 1e-3): the forward operand
 * is then [fp32 fragments | hi fragments | lo fragments (| the ten-unit-slice hi / lo operand of csrc/rnn_fwd_u10.h when H % 160 == 0, H <= 1280)]
 * and the fp32 kernels remain the fallback (shape does not fit, cooldown). */
int ds2_rnn_pack_whh(int gates, const float* whh, void* wp_fwd, void* wp_bwd, int H, int bf16, void* stream);
/* The bf16 weight operands of a whole recurrent stack in ONE launch (bf16 mode, once per optimizer step): per layer the packed W_hh
 * fragments of ds2_rnn_pack_whh with bf16 = 1 and the bf16 copies of W_ih that ds2_cast_bf16_both / ds2_cast_transpose_bf16 write, byte
 * for byte, into the caller's buffers.  whh NULL: no W_hh work for that layer; wih NULL: no W_ih work; wih_r NULL: only the transposed
 * copy.  whh (2, gates*H, H) contiguous, H % 4 == 0; wih (R, Cc) with row pitch ld_wih; wih_t (Cc, ld_t), ld_t % 8 == 0, ld_t >= R;
 * wih_r (R, ld_r), ld_r % 8 == 0, Cc <= ld_r <= the next multiple of 64; pad columns are zero-filled; all buffers 16-byte aligned. */
typedef struct ds2_prep_layer {
  const float* whh; void* wp_fwd; void* wp_bwd;
  const float* wih; void* wih_t; void* wih_r;
  int gates, H, R, Cc, ld_wih, ld_t, ld_r, reserved;
} ds2_prep_layer;
int ds2_weight_prep_bf16(const ds2_prep_layer* layers, int n, void* stream);
/* Status of the persistent recurrences (a layer's whole recurrence in ONE launch whose workgroups exchange h_t / dGh_t through memory;
 * it needs every workgroup resident at once).  out8 = {starved, slice | workgroup, tile | XCD, direction | kind, step, wave, pending
 * chunk mask, L2-local exchange}: starved != 0 (1 forward, 2 backward, 3 the launch never became resident) means a wave gave up
 * polling since the last call (DS2_RNN_SPIN_LIMIT polls, default 2^20 ~ 1 s) and the results of that launch are invalid — the caller
 * must treat the step as failed.  Synchronises the device and clears the record.  After a starved launch the next DS2_RNN_REARM_CALLS
 * (default 64) recurrence calls run on the one-launch-per-step kernels, then the persistent kernels are armed again.
 * DS2_RNN_PERSISTENT=0 selects the one-launch-per-step kernels from the start; DS2_RNN_XCD_LOCAL=0 keeps the placement-independent
 * (sc1) exchange instead of the exchange through the group's own L2 (asr_amd/csrc/rnn.hip: persist_role). */
int ds2_rnn_persistent_status(ds2_rnn_ctx* ctx, int* out8);
/* reporting: out2 = {launches through this context that starved, recurrence calls left before the persistent kernels are armed
 * again (0 = armed, -1 = never)} */
int ds2_rnn_persistent_counters(const ds2_rnn_ctx* ctx, int* out2);
/* Inference path (DeepSpeech.forward in eval mode, modules/deepspeech.py:130-149): instead of a device synchronisation per forward, a
 * kernel in stream order that overwrites buf[0..n) (the logits) with NaN if a persistent launch before it recorded starvation; the record is
 * neither read by the host nor cleared (the next ds2_rnn_persistent_status, at a natural sync point, raises). */
int ds2_rnn_poison_if_starved(ds2_rnn_ctx* ctx, float* buf, size_t n, void* stream);
/* 1 if a ds2_rnn_poison_if_starved kernel has fired since the last ds2_rnn_persistent_status: a read of a pinned host word the kernel
 * sets, no synchronisation and no device call.  Lets inference callers that only ever call forward (deepspeech.py:130-149 in eval mode)
 * notice a starved launch and settle it (status call: report, clear, cooldown onto the step kernels) before their next forward. */
int ds2_rnn_poison_seen(const ds2_rnn_ctx* ctx);
/* device-side validity of the train step enqueued so far, evaluated when the kernel RUNS (stream order): flag_dev[0] = -1 if a persistent
 * recurrence launch starved, else 1 if the loss is finite and >= 0 [check_loss, functional.py:45-61], else 0.  Under data parallelism the
 * MIN over ranks is taken; the gated optimizer applies the update only for 1. */
int ds2_rnn_step_gate(const ds2_rnn_ctx* ctx, const float* loss_dev, int* flag_dev, void* stream);
/* Which recurrences may run as one persistent launch (default both).  Switch the backward one off when other kernels (collectives on a
 * communication stream) run on the device during backward: a persistent launch needs all of its workgroups resident at once. */
int ds2_rnn_persistent_enable(ds2_rnn_ctx* ctx, int forward, int backward);
/* Footprint of one workgroup of the K-split persistent backward recurrence for this (gates, H), read from the loaded binary: out3 =
 * {registers per lane, static LDS bytes, threads}; returns 1 if the shape has such a kernel, 0 if not.  The host side decides with it
 * whether ds2_gemm_bf16_tn_group (4 waves x 128 registers, 84 KB of LDS) fits on a CU BESIDE the recurrence of the layer below
 * (asr_deepspeech/modules/blocks.py:87-89 backward; the weight gradients of blocks.py:76-78 are off its critical path). */
int ds2_rnn_bwd_ksplit_footprint(int gates, int H, int* out3);
/* reporting: which kernel family the last forward and the last backward call through this context took (bench.py labels its roofline with
 * it).  No FWD_* / BWD_* bit: that direction's last call ran on the one-launch-per-step kernels. */
enum {
  DS2_RNN_PATH_FWD_PERSISTENT = 1,  /* forward ran as ONE persistent launch (and produced its optional outputs) */
  DS2_RNN_PATH_BWD_PERSISTENT = 2,  /* backward ran as ONE persistent launch (and produced its optional outputs) */
  DS2_RNN_PATH_BWD_KSPLIT = 4,      /* ... and that launch was the K-split kernel (asr_amd/csrc/rnn_bwd_ksplit.h) */
  DS2_RNN_PATH_BWD_BN_FUSED = 16,   /* ... which applied the BatchNorm1d backward of the layer above on the fly (ds2_rnn_bwd_bn) */
  DS2_RNN_PATH_FWD_SPLIT = 32,      /* fp32 mode (bf16 = 2): a split (hi + lo bf16) persistent forward kernel took the call */
  DS2_RNN_PATH_BWD_SPLIT = 64,      /* fp32 mode: a split backward kernel took the call (without bit 1: the split step kernels) */
  DS2_RNN_PATH_FWD_U10 = 256        /* ... the split forward kernel was the 10-unit-slice one (asr_amd/csrc/rnn_fwd_u10.h) */
};
int ds2_rnn_last_path(const ds2_rnn_ctx* ctx);
size_t ds2_rnn_fwd_workspace_bytes(int B, int H, int bf16);
/* gates_bf16: NULL, or a (T,B,2,H,4) bf16 buffer that receives the saved-for-backward record of every hidden unit as ONE 8-byte
 * store — GRU [r, z, n, W_hn h + b_hn], LSTM [i, f, g, o] — instead of four fp32 stores into gx / aux (gx is then left untouched
 * and, for GRU, aux is not written).  Pass the same buffer to ds2_rnn_bwd. */
int ds2_rnn_fwd(ds2_rnn_ctx* ctx, int gates, float* gx, const void* wp_fwd, const float* bhh, float* hbuf, float* aux, const int* lens_dev, int T, int B,
                int H, int bf16, void* gates_bf16, void* ws, size_t ws_bytes, void* stream);
/* ds2_rnn_fwd plus h_bf16: NULL, or a (T,B,2,H) bf16 buffer that receives a bf16 copy of hbuf (the K-row-major operand of the TN-form
 * dW_hh GEMM).  Written by a PERSISTENT launch only: check ds2_rnn_last_path() & 1 after the call.  ws_armed: see ds2_memset_async (the short
 * forms ds2_rnn_fwd / ds2_rnn_bwd pass 0). */
int ds2_rnn_fwd_ex(ds2_rnn_ctx* ctx, int gates, float* gx, const void* wp_fwd, const float* bhh, float* hbuf, float* aux, const int* lens_dev, int T, int B,
                   int H, int bf16, void* gates_bf16, void* h_bf16, void* ws, size_t ws_bytes, void* stream, int ws_armed);
/* ds2_rnn_fwd_ex for the bf16 TRAINING mode (bf16 operands, packed gate records required) with two more optional operands.
 * gx_bf16: the x-projections as the **bf16** tensor ds2_gemm_bf16_nt_obf16 wrote (same (T,B,2,G*H) layout; half the bytes written by the
 *   projection and read here: aten::gru / aten::lstm of blocks.py:87-89 take them from aten::addmm at full precision — the rounding is part of
 *   the stated bf16-mode tolerance); gx may then be NULL.  Persistent kernels only: the call returns 1 — nothing launched, nothing counted —
 *   when it cannot run as a persistent launch (cooldown, forward kernel switched off, no persistent kernel for the shape); widen with
 *   ds2_cast_f32_from_bf16 and call again with gx.
 * hsum: (2, ceil(B/16), H) fp32, per direction and 16-row batch tile the sums over time of h — the column sums of the layer's output
 *   y = h_fwd + h_bwd (blocks.py:92) without a pass over it; written by a PERSISTENT launch only (ds2_rnn_last_path() & 1); input of
 *   ds2_center_colstats.
 * Returns 0 = done, 1 = see gx_bf16, < 0 = error. */
int ds2_rnn_fwd_x(ds2_rnn_ctx* ctx, int gates, float* gx, const void* gx_bf16, const void* wp_fwd, const float* bhh, float* hbuf, float* aux,
                  const int* lens_dev, int T, int B, int H, void* gates_bf16, void* h_bf16, float* hsum, void* ws, size_t ws_bytes, void* stream,
                  int ws_armed);
size_t ds2_rnn_bwd_workspace_bytes(int gates, int B, int H, int bf16);
/* dgx_bf16: NULL, or a (T,B,2,G*H) bf16 buffer that receives the gradient wrt the x-projections instead of gx (which then keeps
 * the gates): the bf16-mode GEMMs consume it directly.  gates_bf16: NULL, or the packed records written by ds2_rnn_fwd — read
 * instead of gx (and, for GRU, instead of aux, which is then output only: d(W_hn h + b_hn)); gx may be NULL when both are given. */
int ds2_rnn_bwd(ds2_rnn_ctx* ctx, int gates, const float* dy, int lddy, float* gx, float* aux, const float* hbuf, const void* wp_bwd, const int* lens_dev,
                int T, int B, int H, int bf16, void* dgx_bf16, const void* gates_bf16, void* ws, size_t ws_bytes, void* stream);

/* The K-split backward kernel (DS2_RNN_PATH_BWD_KSPLIT in ds2_rnn_last_path() after a backward call; bf16 operands or split form, H a multiple
 * of 256: asr_amd/csrc/rnn_bwd_ksplit.h — bf16 partial sums of dh are exchanged instead of dGh; results equal those of the other kernel
 * families within 4e-3 relative L2 and sit at the same distance from an fp64 recurrence, run-to-run bit-identical).  A K-split launch that
 * is given dhn_bf16 writes ONLY that bf16 copy of d(W_hn h + b_hn), not the fp32 one into aux.
 * ds2_rnn_bwd plus two optional outputs of a PERSISTENT launch (check ds2_rnn_last_path() & 2 after the call; untouched otherwise):
 * dhn_bf16 (GRU): (T,B,2,H) bf16 copy of d(W_hn h + b_hn); bias_part: (B,2,4,H) fp32 per-batch-row sums over time of
 * [d r, d z, d n, d(hn)] (GRU) / [d i, d f, d g, d o] (LSTM) / [d pre, -, -, -] (tanh cell: slot 0 only is written) - their column sums
 * over B are the bias gradients, so no pass over dGx. */
int ds2_rnn_bwd_ex(ds2_rnn_ctx* ctx, int gates, const float* dy, int lddy, float* gx, float* aux, const float* hbuf, const void* wp_bwd, const int* lens_dev,
                   int T, int B, int H, int bf16, void* dgx_bf16, const void* gates_bf16, void* dhn_bf16, float* bias_part, void* ws,
                   size_t ws_bytes, void* stream, int ws_armed);

/* ds2_rnn_bwd_ex for a layer whose output y feeds a BatchNorm1d (SequenceWise(BatchNorm1d) of the next layer, modules/blocks.py:75,85-86, or
 * of the fc block, modules/deepspeech.py:104): dyn = gradient wrt that BatchNorm's OUTPUT, bn_x = its input (= y, pitch ldx), bn_mean /
 * bn_var / bn_gamma its batch statistics and weight, bn_s0 / bn_s1 the column sums of dyn and dyn * xhat (dbeta / dgamma of
 * ds2_bn1d_bwd_f32 called with dX = NULL).  Where the K-split persistent kernel takes the call it applies the elementwise half of the
 * BatchNorm backward on the fly (ds2_rnn_last_path() & 16) and dy_scratch is not touched; otherwise dy is materialised into dy_scratch
 * (T*B, H) and the call proceeds as ds2_rnn_bwd_ex.  dy_scratch may be NULL: the call then returns 1 — nothing launched, nothing counted —
 * when the buffer is needed after all, and the caller repeats it with one (the fused launch never allocates or touches (T*B, H) fp32).
 * Replaces autograd's native_batch_norm_backward + the recurrence backward. */
int ds2_rnn_bwd_bn(ds2_rnn_ctx* ctx, int gates, const float* dyn, int lddyn, const float* bn_x, int ldx, const float* bn_mean, const float* bn_var,
                   const float* bn_gamma, const float* bn_s0, const float* bn_s1, float bn_eps, float* dy_scratch, float* gx, float* aux,
                   const float* hbuf, const void* wp_bwd, const int* lens_dev, int T, int B, int H, int bf16, void* dgx_bf16,
                   const void* gates_bf16, void* dhn_bf16, float* bias_part, void* ws, size_t ws_bytes, void* stream, int ws_armed);

/* ds2_rnn_bwd_bn with the BatchNorm's input given as bf16 (the centred operand of ds2_center_colstats; bn_mean = its delta; even pitch, H % 4 == 0) */
int ds2_rnn_bwd_bn_xbf16(ds2_rnn_ctx* ctx, int gates, const float* dyn, int lddyn, const void* bn_x_bf16, int ldx, const float* bn_mean,
                         const float* bn_var, const float* bn_gamma, const float* bn_s0, const float* bn_s1, float bn_eps, float* dy_scratch, float* gx,
                         float* aux, const float* hbuf, const void* wp_bwd, const int* lens_dev, int T, int B, int H, int bf16, void* dgx_bf16,
                         const void* gates_bf16, void* dhn_bf16, float* bias_part, void* ws, size_t ws_bytes, void* stream, int ws_armed);

/* bias gradients of one recurrent layer from ds2_rnn_bwd_ex's bias_part (B,2,4,H): db_ih (2,G*H) [bias_ih_l0 | bias_ih_l0_reverse] and
 * db_hh (2,G*H); GRU: db_ih = [d r, d z, d n], db_hh = [d r, d z, d(hn)]; LSTM: both = [d i, d f, d g, d o]; tanh cell: both = [d pre]. */
int ds2_rnn_bias_grads(int gates, const float* bias_part, int B, int H, float* dbih, float* dbhh, void* stream);

/* ---- log-softmax + CTC loss + gradient ---------------------------------------------------------
 * out.float().log_softmax(2) + torch.nn.CTCLoss(reduction="sum") and their backward,
 * trainers/deepspeech_trainer.py:108-112, trainers/__main__.py:53.  blank = 0, zero_infinity = False. */
size_t ds2_ctc_workspace_bytes(int T, int B, int max_target_len);
int ds2_ctc_loss_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                     const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float* nll_dev, float* grad, int ldg,
                     float grad_scale, void* ws, size_t ws_bytes, void* stream);
/* The same with the lattice kernel named: lattice = 0 lets the library choose (one wavefront per lattice when 2 * max_target_len + 1 <= 128,
 * one workgroup per lattice otherwise), 1 = always one workgroup per lattice.  The two forms write the same bits. */
int ds2_ctc_loss_ex_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                        const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float* nll_dev, float* grad, int ldg,
                        float grad_scale, int lattice, void* ws, size_t ws_bytes, void* stream);

/* The CTC loss for IMPERFECT transcripts: a wildcard ("star") label and optional first / last tokens, the vocabulary of
 * ds2_ctc_align_star_f32 over (log-sum-exp, +) where the aligner has (max, +).  In the literature: wild-card CTC, star temporal
 * classification.  The reference has no such loss: this text is the contract, restated in fp64 NumPy by tests/ctc_star_loss_oracle.py.
 * Everything that is not named here is ds2_ctc_loss_ex_f32's: inputs, strides, the fused row log-softmax, blank = 0, in_lens,
 * grad_scale, and the two lattice kernels chosen by `lattice` and 2 * max_target_len + 1 <= 128.
 * Wildcard emission: a state whose label is C (one past the last class) emits the constant star_penalty in every valid frame.
 *  star_penalty is fp32, finite and <= 0, natural log: anything else is a nonzero return before any launch.  (The aligner's wildcard
 *  scores "max over all classes + penalty"; the softmax summed over all classes is 1, whose log is 0: no pre-pass, and a frame spent in
 *  the wildcard yields no gradient of its own.)
 *  In the fp32 lattice a wildcard state adds the constant to log(sum) before the max is added, m + (log(sum) + star_penalty), where
 *  every other state computes (m + log(sum)) + emission as in the plain entry: a constant added to the finished value would be rounded
 *  the same way in every frame and drift.
 * Wildcard as a label: an ordinary odd state with blank states on both sides; it takes at least one frame and may repeat; the skip
 *  rule compares label VALUES, so two adjacent C behave like a repeated label.  A target value outside [1, C] makes its utterance
 *  infeasible: nll = +inf, gradient rows 0, nothing read out of bounds (the label is checked before anything is read with it).
 * Flags: flags_dev (B) int32 per utterance, NULL = all 0, the aligner's bits.
 *  bit 0: frame 0 may also start in states 2 and 3: alpha[0][s] = emission for s < min(S, 4) instead of s < 2;
 *  bit 1: the path may also end in states S-3 and S-4: beta[T_b-1][s] = emission there too, and the likelihood is the log-sum-exp of
 *         alpha[T_b-1][s] over the allowed end states that exist, taken as lse2(lse2(S-1, S-2), lse2(S-3, S-4)).
 *  The likelihood is the sum over the legal STATE paths of the lattice.  With bit 1 clear nll is the expression of the plain entry in
 *  the same operand order.
 * Gradient, for c in [0, C):
 *    grad[t,b,c] = grad_scale * ( softmax[t,b,c] * (1 - occ_star[t,b]) - occ[t,b,c] )
 *  occ_star[t,b] the summed occupancy of that utterance's wildcard states at frame t, occ the occupancy of the real classes as in the
 *  plain entry; frames beyond T_b and infeasible utterances get 0.  Repeated labels, the wildcard among them, are summed in the plain
 *  entry's deterministic chain order; the wildcard has an accumulator slot of its own with one writer.
 * Identity: with flags_dev = NULL and no C in the targets this entry writes the SAME BITS as ds2_ctc_loss_ex_f32 (nll, gradient and the
 *  alpha / beta lattices of the workspace, in both lattice kernels).
 * Workspace: that of the plain entry, ds2_ctc_star_workspace_bytes = ds2_ctc_workspace_bytes. */
size_t ds2_ctc_star_workspace_bytes(int T, int B, int max_target_len);
int ds2_ctc_star_loss_f32(const float* logits, int ld, int T, int B, int C, const int* targets_dev, const int* tgt_off_dev,
                          const int* in_lens_dev, const int* tgt_lens_dev, int max_target_len, float star_penalty, const int* flags_dev,
                          float* nll_dev, float* grad, int ldg, float grad_scale, int lattice, void* ws, size_t ws_bytes, void* stream);

/* Minimum-error-rate (MWER) training on an n-best list: the expected risk of K hypotheses per utterance under their renormalised CTC
 * posteriors, and its gradient with respect to the logits.  The reference has no such loss: this text is the contract, restated in
 * fp64 NumPy by tests/ctc_mwer_oracle.py.  Inputs, strides, the fused row log-softmax, blank = 0, in_lens and the two lattice kernels
 * chosen by `lattice` and 2 * max_hyp_len + 1 <= 128 (which write the same bits) are ds2_ctc_loss_ex_f32's.
 * For utterance b with T_b valid frames there are K hypothesis slots; slot k of utterance b is n = b * K + k in every (B, K) array:
 *  hyps_dev: int32 labels; slot n is hyps_dev[hyp_off_dev[n] ..][: hyp_lens_dev[n]], offsets int64, lengths a device array the host
 *  never learns; hyp_valid_dev (B, K) int32, nonzero = valid, NULL = all valid; risk_dev (B, K) fp32, R_k >= 0, given by the caller:
 *  the kernels do not know what the risk counts.  Labels are classes 1 .. C-1.  An EMPTY sequence is a legal hypothesis (the beam
 *  search's empty prefix): one blank state.
 * Quantities:
 *  nll_k  = -log p_ctc(y_k | x_b), the plain loss's lattice; +inf when the slot is invalid, when a label lies outside [1, C-1], when
 *           its length lies outside [0, max_hyp_len], or when the lattice is infeasible (T_b <= 0 with a non-empty sequence included);
 *           an invalid slot and a bad label are found before anything is read through them.
 *  p_k    = exp(-nll_k) / sum_j exp(-nll_j) over the slots with finite nll, a max-subtracted softmax formed in slot order; 0 for the
 *           other slots.
 *  loss_b = sum_k p_k R_k in slot order; 0 when no slot is finite or when T_b <= 0.
 *  w_k    = p_k (R_k - loss_b)  (0 for a slot that is not finite, and for every slot when T_b <= 0).
 *  grad[t,b,c] = prior + grad_scale * sum_k w_k occ_k[t,c] for t < T_b, summed in slot order; occ_k is the plain loss's occupancy of
 *           hypothesis k (repeated labels in its deterministic chain order); prior is the buffer's content when accumulate = 1 and 0
 *           when accumulate = 0.  Rows with t >= T_b get prior: accumulate = 0 writes 0 there, accumulate = 1 leaves the row alone.
 *  The softmax terms of the K CTC gradients cancel because sum_k w_k = 0; this is the cancelled form and no softmax is computed.
 *  Every gradient row sums to 0 over the classes, up to rounding.
 * Outputs: loss_dev (B), nll_hyp_dev (B, K), post_dev (B, K) = p, grad (T, B, C) at row pitch ldg, or NULL for the values alone.
 * Refused with a nonzero return before any launch: a null pointer, T, B <= 0, C <= 1, K < 1, max_hyp_len < 0, a row pitch below C,
 *  accumulate or lattice outside {0, 1}, a grad_scale that is not finite, hypotheses too long for the LDS rows of the chosen kernels,
 *  a workspace below ds2_ctc_mwer_workspace_bytes.
 * Workspace: lse (T, B) + alpha / beta for B * K lattices at pitch 2 * max_hyp_len + 1 + the repeated-label chains + the weights.  The
 *  lattices dominate: 8 B K T (2 max_hyp_len + 1) bytes, about 1 GB at B = 64, K = 4, T = 501 with max_hyp_len = T.  A caller that
 *  knows a tighter bound on the hypothesis lengths passes it. */
size_t ds2_ctc_mwer_workspace_bytes(int T, int B, int K, int max_hyp_len);
int ds2_ctc_mwer_f32(const float* logits, int ld, int T, int B, int C, int K, const int* hyps_dev, const long long* hyp_off_dev,
                     const int* hyp_lens_dev, const int* hyp_valid_dev, const int* in_lens_dev, int max_hyp_len, const float* risk_dev,
                     float* loss_dev, float* nll_hyp_dev, float* post_dev, float* grad, int ldg, float grad_scale, int accumulate,
                     int lattice, void* ws, size_t ws_bytes, void* stream);

/* Word and character confidences: HOW SURE a hypothesis is of one of its parts.  For a hypothesis y and a unit (a label range of y and a
 * frame window) the result is a true conditional probability in [0, 1]: the probability that the whole utterance spells y, given that
 * the audio outside the window spells the rest of y.  It is exact and needs no calibration set.  The reference has nothing like it: this
 * text is the contract, restated in fp64 NumPy by tests/ctc_conf_oracle.py.  Inputs, strides, the fused row log-softmax, blank = 0,
 * in_lens and the two lattice kernels chosen by `lattice` and 2 * max_hyp_len + 1 <= 128 (which write the same bits) are
 * ds2_ctc_loss_ex_f32's; the hypotheses are ds2_ctc_mwer_f32's slots with K = 1: hyps_dev int32 labels, utterance b's hypothesis is
 * hyps_dev[hyp_off_dev[b] ..][: hyp_lens_dev[b]], offsets int64.
 * Utterance b has T_b valid frames, log-softmax rows e[t][c], a hypothesis y[0..U) with labels in [1, C-1] and S = 2U + 1 states.
 *  alpha and beta are the plain loss's lattices, the emission of frame t included in both, as the workspace of ds2_ctc_loss_ex_f32
 *  holds them.  A unit is (lo, hi, ts, te): the labels [lo, hi), 0 <= lo < hi <= U, and the frames [ts, te), 0 <= ts < te <= T_b.
 *  A     = lse(alpha[ts-1][2lo-1], alpha[ts-1][2lo]), a state that does not exist being -inf; for ts = 0: 0 if lo = 0, else -inf.
 *          The probability that the frames before the window spell y[:lo].
 *  Bq    = lse(beta[te][2hi], beta[te][2hi+1]); for te = T_b: 0 if hi = U, else -inf.  The probability that the frames from te on
 *          spell y[hi:].
 *  beta' = the plain beta recurrence, the same moves and the same skip rule on label values, started at frame te from beta[te] with
 *          every state except 2hi and 2hi+1 set to -inf (for te = T_b: started from beta[T_b-1] itself) and run back to frame ts.
 *  num   = lse over s in {2lo-1, 2lo} of ( alpha[ts-1][s] + lse over the legal moves s -> s' of beta'[ts][s'] );
 *          for ts = 0: lse(beta'[0][0], beta'[0][1]).
 *  logconf = NaN if A or Bq is -inf (the context is impossible); else -inf if num is -inf; else min(0, num - (A + Bq)).
 *  Every lse takes its operands in the order state, state + 1, state + 2 (csrc/ctc_conf.h lists each one), so the bits are defined.
 * Units: n_units_dev (B) int32 and four (B, W_max) int32 arrays unit_lo / unit_hi / win_start / win_end.  Units are independent of one
 *  another and may overlap: one call may score words and characters together.  A unit has at most ds2_ctc_conf_max_unit_labels = 63
 *  labels (one wavefront holds its states).
 * Outputs: nll_dev (B), the plain loss's value (+inf for an infeasible hypothesis, a label outside [1, C-1] or a length outside
 *  [0, max_hyp_len], found before anything is read with them); logconf_dev (B, W_max).
 *  NaN goes to: a unit that breaks a bound (a label range outside [0, U], empty or above 63 labels, a window outside [0, T_b]) — that unit
 *  alone; the slots w >= n_units[b]; every slot of an utterance whose n_units lies outside [0, W_max], whose hypothesis has a label
 *  outside [1, C-1] or a length outside [0, max_hyp_len], or which has no frames.  With nll = +inf the rules above hold as they stand.
 *  Nothing at t >= T_b is read into a result.
 * Determinism: no float atomics; the bits depend neither on B, nor on the utterance's place in the batch, nor on the slot, nor on the
 *  lattice kernel, and reruns repeat them.
 * Refused with a nonzero return before any launch: a null pointer, T, B <= 0, C <= 1, W_max < 1, max_hyp_len < 0, a row pitch below C,
 *  lattice outside {0, 1}, hypotheses too long for the LDS rows of the chosen lattice kernel, B above 65535, a workspace below
 *  ds2_ctc_conf_workspace_bytes.
 * Workspace: lse (T, B) + alpha / beta at pitch 2 * max_hyp_len + 1: 8 B T (2 max_hyp_len + 1) bytes and a row. */
int ds2_ctc_conf_max_unit_labels(void);
size_t ds2_ctc_conf_workspace_bytes(int T, int B, int max_hyp_len);
int ds2_ctc_conf_f32(const float* logits, int ld, int T, int B, int C, const int* hyps_dev, const long long* hyp_off_dev,
                     const int* hyp_lens_dev, const int* in_lens_dev, int max_hyp_len, const int* n_units_dev, const int* unit_lo_dev,
                     const int* unit_hi_dev, const int* win_start_dev, const int* win_end_dev, int W_max, float* nll_dev,
                     float* logconf_dev, int lattice, void* ws, size_t ws_bytes, void* stream);

/* out[0] = sum_b nll[b] / B on the device, fixed summation order: `loss = criterion(...) / inputs.size(0)`,
 * trainers/deepspeech_trainer.py:110-112 */
int ds2_ctc_batch_mean_f32(const float* nll_dev, int B, float* out_dev, void* stream);

/* CTC forced alignment: WHEN a known transcript was spoken.  The lattice of the loss over (max, +) instead of log-sum-exp, with
 * back-pointers, the backtrace and the token spans in one launch (csrc/ctc_align.h).  The reference has no aligner: this text is the
 * contract, restated in NumPy by tests/ctc_align_oracle.py.
 * Inputs: x (B,T,C) fp32 with element strides ld_b, ld_t and C contiguous, as in the greedy decode (the model's (T,B,C)-backed eval
 *  output and a contiguous (B,T,C) tensor both work without a copy).  is_log = 1: the emission is e = x (log-probabilities);
 *  is_log = 0: e = log(x) (probabilities, log 0 = -inf), taken on the hardware log2 where the emission is loaded, not on the dependent
 *  chain.  Blank is class 0.  targets / tgt_off / tgt_lens as in the loss call (flat int32 labels, tgt_off[b] the start of utterance b);
 *  in_lens_dev (B) int32 valid frames T_b (clamped to T), or NULL = T frames for every utterance.  A target outside [1, C) makes its
 *  utterance infeasible; nothing is read out of bounds.  NaN input is unspecified.
 * States and recurrence: a target l[0..U) has S = 2U+1 states, state 2u blank, state 2u+1 the label l[u].
 *  v[0][0] = e[0][blank], v[0][1] = e[0][l[0]], every other state -inf; for t >= 1
 *    v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is odd, s >= 3 and l[s>>1] != l[(s>>1)-1]) + e[t][class(s)]
 *  in fp32: the max first, then ONE add, nothing else touches the values.  Back-pointer ties: the smallest move wins (stay beats
 *  step beats skip).  The end state is S-1 or S-2, whichever is larger, a tie going to S-1; U = 0 has the single state 0.  Taken
 *  together: among all optimal alignments, the one whose state sequence read from the last frame backwards is lexicographically
 *  greatest.  With is_log = 1 every output is therefore pinned bit for bit by a float32 restatement.
 * Outputs: score (B) the path's value; states (B,T) int32 the state per frame, -1 for t >= T_b; for every target token, in the flat
 *  target order, tok_start / tok_end (end exclusive) the frames whose state is that token's, and tok_logp the fp32 sum of its emissions
 *  in ascending t (the first emission, then one add per further frame).
 * Edge cases: an infeasible utterance (optimum -inf, T_b below U plus the number of adjacent repeats, a bad label, T_b <= 0 with
 *  U > 0, or tgt_lens[b] outside [0, max_target_len]) gets score -inf, states -1, token spans (-1, -1), tok_logp -inf; T_b <= 0 with
 *  U = 0 gets score 0.  Nonzero return on bad arguments or when the workspace is too small (before any launch).
 * Variants: 1 = one wavefront per utterance, the row in registers, two states per lane (only when 2*max_target_len+1 <= 128: nonzero
 *  return otherwise); 2 = one workgroup per utterance, any target length that fits the LDS rows (beyond 1024 state pairs every thread
 *  loops over its pairs); 0 = the library chooses (1 when it is valid).  All variants write the same bits.
 * Workspace: the back-pointers, 2 bits per (frame, state), packed 8 frames of a state pair to a dword:
 *  ds2_ctc_align_workspace_bytes = 4 * B * ceil(T/8) * (max_target_len+1), from host-known sizes only; tok_* hold sum(tgt_lens)
 *  entries (they may be NULL when max_target_len == 0). */
size_t ds2_ctc_align_workspace_bytes(int B, int T, int max_target_len);
int ds2_ctc_align_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                      const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                      int max_target_len, int variant,
                      float* score, int* states, int* tok_start, int* tok_end, float* tok_logp,
                      void* ws, size_t ws_bytes, void* stream);

/* CTC forced alignment of LONG recordings: the lattice of ds2_ctc_align_f32 cut into tiles of tile_pairs adjacent state pairs x
 * tile_frames frames, each worked by one workgroup (csrc/ctc_align_tiled.h).  Tile (k, f) depends only on tiles (k-1, f) and (k, f-1),
 * so the tiles of one anti-diagonal k + f = d are independent: one launch per anti-diagonal, and the kernel boundary is the only
 * synchronisation between workgroups; one further launch per call walks the back-pointers through a moving window of state pairs
 * and writes the spans.  There is no limit on max_target_len or T beyond the workspace (an hour of speech against 50 000 labels is
 * about 4.5 GB of back-pointers; all addressing is 64-bit).
 * Contract: every input, output, edge case and tie rule is that of ds2_ctc_align_f32 above, word for word: the same recurrence in fp32
 *  (the max first, then one add), stay beats step beats skip, the end state S-1 on a tie, the same infeasible outputs, is_log 0 / 1
 *  with the same emission.  It writes the same bits as the variants of ds2_ctc_align_f32, for either kind of input, under every
 *  tile shape.  Tiles that no legal path can touch (every state above 2t + 1, or too low to reach the end by T_b - 1) are skipped.
 * tile_frames = 0 / tile_pairs = 0 choose the library's defaults (64 frames x 64 pairs, the fastest shape measured); otherwise tile_frames must be a positive
 *  multiple of 8 (a back-pointer dword, 8 transitions of a pair, has one writer) and tile_pairs a positive multiple of 64 up to 1024
 *  (one pair per thread; 64 = one wavefront per tile, the neighbour by DPP instead of LDS).  Nonzero return on anything else, on bad
 *  arguments or when the workspace is too small (before any launch).
 * Workspace, from host-known sizes only, with Wp = max_target_len+1 and K = ceil(Wp / tile_pairs): the back-pointers in the layout of
 *  ds2_ctc_align_f32 (B * ceil(T/8) * Wp dwords), the boundary columns (B * K * T floats: the odd state of every tile's top pair per
 *  frame), the row carries (B * K * tile_pairs * 2 floats: both states of every pair at a frame-block seam) and the end values
 *  (2 B floats); ds2_ctc_align_tiled_workspace_bytes is 4 x their sum, or 0 for an illegal shape. */
size_t ds2_ctc_align_tiled_workspace_bytes(int B, int T, int max_target_len, int tile_frames, int tile_pairs);
int ds2_ctc_align_tiled_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                            const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                            int max_target_len, int tile_frames, int tile_pairs,
                            float* score, int* states, int* tok_start, int* tok_end, float* tok_logp,
                            void* ws, size_t ws_bytes, void* stream);

/* CTC forced alignment of IMPERFECT transcripts: a wildcard ("star") token and optional first / last tokens on top of
 * ds2_ctc_align_f32 (csrc/ctc_align_star.h; the lattice kernels of ctc_align.h / ctc_align_tiled.h instantiated with the two additions).
 * The reference has no aligner: this text is the contract, restated in NumPy by tests/ctc_align_star_oracle.py.  Everything that is not
 * named here (inputs, strides, is_log, recurrence, tie rule, back-pointer layout, outputs, infeasible outputs, variants 0 / 1 / 2) is
 * ds2_ctc_align_f32's, word for word.
 * Wildcard emission, per valid frame, with e the emission of that contract:
 *    g[t] = (max over all classes c in [0, C), blank included, of e[t][c]) + star_penalty
 *  the max first, then ONE fp32 add.  With is_log = 0 the max is taken on x and the emission expression (the hardware log2, then the
 *  ln 2 multiply) is applied to that maximum.  g is stored as a log value in the workspace by a pre-pass that reads x once; the lattice
 *  loads it as it is.  An all -inf row gives -inf.  NaN is unspecified.  star_penalty is fp32, <= 0 and finite: anything else is a
 *  nonzero return before any launch.
 * Wildcard as a label: in targets the value C (one past the last class) is the wildcard, legal only through these entries (the plain
 *  entries keep calling it a bad label).  It is an ordinary odd state that emits g[t]: it takes at least one frame, it may repeat,
 *  blank states sit on both sides, and the skip rule compares label VALUES as before (C differs from every class; two adjacent C
 *  behave like a repeated label).  A target outside [1, C] makes its utterance infeasible.
 * Optional first and last token: flags_dev (B) int32 per utterance, NULL = all 0.
 *  bit 0: the path may also START in state 2 or 3:  v[0][s] = e[0][class(s)] for s < min(S, 4) instead of s < 2;
 *  bit 1: the path may also END in state S-3 or S-4: the end is the largest v[T_b-1][s] over the allowed end states that exist
 *         (S-1, S-2, S-3, S-4, those >= 0), a tie going to the larger state.
 *  The global statement stays true: among all optimal legal paths, the one whose state sequence, read from the last frame backwards,
 *  is lexicographically greatest.  A token whose state no frame takes (a skipped first or last token) gets tok_start = tok_end = -1
 *  and tok_logp = 0; a wildcard token's tok_logp is the fp32 sum of its g[t] in ascending t.  Everything infeasible keeps the outputs
 *  of ds2_ctc_align_f32.  With is_log = 1 every output is pinned bit for bit by a float32 restatement; with flags NULL and no
 *  wildcard label the outputs are the bits of ds2_ctc_align_f32.
 * ds2_ctc_align_star_row_f32 is the pre-pass alone: g (B,T) contiguous, frames t >= T_b are not written.
 * Workspace: that of ds2_ctc_align_f32, then g:  ds2_ctc_align_star_workspace_bytes = ds2_ctc_align_workspace_bytes + 4 * B * T. */
int ds2_ctc_align_star_row_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                               const int* in_lens_dev, float star_penalty, float* g, void* stream);
size_t ds2_ctc_align_star_workspace_bytes(int B, int T, int max_target_len);
int ds2_ctc_align_star_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                           const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                           int max_target_len, int variant, float star_penalty, const int* flags_dev,
                           float* score, int* states, int* tok_start, int* tok_end, float* tok_logp,
                           void* ws, size_t ws_bytes, void* stream);

/* The tiled form of ds2_ctc_align_star_f32 for long recordings: ds2_ctc_align_tiled_f32 with the wildcard and the flags above, and the
 * same bits as ds2_ctc_align_star_f32 under every tile shape.  The two tests that skip a tile move by one pair for an utterance whose
 * flag is set: bit 0, a tile is skipped when every state of it lies above 2t + 3 (instead of 2t + 1); bit 1, when it cannot reach state
 * S-4 (instead of S-2) by frame T_b - 1.  Four end values per utterance are captured instead of two.
 * Workspace: ds2_ctc_align_tiled_workspace_bytes + 8 * B (the two further end values) + 4 * B * T (g), or 0 for an illegal shape. */
size_t ds2_ctc_align_star_tiled_workspace_bytes(int B, int T, int max_target_len, int tile_frames, int tile_pairs);
int ds2_ctc_align_star_tiled_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log,
                                 const int* targets_dev, const int* tgt_off_dev, const int* in_lens_dev, const int* tgt_lens_dev,
                                 int max_target_len, int tile_frames, int tile_pairs, float star_penalty, const int* flags_dev,
                                 float* score, int* states, int* tok_start, int* tok_end, float* tok_logp,
                                 void* ws, size_t ws_bytes, void* stream);

/* Keyword search over CTC posteriors: WHERE a phrase was said, and whether it was said at all (csrc/ctc_kws.h; in the literature:
 * Lengerich & Hannun 2016).  The (max, +) lattice of ds2_ctc_align_f32 entered at any frame, on emissions taken relative to the
 * frame's best class, for K keywords against every utterance of a batch in one call.  The reference has nothing like it: this text is
 * the contract, restated in NumPy by tests/ctc_kws_oracle.py.
 * Inputs: x, ld_b, ld_t, is_log and in_lens_dev mean what they mean for ds2_ctc_align_f32 (blank is class 0, in_lens_dev NULL = T
 *  frames).  The keywords are shared by the batch: kw_labels_dev flat int32 labels, kw_off_dev (K) the start of keyword k in it,
 *  kw_lens_dev (K) its length U_k; max_kw_len >= every U_k and <= 63 (one wavefront holds a keyword, two states per lane; a larger value
 *  is a nonzero return, and a kw_lens entry above max_kw_len makes that keyword one without a hit).  thr_dev (K) fp32: one threshold
 *  per keyword.  max_hits in [1, 1024].
 * Emission: with e the emission of that contract, g[t] = (max over all classes c of e[t][c]) + 0.0f is the wildcard row of
 *  ds2_ctc_align_star_f32 with penalty 0 (with is_log = 0 the max is taken on x, as there), and d[t][c] = e[t][c] - g[t] is ONE fp32
 *  subtract, -inf where e is -inf.  So d <= 0, and a path's value is its log-likelihood ratio against the frame-wise best path.  A
 *  frame whose classes are all -inf is unspecified, and so is NaN.
 * States: the aligner's numbering; a keyword l[0..U) has the live states 1 .. 2U-1, odd state 2u+1 the label l[u], even state 2u the
 *  blank between two labels.  State 0 and a trailing blank do not exist: a detection begins on the first label's first frame and ends
 *  on the last label's last frame.  Every state carries a value v and the start frame s of its path.
 * Recurrence: before frame 0 every value is -inf.  For each frame t < T_b and state q, the max over the moves
 *    stay  v[t-1][q];   step  v[t-1][q-1], q >= 2;   skip  v[t-1][q-2], q odd, q >= 3, l[q>>1] != l[(q>>1)-1];
 *    enter the value 0 with the start t, q == 1 only
 *  then ONE fp32 add of d[t][class(q)]; nothing else touches the values.  Ties: the smallest move wins (stay beats step beats skip)
 *  and enter loses every tie, so an existing path, which has the earlier start, is kept.  The start travels with the chosen move; a
 *  state whose value is -inf has the start -1.
 * Per-frame outputs, (B,K,T) each: frame_score[b][k][t] = v[t][2U-1], frame_start[b][k][t] = s[t][2U-1]; (-inf, -1) for t >= T_b, and
 *  in every frame for a keyword with U = 0 or a label outside [1, C), which has no hit.
 * Pick, per (b, k): greedy non-maximum suppression.  Candidates are the frames with a finite frame_score >= thr[k].  A round takes
 *  the live candidate with the largest score (a tie: the smallest t), writes (hit_start = frame_start[t], hit_end = t + 1, hit_score)
 *  to the next slot and kills every candidate t' whose closed span [frame_start[t'], t'] intersects [frame_start[t], t].  It stops
 *  when no candidate is live or max_hits are written; n_hits[b][k] is the number written, or max_hits + 1 if a live candidate
 *  remained.  hit_start / hit_end / hit_score are (B,K,max_hits), in order of acceptance, unused slots (-1, -1, -inf); n_hits (B,K).
 * With is_log = 1 every output is pinned bit for bit by a float32 restatement (scores compared after + 0.0f: -0 and +0 are equal).
 * Workspace, from host-known sizes only: g (B * T floats), then the pick's compacted candidate frames (B * K * T int32):
 *  ds2_ctc_kws_workspace_bytes = 4 * B * T * (1 + K), or 0 for B, T, K <= 0 or max_hits outside [1, 1024].  There is no back-pointer
 *  array and no limit on T.  Three launches on the stream (the g row, the lattice, the pick).  Nonzero return on bad arguments or a
 *  short workspace, before any launch. */
size_t ds2_ctc_kws_workspace_bytes(int B, int T, int K, int max_hits);
int ds2_ctc_kws_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* in_lens_dev,
                    const int* kw_labels_dev, const int* kw_off_dev, const int* kw_lens_dev, int K, int max_kw_len,
                    const float* thr_dev, int max_hits,
                    float* frame_score, int* frame_start, int* hit_start, int* hit_end, float* hit_score, int* n_hits,
                    void* ws, size_t ws_bytes, void* stream);

/* Streaming keyword search: ds2_ctc_kws_f32 fed a chunk of frames at a time, with every detection reported as final as soon as no later
 * frame can change it (csrc/ctc_kws_stream.h; restated in NumPy by tests/ctc_kws_stream_oracle.py).  The lattice is the same kernel in a
 * streaming instance; what is new is the rule for when the greedy pick, which is not causal (a later, better candidate kills an earlier
 * one), has settled.  Memory and time per feed depend on the chunk and on `pending`, not on how long the stream has run; step 4 scans the
 * list once per lowering of c, so it is quadratic in the candidates pending in the worst case (a chain of candidates that overlap
 * pairwise: at pending = 65536 about 6.7e7 loads by one wavefront), linear when c cuts no candidate.
 * State, per (utterance b, keyword k), caller-owned device memory, opaque, written by every feed: the frames consumed n_b; the value and
 *  start frame of the keyword's states as the lanes of the lattice kernel hold them (E, O, sE, sO per lane), start frames ABSOLUTE,
 *  counted from the stream's first frame; the tail c (every frame below it is settled); a pending list of at most `pending` candidates
 *  (t, start, score), ascending in t; the counters `forced` and `dropped`.  The per-frame arrays are not kept across feeds.  All zero
 *  bytes is a freshly opened stream (opening is one ds2_memset_async): a frame count of 0 means "initialise, do not load".
 *  ds2_ctc_kws_stream_state_bytes(B, K, pending) = 4 * B * K * (264 + 3 * pending), or 0 for B, K <= 0, B * K >= 2^31 or pending outside
 *  [1, 65536].  The keywords, the thresholds, B, C, `pending` and max_lag must not change within a stream: the state does not record
 *  them, and a state of another stream or one not written by this entry is not detected.
 * Arguments: x (B,T,C), ld_b, ld_t, is_log as ds2_ctc_kws_f32 takes them, T >= 0 frames in this call (x may be NULL at T == 0);
 *  in_lens_dev (B) the valid frames of THIS call per utterance (clamped to [0, T]; NULL: T each), 0 leaves the utterance's lattice and
 *  frame count untouched; the packed keywords and thr_dev exactly as ds2_ctc_kws_f32 takes them; max_hits in [1, 1024]; max_lag: the
 *  most frames the tail may lie behind n_b after a feed (negative: no limit); finish 0 or 1 (T == 0 with finish == 1 is a pure flush;
 *  T == 0 with finish == 0 reads the tentative detections out again).  frames_bound: an upper bound of the frames any utterance has
 *  consumed so far (the sum of the earlier calls' T will do); frames_bound + T > 2^31 - 1 is refused, and the kernel itself never takes
 *  n_b past 2^31 - 1 (it consumes fewer frames instead).
 * A feed does, per (b, k):
 *  1. Lattice.  Frames n_b .. n_b + T_b - 1 run the recurrence of ds2_ctc_kws_f32 (the same cell, tie order, single subtract and single
 *     add) with t absolute, g being the best-class row of the chunk.  frame_score / frame_start (B,K,T), optional (both NULL or both
 *     given): chunk-relative in position, absolute in the start values, (-inf, -1) beyond T_b.  Concatenated over the feeds they have
 *     the BITS of ds2_ctc_kws_f32 on the concatenated frames, for any cuts.
 *  2. Intake.  Every frame of the chunk whose end-state score is finite and >= thr[k] becomes a candidate (t, start, score).  One whose
 *     start lies below the tail is dropped and counted in `dropped` (possible only after a forced cut, step 4); one that does not fit
 *     into the list is dropped and counted.
 *  3. Horizon.  h = min(n, min over the states q whose value is finite and >= thr[k] of start[q]), after the chunk's last frame.  Every
 *     emission term d is <= 0 and an fp32 add of a non-positive number never increases a value, so a state below the threshold can
 *     never again produce a candidate: every candidate of a later feed starts at or after h.
 *  4. Settle.  c = the largest value in [tail, max(tail, h)] for which no pending candidate has start < c <= t; with finish, c = n.  If
 *     max_lag >= 0 and n - c > max_lag: c = n - max_lag, `forced` is incremented, and the pending candidates with start < c <= t are
 *     dropped and counted (a forced cut).
 *  5. Pick.  The greedy rule of ds2_ctc_kws_f32 (largest score first, a tie to the smaller t, a winner kills every candidate whose
 *     closed span intersects its own) on the pending candidates with t < c, which are FINAL, then on the rest, which are TENTATIVE,
 *     into the same max_hits slots.  Candidates on the two sides of c cannot overlap, so the two passes select what one pass would;
 *     final first means an overflow costs tentative detections before final ones.  hit_start / hit_end (exclusive) / hit_score /
 *     hit_final (B,K,max_hits) in order of acceptance, absolute frames, unused slots (-1, -1, -inf, 0); n_hits (B,K) the slots
 *     written, or max_hits + 1 if a live candidate remained; tail = c, frames = n, forced, dropped (B,K), the last two totals of the
 *     stream.
 *  6. The candidates with t < c leave the list, and tail = c.
 * Consequences.  Without max_lag and without an overflow (of the list or of the slots), for ANY cuts of the frames into feeds: the
 *  detections reported final so far together with the current tentative ones are exactly the detections of ds2_ctc_kws_f32 on the
 *  frames consumed so far, as a set of (start, end, score bits); a final detection is reported in exactly one feed and never changes.
 *  Final detections of one keyword never overlap, with or without max_lag.  A forced cut is the only place where a stream may differ
 *  from the one-call search.  A final detection can be withheld for as long as a path at or above the threshold that began before it
 *  stays alive; the typical case is the keyword spoken up to its last label but one, then silence, which keeps that path's value.  That
 *  is what max_lag is for; which max_lag serves real recordings is unmeasured.  A forced cut that falls into the span of a pending
 *  candidate loses that candidate: it lies at n - max_lag after the feed that forces it, so with feeds of one frame and a path that
 *  stays alive it moves through every frame, and a withheld detection of more than one frame is dropped, not released.
 * Workspace: the row g (B * T floats) and, when frame_score is NULL, the two per-frame arrays of the chunk:
 *  ds2_ctc_kws_stream_workspace_bytes(B, T, K, frames_out) = 4 * B * T * (frames_out ? 1 : 1 + 2 * K); 0 at T == 0 (ws may be NULL).
 * Launches on `stream`: the g row and the lattice (T > 0 only), then intake / settle / pick as one kernel, one wavefront per (b, k).
 * Nothing is copied back.  Nonzero return on bad arguments, a short state or a short workspace, before any launch: the state is then
 * unchanged. */
size_t ds2_ctc_kws_stream_state_bytes(int B, int K, int pending);
size_t ds2_ctc_kws_stream_workspace_bytes(int B, int T, int K, int frames_out);
int ds2_ctc_kws_stream_feed_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, int is_log, const int* in_lens_dev,
                                const int* kw_labels_dev, const int* kw_off_dev, const int* kw_lens_dev, int K, int max_kw_len,
                                const float* thr_dev, int max_hits, int max_lag, int finish, int pending, long long frames_bound,
                                void* state, size_t state_bytes, float* frame_score, int* frame_start,
                                int* hit_start, int* hit_end, float* hit_score, int* hit_final, int* n_hits,
                                int* tail, int* frames, int* forced, int* dropped, void* ws, size_t ws_bytes, void* stream);

/* softmax over the last dim (eval-mode InferenceBatchSoftmax, modules/blocks.py:59-64) */
int ds2_softmax_rows_f32(const float* x, int ldx, float* y, int ldy, int rows, int C, void* stream);

/* greedy CTC decode: per-frame arg-max (ties -> lowest class, torch.max's first-maximum rule), collapse repeats,
 * drop blanks; replaces GreedyDecoder.decode / convert_to_strings / process_string,
 * decoders/greedy_decoder.py:10-68 (a per-frame host loop with one .item() sync per frame).
 * probs (B,T,C) fp32 with element strides ld_b, ld_t (C contiguous); sizes_dev (B) int32 or NULL (= T frames).
 * Outputs: ids/offs (B,T) int32 — the first out_len[b] entries of row b are the kept labels and their frames. */
size_t ds2_greedy_decode_workspace_bytes(int B, int T);
int ds2_greedy_decode_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                          int* ids, int* offs, int* out_len, void* ws, size_t ws_bytes, void* stream);

/* CTC prefix beam search without a language model; replaces BeamCTCDecoder.decode, decoders/beam_decoder.py (which calls the
 * external ctcdecode package).  One workgroup per utterance runs every frame in one launch (csrc/ctc_beam.h).
 * Contract, in natural log (log 0 = -inf), logaddexp written (+):
 *  - every prefix l (labels without blanks) carries pb (paths ending in blank) and pnb (ending in l's last label e);
 *    total = pb (+) pnb; the start is the empty prefix with pb = 0, pnb = -inf;
 *  - per frame the classes are sorted by probability, highest first, ties to the lower index; at most cutoff_top_n are kept,
 *    and if cutoff_prob < 1 the list stops after the first class at which the running sum reaches cutoff_prob (the blank
 *    is pruned like any class);
 *  - for every beam l and kept class c with log-prob lp, into fresh -inf accumulators: c == blank: pb'(l) (+)= total(l) + lp;
 *    c == e: pnb'(l) (+)= pnb(l) + lp and pnb'(l+c) (+)= pb(l) + lp; otherwise pnb'(l+c) (+)= total(l) + lp.  Contributions to
 *    the same prefix are summed whichever beam they came from; a prefix with total -inf drops out;
 *  - the beam_width (K) prefixes with the highest total survive; ties: shorter prefix first, then the lexicographically
 *    smaller class-index sequence.  A prefix that was a beam keeps its offsets, a new l+c gets offsets(l) followed by t;
 *  - after frame sizes[b]-1 the survivors, in that order, fill the K output slots; empty slots have length 0, score -inf.
 * probs (B,T,C) fp32 probabilities with element strides ld_b, ld_t (C contiguous); sizes_dev (B) int32 or NULL (= T; 0 leaves
 * only the empty prefix).  Outputs: labels / offsets (B,K,T) int32 (zero past each length), lens (B,K) int32, scores (B,K) fp32,
 * best beam first.  Accuracy: fp32 on the device against the fp64 restatement tests/ctc_beam_oracle.py.
 * Limits: 1 <= K <= ds2_ctc_beam_max_width() (256), 2 <= C <= 16384, T < 2^20, cutoff_top_n >= 1.  The workspace holds the prefix
 * back-pointers (parent, label, frame per node, at most T*K nodes per utterance): ds2_ctc_beam_workspace_bytes = 12*B*T*K. */
int ds2_ctc_beam_max_width(void);
size_t ds2_ctc_beam_workspace_bytes(int B, int T, int beam_width);
int ds2_ctc_beam_decode_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                            int beam_width, int cutoff_top_n, float cutoff_prob, int* labels, int* offsets, int* lens, float* scores,
                            void* ws, size_t ws_bytes, void* stream);

/* The same search with shallow fusion of an n-gram language model (LM) read from an ARPA file (asr_amd/decoders/lm.py parses it;
 * replaces ctcdecode's KenLM scorer).  Logs are natural except LM scores, which are log10 as the file stores them; alpha multiplies
 * those log10 values.  Parity with ctcdecode is not pinned.
 *  - vocabulary: the file's 1-grams, token id = position among them.  Character mode when every entry other than <s>, </s> and
 *    <unk> is one Unicode character, word mode otherwise (word mode needs a space label);
 *  - lm(w | h), h the last N-1 tokens left-padded with <s> (N the order): the listed n-gram (h, w)'s log10 prob, else backoff(h)
 *    (0 when h is not listed) + lm(w | h[1:]); OOV = -1000 when any token of (h, w) is outside the vocabulary; </s> is never scored;
 *  - word mode: a word is the run of labels between spaces, spelt with the decoder's characters, matched exactly.  The dictionary
 *    is every vocabulary word other than <s>, </s>, <unk> whose characters are all non-blank, non-space labels.  A prefix survives
 *    only in the form (word ' ')* partial with every word in the dictionary and partial a (possibly empty) prefix of a dictionary
 *    word (no leading or double space): any other extension is -inf.  Appending the space adds alpha*lm(word | ctx) + beta to
 *    that extension's contribution.  After the last frame every surviving non-empty beam not ending in a space gets
 *    alpha*lm(partial | ctx) + beta (OOV when partial is no dictionary word) and the survivors are re-sorted by the order above;
 *  - character mode: every non-blank extension l -> l+c adds alpha*lm(char(c) | ctx) + beta; no dictionary, no end term.  An ARPA
 *    line is split on whitespace, so no file can hold the token " ": a character model spells the space as U+2581 (LOWER ONE EIGHTH
 *    BLOCK), and the loader gives the space label that token (models without it price a space as OOV, as before);
 *  - everything else is the contract above: the LM terms ride in pnb of the extension, so pb / pnb / total include every bonus
 *    so far (the bonus depends only on the prefix, so merging stays exact), and scores are the fused totals.  ctcdecode's
 *    min_cutoff heuristic and its "approx_ctc" returned score are deliberately left out.
 * Every beam is extended by every kept non-blank class (the no-LM staircase bound does not hold with per-class bonuses):
 * K * (min(cutoff_top_n, C-1) + 2) <= ds2_ctc_beam_lm_max_candidates() (4096), e.g. K = 100 at C = 29.
 * The packed LM (csrc/ctc_lm.h): ds2_ctc_lm_packed_bytes sizes it, ds2_ctc_lm_pack fills it on the host from the parsed arrays
 * (ngram_tok n_ngrams x order, -1 padded; ngram_n their orders; prob / bow log10; the trie's edges (node, label) -> child, node 0
 * the root; node_word the token id of the word a node spells or -1; label_tok (C) the token of every label in character mode;
 * bos the token id of <s> or -1; mode 1 character, 2 word).  ds2_ctc_lm_score is lm(w | hist) on the host (hist: order-1 token
 * ids, oldest first; -1 = out of vocabulary).  The decode reads the packed bytes from device memory (lm_dev, lm_bytes). */
int ds2_ctc_beam_lm_max_candidates(void);
size_t ds2_ctc_lm_packed_bytes(int order, int n_ngrams, int n_edges, int n_nodes, int C);
int ds2_ctc_lm_pack(int order, int n_ngrams, const int* ngram_tok, const int* ngram_n, const float* prob, const float* bow, int n_edges,
                    const int* edge_node, const int* edge_label, const int* edge_child, int n_nodes, const int* node_word, int C,
                    const int* label_tok, int bos, int mode, void* out, size_t out_bytes);
int ds2_ctc_lm_score(const void* packed, const int* hist, int n_hist, int w, float* out);
int ds2_ctc_beam_decode_lm_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                               int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev, size_t lm_bytes, int lm_order,
                               int lm_mode, int space, float alpha, float beta, int* labels, int* offsets, int* lens, float* scores,
                               void* ws, size_t ws_bytes, void* stream);

/* N-best rescoring, part 1: the LM term of FINISHED label sequences as a number of its own (csrc/lm_score.h; restated by
 * tests/lm_score_oracle.py).  The search above fuses that term into its totals, where alpha and beta cannot be varied without decoding
 * again; with it apart, a list decoded once can be re-ranked under any weights, or under a larger model than the first pass could carry.
 * P sequences: labels flat int32 (n_labels of them), sequence p is labels[off[p] .. off[p] + len[p]); off (P) int64, len (P) int32,
 * device arrays; max_len bounds every length.  The model is the blob ds2_ctc_lm_pack made, on the device (lm_dev) and as the host copy
 * (lm_host, lm_bytes) whose magic and sizes are checked before the launch, against lm_order, lm_mode and C as well; space, C, blank as
 * the LM search takes them.  The kernel's lookups end only because the packer keeps its tables at most half full: pass no other bytes.
 *  - tokens, character mode: every label is a token, label_tok[label], the space label included;
 *  - tokens, word mode: the sequence is split at the space label; empty runs (a leading, doubled or trailing space) are skipped and
 *    score nothing; every non-empty run is one token, the word id of the trie node its labels spell, -1 when the walk leaves the trie
 *    or the node spells no word.  The last run is scored whether or not a space follows it (the search's end-of-utterance term), so
 *    "a b" and "a b " score alike.  </s> is never scored;
 *  - score of token i: s_i = lm(w_i | h_i) as above (cond_score of csrc/ctc_lm.h), h_i the previous order-1 tokens of the sequence,
 *    out-of-vocabulary ids included, left-padded with <s>.  If s_i is the OOV constant -1000 (w_i or a context token is outside the
 *    vocabulary) n_oov is incremented and nothing is added; otherwise lm_sum += s_i in fp32, IN TOKEN ORDER.  n_tok counts every
 *    token, OOV ones included.  So lm_sum + n_oov * (-1000) is the search's LM total of an admissible labeling at alpha = 1, beta = 0,
 *    and a caller may price OOV differently;
 *  - outputs per sequence: lm_sum fp32 (log10), n_tok int32, n_oov int32.  They are a function of the sequence and the blob alone:
 *    not of P, of the position in the batch or of max_len;
 *  - a sequence with len outside [0, max_len], a range outside [0, n_labels), or a label outside [0, C) or equal to the blank is
 *    refused: NaN, -1, -1, found by a ballot before anything is read through the label; its neighbours are not disturbed.
 * One launch, one wavefront per sequence, no workspace, any length.  ds2_lm_score_seq_host scores ONE sequence on the host, serially,
 * through the same token and score routines and the same order of additions (order and mode are the packed header's). */
int ds2_lm_score_seqs(const int* labels, long long n_labels, const long long* off, const int* len, int P, int max_len,
                      const void* lm_dev, const void* lm_host, size_t lm_bytes, int lm_order, int lm_mode, int space, int C, int blank,
                      float* lm_sum, int* n_tok, int* n_oov, void* stream);
int ds2_lm_score_seq_host(const void* packed, size_t packed_bytes, const int* labels, int len, int max_len, int space, int C, int blank,
                          float* lm_sum, int* n_tok, int* n_oov);

/* N-best rescoring, part 2: which slot of every utterance's list wins at every point of an (alpha, beta) grid, and what the winners'
 * errors add up to (csrc/lm_score.h).  Per (utterance n < N, slot k < K), device arrays: ac fp32 (natural log), lm_sum fp32, n_tok and
 * n_oov int32 (the outputs above), err (N,K,R) int32 for 1 <= R <= 64 error kinds; oov_score (log10, not NaN); alphas (Ga), betas (Gb)
 * fp32 on the device.  Score of slot k at (a, b), fp32, every operation rounded on its own (no contraction into an fma, so a float32
 * restatement matches the bits):  lm = lm_sum + oov_score * n_oov;  s = (ac + alpha * lm) + beta * n_tok.
 * A NaN score counts as -inf; the pick is the highest s, ties to the lowest k; if every slot is -inf the pick is slot 0.
 * Outputs: pick (Ga,Gb,N) int32 or NULL; total (Ga,Gb,R) int64 = sum over n of err[n, pick, r], integer atomics: exact, order-free.
 * One launch (and one memset of total); nothing of size N * K * Ga * Gb is stored.  N may be 0 (totals of 0). */
int ds2_nbest_sweep(const float* ac, const float* lm_sum, const int* n_tok, const int* n_oov, const int* err, int N, int K, int R,
                    float oov_score, const float* alphas, int Ga, const float* betas, int Gb, int* pick, long long* total, void* stream);

/* Estimation of the n-gram models the entries above read: interpolated modified Kneser-Ney from sentences of token ids
 * (csrc/ngram_train.h; restated in fp64 by tests/ngram_train_oracle.py; asr_amd/decoders/lm_train.py tokenises and writes the ARPA
 * file).  Byte parity with KenLM's lmplz is not pinned; model interpolation is not offered; pruning (a count cut and an entropy
 * threshold) and perplexity are the entries after these.
 * Input: tokens flat int32, offsets (n_sent + 1) int64 ascending from 0 to n_tokens; ids 0 = <unk> (never in the input), 1 = <s>,
 * 2 = </s>, tokens in [3, n_vocab).  N the order, 1 <= N <= 6.
 *  - framing: a sentence is its tokens between one <s> and one </s>; a sentence without tokens is skipped; no n-gram spans two;
 *  - raw counts c_n(g), n = 1..N, over the framed sentences;
 *  - adjusted counts: a_N = c_N; for n < N, a_n(g) = c_n(g) if g[0] = <s> and n >= 2, else |{v : c_{n+1}(v g) > 0}|; a_1(<s>) = 0 at
 *    every N;
 *  - discounts of order n: t_k = |{g : a_n(g) = k}|, k = 1..4 (the count-of-counts); Y = t_1 / (t_1 + 2 t_2);
 *    D_{n,k} = k - (k + 1) Y t_{k+1} / t_k, k = 1..3; D_{n,0} = 0, counts >= 3 use D_{n,3}.  When a t_k is 0 or a D_{n,k} is outside
 *    [0, k] the order FALLS BACK to the caller's three discounts (each within [0, k]);
 *  - a context h of n - 1 tokens has S_n(h) = sum_w a_n(h w), N_{n,k}(h) = |{w : a_n(h w) = k}| (k = 3: >= 3), and
 *    gamma_n(h) = ((D_1 N_1 + D_2 N_2) + D_3 N_3) / S_n(h);
 *  - V = every token seen, </s> and <unk>, without <s>; p_1(w) = (a_1(w) - D) / S_1 + gamma_1 / |V|, a_1(<unk>) = 0;
 *    p_n(w | h) = (a_n(h w) - D) / S_n(h) + gamma_n(h) * p_{n-1}(w | h[1:]) for every counted h w; all in fp64;
 *  - listed per counted g: log10 p (-99 for <s>), and log10 gamma_{n+1}(g) as its backoff when n < N, g does not end in </s> and
 *    S_{n+1}(g) > 0 (a gamma of 0 is -99), else none (NaN in these arrays); <unk> is log10(gamma_1 / |V|).
 * Keys: an n-gram is n * b bits of one 64-bit word, b the bit width of n_vocab - 1, the oldest token highest, so keys of one order sort
 * as their token ids do; n * b > 64 is refused (ds2_ngram_max_order(n_vocab) is the largest order admitted).  No key is 0.
 * Device tables, one per order n, caller-allocated: keys (slots[n-1] x u64), vals (slots x 8 uint32: c, lext, adjusted, S, N_1, N_2,
 * N_3, unused; the last four describe the entry AS A CONTEXT of order n + 1), prob (slots x 2 fp64: log10 p, log10 backoff); slots a
 * power of two in [2, 2^30], at least the distinct n-grams of that order (twice min(positions, n_vocab^n) is what ops.py takes);
 * glob: ds2_ngram_glob_words() u64 words (flags: 0 overflow, 5 bad input, 6 missing entry; 1..4 the empty context's S_1, N_{1,k};
 * 7 the distinct 1-grams = |V|; 8 + 4 (n - 1) + (k - 1) = t_k of order n).  All accumulation is integer atomics: the values do not
 * depend on arrival order, the slot of a key does, so callers sort the live slots (key != 0) by key.  Probe loops run at most `slots`
 * steps and then set a flag.
 *   ds2_ngram_count      clears the tables and glob, then one launch: a lane per token position inserts the n-grams ending there
 *                        (64-bit compare-and-swap on the key, integer atomic on c); <s> and </s> come from the offsets;
 *   ds2_ngram_adjust     N launches, order N down to 1: adjusted counts, left extensions of the suffix, sums of the context, t_k;
 *   ds2_ngram_discounts  HOST: from a copy of glob, D (order x 4), fell_back (order), coc (order x 4), log10 p(<unk>); refuses a set flag;
 *   ds2_ngram_probs      N launches, order 1 up to N, then N that take the logarithms; D as ds2_ngram_discounts gave it (host);
 *   ds2_ngram_estimate_host  the whole estimator on the host (std::unordered_map, the same formula routines): per order, cap[n-1]
 *                        rows of room, n_distinct[n-1] rows written in key order: keys, count, adjusted, log10 p, log10 backoff. */
int ds2_ngram_max_order(int n_vocab);
int ds2_ngram_glob_words(void);
int ds2_ngram_count(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                    const long long* slots, void* const* keys, void* const* vals, void* glob, void* stream);
int ds2_ngram_adjust(int n_vocab, int order, const long long* slots, void* const* keys, void* const* vals, void* glob, void* stream);
int ds2_ngram_discounts(int order, const unsigned long long* glob_host, const double* fallback, double* D, int* fell_back, long long* coc,
                        double* unk_log10);
int ds2_ngram_probs(int n_vocab, int order, const long long* slots, void* const* keys, void* const* vals, void* const* prob, void* glob,
                    const double* D, void* stream);
int ds2_ngram_estimate_host(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                            const double* fallback, const long long* cap, unsigned long long* const* keys_out, unsigned* const* count_out,
                            unsigned* const* adjusted_out, double* const* lp_out, double* const* bow_out, long long* n_distinct,
                            long long* coc, double* D, int* fell_back, double* unk_log10);

/* Evaluation and pruning of such models (csrc/ngram_prune.h; restated in fp64 by tests/ngram_prune_oracle.py;
 * asr_amd/decoders/lm_train.py: NgramEstimate.perplexity / .prune, prune_arpa).  The pruning rule is the project's own: parity with
 * SRILM's -prune and with lmplz's --prune is not pinned (neither tool was at hand).  Interpolation of several models is not offered.
 * The model M: per order n = 1..N, cnt[n-1] rows of keys (u64 as above, ASCENDING), lp (fp64 log10 p) and lb (fp64 log10 backoff,
 * NaN where none is listed).  The 1-grams list <unk> (key 0) as an ordinary row when the model has one.  Ids: 0 <unk>, 1 <s>, 2 </s>.
 *  - p_M(w | h), h of m <= N - 1 tokens: the listed (m+1)-gram h w, else backoff(h) * p_M(w | h[1:]), backoff(h) = 1 where h is not
 *    listed or lists none; at m = 0 an unlisted w is OOV: reported, not scored.  Every lookup is a binary search, at most
 *    log2(cnt) + 1 steps; no loop spins, no shift is by 64 (keys of N * b = 64 bits are legal), nothing is added with an atomic.
 *  - ds2_ngram_eval: sentences as in ds2_ngram_count (flat int32 ids, n_sent + 1 int64 offsets), but EVERY sentence is scored, an
 *    empty one as </s> after <s>, and ids may be 0.  Sentence s owns the positions off[s] + s .. off[s+1] + s of the outputs (its
 *    tokens, then </s>), n_tokens + n_sent in all, one lane each: out_lp = log10 p_M(token | the N - 1 framed tokens before it), out_order
 *    = the order of the n-gram that was listed; OOV (or an id outside [0, n_vocab)): order 0 and NaN.  An id outside [0, n_vocab) in
 *    the context ends the context there.  Nothing is accumulated: the caller sums.
 *  - pruning marks n-grams of order >= 2; for a listed h w of order n: p its listed probability, q = p_M(w | h[1:]),
 *    sp(h) / sq(h) = the sums of p / q over the listed children of h, num = 1 - sp, den = 1 - sq, alpha = h's listed backoff or 1,
 *    alpha' = (num + p) / (den + q), P(h) = prod_i p_M(h_i | h_1 .. h_{i-1}) with a leading <s> scored as p_M(</s>), and in natural
 *    logarithms  dH = -P(h) (p (ln q + ln alpha' - ln p) + num (ln alpha' - ln alpha));  val = exp(dH) - 1; marked when val < theta
 *    (Stolcke 1998: each n-gram judged as if it alone left its context).  An n-gram whose context is not listed has val NaN, unmarked.
 *  - ds2_ngram_prune_sums, one call per order n = 2..N: sp and sq per row of order n - 1 (NaN: no child) and q per row of order n
 *    (q_out may be null).  A lane per n-gram, a segmented scan over the wave in lane order, and for contexts whose children cross
 *    waves a second launch over one partial per wave: the order of the additions depends on the keys alone, so equal arrays give
 *    equal bits.  scratch: 4 doubles per 64 rows of order n.  The host twin adds each context's children in row order.
 *  - ds2_ngram_prune_entropy, one launch over all orders >= 2: q, sp, sq, val, mark are `order` pointers, entry n - 1 for the n-grams
 *    of order n (entry 0 unused; sp / sq of entry n - 1 have the rows of order n - 1); val fp64, mark one byte per row.
 *  - ds2_ngram_prune_closure, one call per order n = N down to 3: a row of order n with mark 0 clears the mark of its context, so
 *    every kept n-gram's prefix is kept and kept sets are nested in theta.
 *  - ds2_ngram_prune_backoff, one call per order bottom up, on the KEPT rows: lb = log10((1 - sp) / (1 - sq)) from ds2_ngram_prune_sums
 *    over the kept children and the model already finished below; NaN where sp is NaN (a context left without children).
 * The *_host twins run the same per-entry routines serially from host arrays. */
int ds2_ngram_eval(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                   const long long* cnt, void* const* keys, void* const* lp, void* const* lb, double* out_lp, int* out_order, void* stream);
int ds2_ngram_eval_host(const int* tokens, long long n_tokens, const long long* offsets, long long n_sent, int n_vocab, int order,
                        const long long* cnt, void* const* keys, void* const* lp, void* const* lb, double* out_lp, int* out_order);
int ds2_ngram_prune_sums(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, int n,
                         double* q_out, double* sp, double* sq, double* scratch, long long scratch_doubles, void* stream);
int ds2_ngram_prune_sums_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, int n,
                              double* q_out, double* sp, double* sq);
int ds2_ngram_prune_entropy(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb,
                            void* const* q, void* const* sp, void* const* sq, double theta, void* const* val, void* const* mark,
                            void* stream);
int ds2_ngram_prune_entropy_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb,
                                 void* const* q, void* const* sp, void* const* sq, double theta, void* const* val, void* const* mark);
int ds2_ngram_prune_closure(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, int n,
                            const unsigned char* mark, unsigned char* mark_ctx, void* stream);
int ds2_ngram_prune_closure_host(int n_vocab, int order, const long long* cnt, void* const* keys, void* const* lp, void* const* lb, int n,
                                 const unsigned char* mark, unsigned char* mark_ctx);
int ds2_ngram_prune_backoff(long long cnt, const double* sp, const double* sq, double* lb, void* stream);
int ds2_ngram_prune_backoff_host(long long cnt, const double* sp, const double* sq, double* lb);

/* The same search with hotword boosting: the caller names a few phrases and the search prefers prefixes that spell them, with or
 * without the LM above (asr_amd/decoders/hotwords.py builds the automaton; restated by tests/ctc_beam_hot_oracle.py).  Parity with
 * pyctcdecode, WeNet or icefall biasing is not pinned.
 *  - phrases: N >= 1 sequences of 1..64 non-blank label ids, each with a weight w >= 0 per label, finite, in NATURAL-log units (the
 *    units of the acoustic totals, not the LM's log10).  No two phrases are equal and none is a proper prefix of another (the host
 *    refuses such a set); a phrase may be an infix or a suffix of another;
 *  - automaton: the trie of the phrases, root at depth 0, with Aho-Corasick failure links.  Node n has the potential
 *    phi(n) = depth(n) * max(w of the phrases through n), computed in fp64 and rounded once to fp32; phi(root) = 0, and the end node
 *    of a phrase lies on that phrase only, so its phi is len * w of that phrase;
 *  - step from state n on label c: n' = the longest suffix of path(n) + c that is a trie node (goto / failure walk; the root when
 *    there is none).  The term of the extension is phi(n') - phi(n), in fp32; it may be negative: a broken partial match gives its
 *    lead back.  If n' ends a phrase the new state is the root and the phrase's len * w stays banked, otherwise the new state is n';
 *  - end of utterance: every surviving beam gets -phi(state) added to its total, then the survivors are re-sorted by the order above
 *    (total descending, length ascending, label sequence ascending);
 *  - invariant: the terms of a complete labeling sum to the len * w of the phrases credited by this scan: keep the longest suffix of
 *    the labels since the last credit that is a prefix of a phrase; when that suffix is a whole phrase, credit it and restart.  So an
 *    occurrence hidden inside a longer partial match is not credited, matching restarts at the root after a credit, and matching
 *    is on the label stream and knows no word boundary ("CAT" also boosts "CATALOG");
 *  - composition: the term adds to the LM term of the same extension (a -inf from word mode's dictionary stays -inf) and rides in
 *    pnb exactly as the LM term does; the state of a prefix is a function of its labels, so merged contributions agree.  lm_dev may
 *    be NULL ("hot-only"): the LM term is 0, no LM table is read, and lm_bytes .. beta are ignored.
 * Every beam is extended by every kept non-blank class, with or without an LM: the LM arm's candidate limit applies, and one more
 * int of LDS per beam and beam buffer; a shape whose layout then exceeds 160 KiB is refused with a message (at K = 256, C = 29,
 * cutoff_top_n = 14, the LM arm's largest grid, it is 150 752 bytes).
 * The packed automaton (csrc/ctc_hot.h): at most 2^20 trie nodes (1000 phrases of 64 labels need 64001), 64 labels per phrase,
 * C <= 16384.  ds2_ctc_hot_packed_bytes sizes it (0: outside the limits; n_edges = n_nodes - 1), ds2_ctc_hot_pack fills it on the
 * host from the edges (node, label) -> child (node 0 the root), fail / phi / terminal per node, and refuses a trie that is no tree, a
 * node deeper than 64, a failure link that does not point to a strictly shallower node (the root's: to itself), and a phi that is
 * not finite and >= 0: a walk then ends within the depth.  ds2_ctc_hot_step is one step on the host, by the device's code: next
 * state and fp32 term.  The decode reads the packed bytes from device memory (hot_dev) and checks the magic and sizes of the host
 * copy (hot_host, hot_bytes) before it launches. */
size_t ds2_ctc_hot_packed_bytes(int n_nodes, int n_edges);
int ds2_ctc_hot_pack(int n_nodes, int n_edges, const int* edge_node, const int* edge_label, const int* edge_child, const int* fail,
                     const float* phi, const int* terminal, int C, void* out, size_t out_bytes);
int ds2_ctc_hot_step(const void* packed, int node, int label, int* next, float* term);
int ds2_ctc_beam_decode_hot_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                                int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev, size_t lm_bytes, int lm_order,
                                int lm_mode, int space, float alpha, float beta, const void* hot_dev, const void* hot_host,
                                size_t hot_bytes, int* labels, int* offsets, int* lens, float* scores, void* ws, size_t ws_bytes,
                                void* stream);

/* Streaming beam search: the three searches above, fed a chunk of frames at a time (csrc/ctc_beam_stream.h).  The same kernel in
 * streaming instances: a call loads every utterance's beams from `state`, runs the unchanged frame loop over this call's frames,
 * writes the beams back, optionally reads them out, and reports how much of the text is final.  After any cuts of an utterance's
 * frames into calls, a read-out gives the BITS of one decode call on the frames consumed so far (labels, offsets, lengths, scores).
 *  - search arguments: those of ds2_ctc_beam_decode_hot_f32.  lm_dev and hot_dev are both nullable: both NULL is the plain search
 *    with its staircase, lm_dev alone the LM arm, hot_dev the hotword arm (with or without lm_dev); the limits and refusals of the
 *    arm apply.  T >= 0 frames in this call (probs may be NULL at T == 0); sizes_dev (B) valid frames of THIS call per utterance
 *    (clamped to [0, T]; NULL: T each), so an utterance with 0 simply does not advance.  Every call of one stream passes the same B,
 *    C, blank, beam_width, cut-offs, model and hotwords: the state does not record them.
 *  - state: ds2_ctc_beam_stream_state_bytes(B, beam_width, lm, hot) bytes of device memory (lm / hot: non-zero when lm_dev / hot_dev
 *    will be given; 0 for B or beam_width outside the limits), opaque, written by every call.  All zero bytes is a freshly opened
 *    stream: opening is one ds2_memset_async.
 *  - nodes: the back-pointers (parent | label | frame per utterance, cap_frames * beam_width int32 each), caller-owned,
 *    ds2_ctc_beam_stream_nodes_bytes(B, cap_frames, beam_width) = 12 * B * cap_frames * beam_width bytes.  Node ids do not depend on
 *    cap_frames: to grow, allocate for a larger capacity and copy each utterance's three arrays to the front of their new places.
 *    frames_bound: an upper bound of the frames any utterance has consumed so far (the sum of the earlier calls' T will do);
 *    frames_bound + T <= cap_frames < 2^20 or the call is refused.  This entry compacts nothing: 12 * beam_width bytes per frame
 *    (ds2_ctc_beam_stream_commit below does; a state that went through it must be fed through the committed entry, not this one).
 *  - read-out, when n_out > 0 (n_out <= beam_width): the end-of-utterance stage (word mode's partial-word term, the hotwords'
 *    -phi(state), the re-sort) on a copy the next call does not see, then labels / offsets (B, n_out, W) int32, zero past each length,
 *    lens (B, n_out), scores (B, n_out): the first n_out slots of the decode call's outputs; a slot past the surviving beams has
 *    length 0 and score -inf.  W >= frames_bound + T.  With n_out == 0 the four pointers may be NULL.  T == 0 with n_out > 0 is a pure
 *    read-out (the final result: n_out = beam_width); T == 0 with n_out == 0 is refused.
 *  - stable_len (B) int32: the length of the longest prefix of (label, offset) pairs common to ALL live beams.  Every beam of every
 *    later call descends from a live beam, so the first stable_len labels and offsets of any later read-out, of any slot, are these:
 *    the value never decreases, and with no live beam it is kept.  frames (B) int32: frames consumed so far, this call included.
 * One launch on `stream`, nothing is copied back.  A state of another arm, width or stream, or one not written by this entry, is
 * not detected. */
size_t ds2_ctc_beam_stream_state_bytes(int B, int beam_width, int lm, int hot);
size_t ds2_ctc_beam_stream_nodes_bytes(int B, int cap_frames, int beam_width);
int ds2_ctc_beam_stream_feed_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev, int blank,
                                 int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev, size_t lm_bytes, int lm_order,
                                 int lm_mode, int space, float alpha, float beta, const void* hot_dev, const void* hot_host,
                                 size_t hot_bytes, void* state, size_t state_bytes, void* nodes, size_t nodes_bytes, int cap_frames,
                                 int frames_bound, int n_out, int W, int* labels, int* offsets, int* lens, float* scores,
                                 int* stable_len, int* frames, void* stream);

/* Bounding an open stream: commit and compaction of its back-pointers (csrc/ctc_beam_commit.h).  Every later beam descends from a
 * live beam, so the stable prefix can leave the device, and of the nodes only the LIVE TREE is still needed: the chains from the live
 * beams down to the node of the last committed pair.  ds2_ctc_beam_stream_commit, one launch, per opened utterance with live beams:
 *  - forced cut, only where cut_frame[b] >= 0 (cut_frame (B) int32 on the device, or NULL: no cut anywhere).  The first slot of the
 *    saved state (the search's own order, before any end-of-utterance term) has m pairs with an offset < cut_frame[b]; if m exceeds the
 *    stable length, every live beam that is shorter than m or does not share those m pairs is dropped, the survivors keep their order
 *    and every per-beam field, and the stable prefix becomes those m pairs.  This is the ONLY step after which a stream may differ from
 *    one decode call.  dropped (B) int32, nullable: the beams dropped.
 *  - commit: the pairs from the committed length up to min(stable length, committed length + Wc) are written in text order to
 *    labels / offsets (B, Wc) int32 (cells past them are not written); Wc >= 0, the rows may be NULL at Wc == 0.
 *  - compaction: the live tree is renumbered in the order of its ids (a parent stays below its children) and written to nodes_out, a
 *    DISTINCT buffer of cap_rows_out >= cap_rows rows (an overlap with `nodes` is refused), so growth and compaction are one copy; the
 *    node of the last committed pair becomes the root (parent -1).  The next frame writes row ceil(M / beam_width) of nodes_out.
 *  - info (B, 4) int32: pairs committed by this call, M = nodes of the live tree, the longest live beam's length less the committed
 *    length (a bound on the row width a read-out needs, grows by at most one per frame), the frame of the last committed pair.
 * An utterance never fed, or one with no live beam, has nothing to move: M = 0.  lm / hot as ds2_ctc_beam_stream_state_bytes takes them.
 * ws: ds2_ctc_beam_stream_commit_workspace_bytes(B, cap_rows, beam_width) bytes of device memory, 0 (ws may be NULL) where the
 * bitmap of cap_rows * beam_width nodes fits LDS; the query gives 0 for sizes outside the limits as well, which the entry refuses.
 * The search's results do not depend on node ids, so without a forced cut a read-out keeps the bits of one decode call.
 * A COMMITTED state (one that went through this entry) is fed through ds2_ctc_beam_stream_feed_committed_f32 and must NOT go through
 * ds2_ctc_beam_stream_feed_f32, whose bounds count frames: here the node capacity and the bound count ROWS of beam_width nodes
 * (rows_bound >= ceil(M / beam_width) + the frames fed since the commit, for every utterance; rows_bound + T <= cap_rows), the read-out
 * rows hold only the pairs from the committed length on (at position s - committed length; lens, scores and stable_len stay absolute,
 * offsets stay absolute frames), and W >= labels_bound + T with labels_bound >= info[b][2] + the frames fed since, for every
 * utterance.  Everything else is ds2_ctc_beam_stream_feed_f32's contract; a state that never committed may be fed through either.
 * Limits that remain: 2^20 - 1 labels per utterance between resets (the candidate key's length field), and fp32 totals that are
 * absolute, not rebased. */
size_t ds2_ctc_beam_stream_commit_workspace_bytes(int B, int cap_rows, int beam_width);
int ds2_ctc_beam_stream_commit(void* state, size_t state_bytes, int B, int beam_width, int lm, int hot, const void* nodes,
                               size_t nodes_bytes, int cap_rows, void* nodes_out, size_t nodes_out_bytes, int cap_rows_out,
                               const int* cut_frame, int Wc, int* labels, int* offsets, int* info, int* dropped, void* ws,
                               size_t ws_bytes, void* stream);
int ds2_ctc_beam_stream_feed_committed_f32(const float* probs, long long ld_b, long long ld_t, int B, int T, int C, const int* sizes_dev,
                                           int blank, int beam_width, int cutoff_top_n, float cutoff_prob, const void* lm_dev,
                                           size_t lm_bytes, int lm_order, int lm_mode, int space, float alpha, float beta,
                                           const void* hot_dev, const void* hot_host, size_t hot_bytes, void* state, size_t state_bytes,
                                           void* nodes, size_t nodes_bytes, int cap_rows, int rows_bound, int labels_bound, int n_out,
                                           int W, int* labels, int* offsets, int* lens, float* scores, int* stable_len, int* frames,
                                           void* stream);

/* Batched Levenshtein distance (unit costs: insert, delete, substitute) of P independent pairs of int32 symbol sequences, one launch;
 * the WER / CER scoring of DeepSpeech.evaluate() (replaces Decoder.wer / Decoder.cer's per-utterance DP, decoders/decoder.py:26-58,
 * whose reference uses the `Levenshtein` C package).  The host maps words / characters to ids (asr_amd/decoders), symbols compare
 * as plain int32 values.  Problem p compares seq[a_off[p] .. a_off[p] + a_len[p]) with seq[b_off[p] .. b_off[p] + b_len[p]);
 * sides may alias or overlap.  a_off / b_off (P) int64, a_len / b_len (P) int32, all device arrays; n_seq = symbols in seq.
 * Output dist (P) int32: the exact distance (an empty side gives the other side's length), or -1 for a problem whose range leaves
 * [0, n_seq) or whose longer side exceeds max_len while its shorter side exceeds 64.
 * Method: blocked Myers / Hyyroe bit-vectors (csrc/edit_distance.h), one wave per problem, ceil(min/64) * max column steps.
 * Workspace: one int8 row of the longer side per problem, ds2_edit_distance_workspace_bytes(P, max_len) with max_len >= every
 * problem's longer side (host-known lengths: the call never synchronises); 0 bytes (ws may be NULL) when max_len <= 64. */
size_t ds2_edit_distance_workspace_bytes(int P, long long max_len);
int ds2_edit_distance_i32(const int* seq, long long n_seq, const long long* a_off, const int* a_len, const long long* b_off,
                          const int* b_len, int P, long long max_len, int* dist, void* ws, size_t ws_bytes, void* stream);

/* Batched edit ALIGNMENT: the hits, substitutions, deletions and insertions behind each of those distances, and which symbol pairs
 * with which (csrc/edit_align.h); every output is pinned to the integer by tests/edit_align_oracle.py, which restates this text.  The
 * problem layout (seq, n_seq, a_off, a_len, b_off, b_len, P) is ds2_edit_distance_i32's.  Side a is the hypothesis (m symbols), side
 * b the reference (n symbols).
 * The DP: D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i][j-1] + 1, D[i-1][j] + 1).
 * The path is traced from (m, n) to (0, 0); at (i, j) the FIRST option that holds is taken:
 *   1. i > 0 && j > 0 && D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j]: a[i-1] pairs with b[j-1], a hit if equal, else a substitution;
 *   2. j > 0 && D[i][j-1] + 1 == D[i][j]: b[j-1] is a deletion;
 *   3. otherwise a[i-1] is an insertion.
 * Optimal alignments are not unique; this rule picks one, whichever side the kernel puts on its rows.
 * Outputs: counts (P,4) int32 = (hits, substitutions, deletions, insertions), so S + D + I is ds2_edit_distance_i32's distance;
 *  a_map (P,max_len): a_map[p][i] = the index in b paired with a[i], -1 for an insertion; b_map (P,max_len): b_map[p][j] = the index
 *  in a paired with b[j], -1 for a deletion; entries at or beyond a side's length are -1, so every row is fully written.  A problem
 *  whose range leaves [0, n_seq) or with a side above max_len gets counts (-1,-1,-1,-1) and rows of -1.  An empty side gives all
 *  insertions or all deletions.
 * Workspace: ds2_edit_align_workspace_bytes(P, max_len) = P * ceil(max_len / 64) * max_len * 16 bytes (every column's bit-vector pair,
 *  2 bits per DP cell) + ds2_edit_distance_workspace_bytes(P, max_len), or 0 for P <= 0 or max_len <= 0; ws 16-byte aligned.  It grows
 *  with the SQUARE of max_len: about 3 MB for 128 problems of 300 symbols, 625 MB for one pair of 50 000; there is no linear-memory
 *  traceback.  max_len >= every problem's longer side (host-known lengths: the call never synchronises); it must fit int32.
 * One launch, one wave per problem: ceil(min/64) * max column steps, then at most m + n traceback steps. */
size_t ds2_edit_align_workspace_bytes(int P, long long max_len);
int ds2_edit_align_i32(const int* seq, long long n_seq, const long long* a_off, const int* a_len, const long long* b_off,
                       const int* b_len, int P, long long max_len, int* counts, int* a_map, int* b_map, void* ws, size_t ws_bytes,
                       void* stream);

/* Pause segmentation of CTC posteriors (csrc/ctc_segment.h): where to cut a long recording so that its pieces can be decoded as one
 * batch.  Integer work on the blank column; every output is pinned to the integer by tests/ctc_segment_oracle.py, which restates this
 * text.  The reference has nothing like it.
 * Inputs: x (B,T,C) fp32 with element strides ld_b / ld_t (class dim contiguous); in_lens_dev (B) int32 or NULL (= T),
 *  T_b = clamp(in_lens[b], 0, T); blank in [0, C); thr fp32, compared against the raw value: silent(t) := x[b][t][blank] >= thr, which
 *  is false for NaN (for log-probabilities pass the logarithm of the threshold: there is no is_log); min_gap >= 1, pad >= 0,
 *  max_len >= 2, max_segs >= 1.
 * Pauses: a pause is a maximal run [a, b) of silent frames of [0, T_b) with b - a >= min_gap, or a == 0, or b == T_b (a silent run at
 *  either end of the utterance is a pause at any length).
 * Regions: the maximal intervals of [0, T_b) that no pause covers, in order; shorter silent runs stay inside their region.  No region:
 *  0 segments.
 * Padding: with m(a, b) = a + (b - a) / 2 (integer division) for a pause [a, b), a region [s, e) becomes [s', e'):
 *    s' = max(s - pad, lo), lo = 0 if s == 0 or the pause in front starts at frame 0, else m of the pause in front;
 *    e' = min(e + pad, hi), hi = T_b if e == T_b or the pause behind ends at T_b, else m of the pause behind.
 *  Segments therefore never overlap.
 * Forced cuts: a padded region longer than max_len is split left to right.  cur = s'; while e' - cur > max_len: the cut c is the frame
 *  of [cur + (max_len + 1) / 2, cur + max_len] (both ends included) with the greatest x[b][c][blank], scanned upwards with a strict >
 *  (the smallest c wins a tie; which frame wins among NaN values is unspecified); emit [cur, c) with flag bit 1 (value 2: ends at a
 *  forced cut); cur = c, and the next piece carries flag bit 0 (value 1: starts at a forced cut).  The last piece is [cur, e').  So
 *  every segment has 1 <= length <= max_len, and a piece that ends at a forced cut has at least (max_len + 1) / 2 frames.
 * Outputs: seg_start, seg_end (exclusive), seg_flags (B, max_segs) int32, ascending in time, unused slots (-1, -1, 0); n_segs (B) the
 *  full count, which may exceed max_segs: then only the first max_segs are written.
 * Workspace, from host-known sizes only: ds2_ctc_segment_workspace_bytes(B, T) = B * (8 * ceil(T / 64) + 4 * (4 * (T / 2 + 1) + T))
 *  bytes (the silence bits, the run and pause lists, the forced cuts), or 0 for B, T <= 0; ws 8-byte aligned.  Two launches on the
 *  stream: one lane per frame writes a 64-bit ballot word per 64 frames, spread over the GPU; then one workgroup per utterance works
 *  on the words.  Nonzero return on bad arguments or a short workspace, before any launch. */
size_t ds2_ctc_segment_workspace_bytes(int B, int T);
int ds2_ctc_segment_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, const int* in_lens_dev, int blank, float thr,
                        int min_gap, int pad, int max_len, int max_segs, int* seg_start, int* seg_end, int* seg_flags, int* n_segs,
                        void* ws, size_t ws_bytes, void* stream);

/* Packs S segments of x (the same x, ld_b, ld_t, B, T, C as above) into one padded batch, one launch: out (S, T_max, C) contiguous,
 * row s a bit-exact copy of x[seg_b[s]][seg_start[s] : seg_start[s] + seg_len[s]] followed by zeros up to T_max, and out_sizes[s] =
 * seg_len[s].  seg_b_dev, seg_start_dev, seg_len_dev (S) int32 device arrays.  A segment with seg_b outside [0, B), seg_start < 0,
 * seg_len < 0, seg_start + seg_len > T or seg_len > T_max is rejected: an all-zero row and out_sizes[s] = 0.  Nonzero return on bad
 * arguments, before the launch. */
int ds2_ctc_segment_gather_f32(const float* x, long long ld_b, long long ld_t, int B, int T, int C, const int* seg_b_dev,
                               const int* seg_start_dev, const int* seg_len_dev, int S, int T_max, float* out, int* out_sizes,
                               void* stream);

/* conv1 in bf16 mode (Conv2d(1,32,(41,11),s=(2,2),p=(20,5)), deepspeech.py:61, forward + weight gradient; conv1 has no data
 * gradient).  ds2_conv1_gather_bf16 builds the two bf16 operand images from the spectrogram batch: XB (B,F,P) = the rows themselves as
 * bf16, XB[..][7 + s] = x[..][s] with zeros in front and behind (P = ds2_conv1_bf16_row_pitch(T)) for the forward — the 16 taps of an output
 * step are 16 consecutive samples of a row — and X16T (B,F,16,pad64(T)) time-contiguous per tap for the weight gradient (either may be NULL).
 * ds2_conv1_bf16_bytes(which = 0 packed weights | 1 XB | 2 X16T, B, F, T) sizes the buffers. */
int ds2_conv1_bf16_row_pitch(int T);
size_t ds2_conv1_bf16_bytes(int which, int B, int F, int T);
int ds2_conv1_pack_bf16(const float* w1, void* wp, void* stream);
int ds2_conv1_gather_bf16(const float* x, void* XB, void* X16T, int B, int F, int Tin, void* stream);
int ds2_conv1_fwd_bf16(const void* XB, const void* wp, const float* bias, const int* lens_dev, float* y1, int B, int F, int Tin,
                       void* stream);
/* ... with the BatchNorm2d statistics of y1 taken in the epilogue: stat_part = ds2_conv1_fwd_bf16_stat_blocks() x 32 x 2 floats of per-block
 * (sum, sum of squares) per channel; ds2_chanstats_from_partials turns them into mean / biased var (+ running stats) - no pass over y1 */
int ds2_conv1_fwd_bf16_stat_blocks(int B, int F, int Tin);
int ds2_conv1_fwd_bf16_stats(const void* XB, const void* wp, const float* bias, const int* lens_dev, float* y1, int B, int F, int Tin,
                             float* stat_part, void* stream);
size_t ds2_conv1_wgrad_bf16_workspace_bytes(int B, int Tin);
int ds2_conv1_wgrad_bf16(const void* X16T, const float* dy1, const int* lens_dev, float* dW1, int B, int F, int Tin, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- spectrogram front-end -------------------------------------------------------------
 * SpectrogramParser.parse_audio's arithmetic, data/parsers/spectrogram_parser.py:45-60, for a whole batch:
 * librosa.stft (centred frames, win_length = n_fft) -> |.| -> log1p -> optional (x - mean) / std(unbiased) per utterance,
 * written in the zero-padded (B,1,n_bins,T) layout of _collate_fn (functional.py:18-30).
 * audio (B, ld_audio) fp32 device waveforms, n_samples_dev (B) int32; basis (n_fft, 2*n_bins) = window-folded DFT basis
 * [w cos | -w sin interleaved per bin]; pad_mode 0 = zeros (librosa >= 0.10 default) / 1 = reflect; hop % 4 == 0. */
int ds2_spectrogram_frames(int n_samples, int hop);
size_t ds2_spectrogram_workspace_bytes(int B, int T, int n_fft, int hop);
int ds2_spectrogram_f32(const float* audio, long long ld_audio, const int* n_samples_dev, int B, int T, int n_fft, int hop,
                        const float* basis, int pad_mode, int normalize, float* out, void* ws, size_t ws_bytes, void* stream);
/* The augmented front-end: the same spectrogram with noise injection before the STFT and SpecAugment masks after the statistics.
 * Per-utterance parameters are drawn on the host (asr_amd.data.GpuSpectrogramFrontEnd); the device only applies them.
 *  Noise injection (asr_deepspeech/data/noise_injection.py:22-38): utterance b with noise_level[b] != 0 is mixed as
 *      y[j] = x[j] + level_b * seg[j] * rms(x) / rms(seg),   seg[j] = noise[noise_base[b] + (noise_start[b] + j) mod noise_period[b]],
 *  rms over the utterance's own n_b samples (energies: fp32 block partials combined in fp64); rms(seg) == 0 leaves the utterance unmixed.
 *  The padding (zeros or reflect) is that of the mixed signal; no mixed copy of the waveform is written and `audio` is not modified.
 *  noise (noise_len) fp32 = ONE bank of concatenated noise files; noise_base (B) int64, noise_period / noise_start (B) int32,
 *  noise_level (B) fp32 (0 = off); a segment outside the bank (base + period > noise_len, start outside [0, period)) is not mixed.
 *  The four arrays are all NULL for no noise at all.
 *  SpecAugment (no time warp): freq_masks (B, n_freq_masks, 2) / time_masks (B, n_time_masks, 2) int32 [lo, hi) bin / frame ranges,
 *  at most 8 of each; an element inside any range of its utterance, with t < frames_b, is written as 0 — after the per-utterance
 *  normalisation when `normalize` (masks do not enter the statistics).  Padding frames stay exactly 0.
 *  Level 0 and no masks give the bits of ds2_spectrogram_f32. */
size_t ds2_spectrogram_aug_workspace_bytes(int B, int T, int n_fft, int hop);
int ds2_spectrogram_aug_f32(const float* audio, long long ld_audio, const int* n_samples_dev, int B, int T, int n_fft, int hop,
                            const float* basis, int pad_mode, int normalize, const float* noise, long long noise_len,
                            const long long* noise_base, const int* noise_period, const int* noise_start, const float* noise_level,
                            const int* freq_masks, int n_freq_masks, const int* time_masks, int n_time_masks, float* out, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- tempo / gain perturbation (audio_conf.speed_volume_perturb) ----------------------------------------------
 * load_randomly_augmented_audio, audio/functional.py:94-104, runs `sox ... tempo f gain g` per utterance, before noise injection
 * (spectrogram_parser.py:36-44).  sox is not part of the reference tree: PARITY WITH SOX IS UNPINNED.  The contract below is modelled
 * on what its `tempo` effect is published to do (WSOLA, waveform-similarity overlap-add) and is what tests/tempo_oracle.py restates.
 * Per utterance: x[0..n) fp32 (reads outside [0, n) give 0), tempo factor f (fp64, 0.5 <= f <= 2), linear gain G (fp32, >= 0).
 *  Sizes, each int(sample_rate * ms / 1000 + 0.5): segment S (82 ms), search R (14.68 ms), overlap O (12 ms); hop H = S - O
 *  (16 kHz: 1312, 235, 192, 1120).  S > 2 O, R >= 1, O >= 1, R + O <= 2048.  ds2_tempo_sizes returns them (non-zero: outside the contract).
 *  n_out = floor(n / f + 0.5) in fp64 (ds2_tempo_out_samples, a host function; -1 for n outside [0, 2^29] or f outside [0.5, 2]);
 *  K = ceil(n_out / H) segments.  Nominal input position of segment k: p_k = floor(k * f * H + 0.5), IEEE fp64, every operation
 *  rounded on its own — the device evaluates exactly this expression.
 *  Search signal: s[i] = clamp(rint(x[i] * 32768), -32768, 32767), an integer (round half to even): the 16-bit sample sox is handed.
 *  q_0 = 0.  For k >= 1, with the tail t[i] = s[q_{k-1} + H + i], i in [0, O) — what would naturally follow segment k-1 — d_k in [0, R)
 *  minimises SSD(d) = sum_i (s[p_k + d + i] - t[i])^2 in exact integer arithmetic, the lowest d on ties; q_k = p_k + d_k.
 *  Output of segment k at y[k H ...], cut to n_out: O samples a + w_i (b - a), a = x[q_{k-1} + H + i], b = x[q_k + i],
 *  w_i = (i + 0.5) / O in fp32 (k = 0: x[i]; b == a gives a itself), then H - O samples x[q_k + O + j].
 *  Last, y = min(max(G y, -1), 1).  f = 1, G = 1 returns x bit for bit (|x| <= 1).  sox's requantisation to 16 bits with dither is
 *  noise by design and is not reproduced.
 * ds2_tempo_gain_f32: audio (B, ld_audio) fp32 device rows; n_samples (B) int32, tempo (B) fp64 and gain (B) fp32 (linear) are HOST
 * arrays (the host sizes everything from them; nothing is copied back).  out (B, ld_out) fp32 device: y in [0, n_out_b), exact zeros
 * in [n_out_b, ld_out), so the batch can go straight into ds2_spectrogram_f32 / ds2_spectrogram_aug_f32 with n_out_dev (B) int32 device,
 * which is written too.  offsets_out (B, ld_offsets) int32 device: d_k for k < K_b (d_0 = 0), 0 for K_b <= k < ld_offsets;
 * ld_offsets >= every K_b.  workspace: ds2_tempo_workspace_bytes(B) device bytes.  Arguments outside the contract return non-zero
 * and launch nothing.  Two kernels (csrc/tempo.hip): the chain of searches, one workgroup per utterance, and the synthesis over
 * (utterance, segment); no atomics, reruns are bit-identical. */
int ds2_tempo_sizes(int sample_rate, double segment_ms, double search_ms, double overlap_ms, int* S, int* R, int* O);
int ds2_tempo_out_samples(int n, double f);
size_t ds2_tempo_workspace_bytes(int B);
int ds2_tempo_gain_f32(const float* audio, long long ld_audio, const int* n_samples, const double* tempo, const float* gain, int B,
                       int sample_rate, double segment_ms, double search_ms, double overlap_ms, float* out, long long ld_out,
                       int* n_out_dev, int* offsets_out, int ld_offsets, void* workspace, size_t workspace_bytes, void* stream);

/* ---- packed waveform feed (asr_amd.data, get_loader(front_end="gpu", prefetch=N)) ------------------------------
 * The host side of the waveform loader (data/loaders/functional.py:6-24 + the per-item parse_audio, spectrogram_parser.py:36-44) sends
 * ONE ragged buffer per batch; this pass makes the zero-padded (B, n_max) fp32 batch that ds2_tempo_gain_f32 / ds2_spectrogram_f32 /
 * ds2_spectrogram_aug_f32 read, in place of B host slice copies into a pageable fp32 tensor.
 *  packed (packed_elems) device elements of the type `dtype` tags: 0 = int16 (raw 16-bit PCM), 1 = fp32; 16-byte aligned;
 *  packed_elems a multiple of 8, below 2^31 (0 allowed, packed may then be NULL).
 *  Utterance u occupies [offsets[u], offsets[u] + lengths[u]); ALIGNMENT RULE: every offset is a multiple of 8 ELEMENTS and
 *  offsets[u] + round_up(lengths[u], 8) <= packed_elems, so the elements up to the next multiple of 8 exist (their values are not used).
 *  lengths[u] == 0 is allowed (the row is all zeros).  offsets_dev, lengths_dev, src_index_dev: (B) int32 DEVICE arrays.
 *  out (B, ld_out) fp32 device, ld_out >= n_max, any 4-byte-aligned pitch: row b is utterance u = src_index[b] (any index in [0, B),
 *  repeats allowed): out[b][j] = x_u[j] for j < lengths[u], exact 0 for lengths[u] <= j < n_max; columns n_max .. ld_out are not
 *  written.  int16 samples are scaled by 2^-15, which is exact: the bits of numpy's `astype(float32) / 32768`; fp32 is copied.
 *  Rejected (non-zero, nothing launched): null pointers, another dtype tag, B outside [1, 65535], n_max outside [0, 2^30],
 *  ld_out < n_max, packed_elems negative / not a multiple of 8 / >= 2^31, a misaligned packed or out.  n_max == 0 launches nothing.
 *  The per-utterance arrays live on the device, so the CALLER checks them (asr_amd.ops.wave_unpack does, on the host values it uploads);
 *  the kernel re-checks each row it is given — src_index in range, offset >= 0 and a multiple of 8, length in [0, n_max], the rounded-up
 *  end inside packed_elems — and writes a row that fails as zeros: nothing outside the two buffers is read or written.
 *  One kernel (wave_unpack_kernel, csrc/stft.hip), one pass: a 128-bit load per 8 int16 samples (two per 8 fp32), two 128-bit stores; no atomics. */
int ds2_wave_unpack_f32(const void* packed, long long packed_elems, int dtype, const int* offsets_dev, const int* lengths_dev,
                        const int* src_index_dev, int B, int n_max, float* out, long long ld_out, void* stream);

/* ---- sample-rate conversion in the packed waveform feed (get_loader(front_end="gpu", resample=True)) -----------
 * The reference converts its corpus outside the loader: audio/wav_converter.py runs `ffmpeg -ar 16000` over every file and audio_with_sox
 * (audio/functional.py) `sox -r` per noise segment.  Neither tool is part of the reference tree: PARITY WITH SOX AND FFMPEG IS UNPINNED.
 * The contract below — band-limited sinc interpolation with a Kaiser window — is what tests/resample_oracle.py restates.
 * Per utterance: source rate fs, target rate ft, g = gcd(fs, ft), L = ft / g, M = fs / g; x[0..n), reads outside [0, n) give 0.
 *  n_out = ceil(n L / M) in 64-bit integers (ds2_resample_out_samples, a host function; -1 for n outside [0, 2^31] or L, M < 1).
 *  Output sample m sits at input time m M / L: i0 = (m M) div L, phase p = (m M) mod L, exact integers, and
 *      y[m] = sum_{j in [0, P)} tab[p][j] * x[i0 - J + 1 + j],   P = 2 J.
 *  The table is the CALLER's (asr_amd.ops.resample_taps builds it in fp64 and rounds to fp32, as dft_basis does for the STFT):
 *      tab[p][j] = fp32( s sinc(s tau) w(tau) ),  tau = p / L + J - 1 - j,  sinc(t) = sin(pi t) / (pi t),
 *      s = rolloff min(1, L / M),  J = ceil(zeros / s),  w(tau) = I0(beta sqrt(1 - (tau s / zeros)^2)) / I0(beta) for |tau| <= zeros / s, else 0;
 *  defaults zeros = 32, rolloff = 0.945, beta = 9.0 (P = 204, 188, 94, 68 for 48, 44.1, 22.05 and 8 kHz -> 16 kHz).
 *  The device accumulates in fp32, j ascending, one fused multiply-add per tap; no atomics, reruns are bit-identical.
 *  An utterance with L = M = 1 is copied bit for bit (its J and tab_base are not used).
 * ds2_wave_resample_f32 is the ds2_wave_unpack_f32 contract with more arguments.  Unchanged: packed / packed_elems / dtype (int16 scaled
 *  by 2^-15), the 8-element ALIGNMENT RULE, offsets_dev, lengths_dev (SOURCE samples), src_index_dev.  New: L_dev, M_dev, J_dev,
 *  tab_base_dev, (B) int32 DEVICE arrays indexed by utterance like offsets; tab (tab_elems) fp32 device, the concatenated tables:
 *  utterance u reads tab[tab_base[u] + p * 2 J[u] + j]; out (B, ld_out) fp32 device, ld_out >= n_out_max: row b holds the resampled
 *  utterance u = src_index[b] in [0, n_out_u) and exact zeros in [n_out_u, n_out_max); columns n_out_max .. ld_out are not written.
 *  Rejected (non-zero, nothing launched): everything ds2_wave_unpack_f32 rejects (n_out_max in place of n_max: outside [0, 2^30]), a null
 *  per-utterance array, tab_elems outside [0, 2^22], a null tab with tab_elems > 0, a tab that is not 4-byte aligned.
 *  The per-utterance arrays live on the device, so the CALLER checks them (asr_amd.ops.wave_resample does, on the host values it uploads);
 *  the kernel re-checks each row it is given — the ds2_wave_unpack_f32 row checks, 1 <= L, M <= 2^16 with M <= 8 L and L <= 8 M, and unless
 *  L = M = 1: 1 <= J <= 512, tab_base >= 0, tab_base + L * 2 J <= tab_elems; n_out in [0, n_out_max] — and writes a row that fails as
 *  zeros: nothing outside the three buffers is read or written.
 *  One kernel (wave_resample_kernel, csrc/resample.h): one workgroup per (row, tile of ds2_resample_tile_samples() outputs), the
 *  tile's input window staged once in LDS. */
long long ds2_resample_out_samples(long long n, int L, int M);
int ds2_resample_tile_samples(void);
int ds2_wave_resample_f32(const void* packed, long long packed_elems, int dtype, const int* offsets_dev, const int* lengths_dev,
                          const int* src_index_dev, const int* L_dev, const int* M_dev, const int* J_dev, const int* tab_base_dev,
                          const float* tab, long long tab_elems, int B, int n_out_max, float* out, long long ld_out, void* stream);

/* ---- reverberation of the waveform batch (GpuSpectrogramFrontEnd(reverb=...), audio_conf.rir_dir) ---------------
 * Multi-condition training (Ko et al. 2017, "A study on data augmentation of reverberant speech for robust speech recognition"): an
 * utterance is convolved with a room impulse response (RIR) before the noise goes in.  The reference has no such step; the contract
 * below is what tests/reverb_oracle.py restates in fp64.
 * Per row b: x = the n_b samples of audio[b], h = the P_b taps rir[rir_base[b] .. rir_base[b] + P_b).  The truncated causal convolution
 *      y[i] = sum_{k = 0 .. min(i, P_b - 1)} h[k] * x[i - k],   i in [0, n_b)
 *  out[b][i] = y[i] for i < n_b, exact 0 for n_b <= i < n_max; columns n_max .. ld_out are not written.  The tail beyond n_b is dropped:
 *  the utterance keeps its length (sort, frame counts and CTC sizes stay valid); the bank (asr_amd.data.ImpulseResponses) puts the direct
 *  path at lag 0, so nothing shifts in time.
 *  Arithmetic: fp32 products, fp32 accumulation, one fused multiply-add per tap in a FIXED order (tap chunks of ds2_reverb_tap_chunk()
 *  ascending, inside a chunk the taps descending); no atomics; reruns are bit-identical, and a row's bits depend only on (x, h) — not on
 *  its position in the batch, on B or on n_max.  DENORMALS: subnormal products and sums may be flushed to zero (today's kernel keeps
 *  them; callers must not rely on either).  Non-finite samples inside [0, n_b) are outside the contract (0 * inf).
 *  P_b == 0: "not reverberated" — the row is copied bit for bit and zero-filled to n_max.
 *  Samples of audio[b] at and beyond n_b may hold anything, NaN included: they never reach the output (ds2_tempo_gain_f32's input rule).
 *  out must not alias audio.
 * ds2_reverb_f32: audio (B, ld_audio) fp32 device; n_samples_dev (B) int32 device; rir (rir_elems) fp32 device, ONE bank of concatenated
 *  responses; rir_base_dev (B) int64 device; rir_taps_dev (B) int32 device; out (B, ld_out) fp32 device.
 *  Rejected (non-zero, nothing launched): null pointers (rir may be NULL when rir_elems == 0), pointers not aligned to their element
 *  size, out == audio, B outside [1, 65535], n_max outside [0, 2^30], ld_out < n_max, ld_audio < n_max, rir_elems outside [0, 2^31).
 *  n_max == 0 is accepted and launches nothing.
 *  The per-row arrays live on the device, so the CALLER checks them (asr_amd.ops.reverb does, on the host values it uploads); the kernel
 *  re-checks each row — n_b in [0, n_max], P_b in [0, ds2_reverb_max_taps()], rir_base >= 0, rir_base + P_b <= rir_elems — and writes
 *  a row that fails as zeros: nothing outside the three buffers is read or written.
 *  One kernel (reverb_kernel, csrc/reverb.h) on v_mfma_f32_16x16x4_f32, a FIR filter being a GEMM with a Toeplitz operand: one
 *  workgroup per (row, tile of ds2_reverb_tile_samples() outputs), looping over tap chunks; the tile's x window and the chunk's taps
 *  are staged in LDS.  ds2_reverb_max_taps() = 16384 (1.02 s at 16 kHz). */
int ds2_reverb_max_taps(void);
int ds2_reverb_tile_samples(void);
int ds2_reverb_tap_chunk(void);
int ds2_reverb_f32(const float* audio, long long ld_audio, const int* n_samples_dev, const float* rir, long long rir_elems,
                   const long long* rir_base_dev, const int* rir_taps_dev, int B, int n_max, float* out, long long ld_out, void* stream);

/* ---- optimizer ----------------------------------------------------------------------------------
 * torch.optim.AdamW.step over one flat parameter buffer, trainers/__main__.py:41-47. */
int ds2_adamw_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, float grad_scale, void* stream);
/* the same update behind a device-side gate: apply_flag (device int, may be NULL = always) is read when the kernel runs, 0 = no-op */
int ds2_adamw_gated_f32(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float grad_scale, const int* apply_flag, void* stream);
int ds2_scale_f32(float* x, long long n, float s, void* stream);
/* fp32 mode, conv2 on the bf16 matrix cores (three-term split products; engine.F32_CONV): r = x - float(bf16(x)) — the bf16 mode's cast / pack
 * entries applied to r give the "lo" operand — and out = a + b + c for the partial results (out may alias a; c may be NULL: out = a + b). */
int ds2_bf16_residual_f32(const float* x, float* r, long long n, void* stream);
int ds2_sum3_f32(const float* a, const float* b, const float* c, float* out, long long n, void* stream);
/* x[0..n) += v (int64): every BatchNorm's num_batches_tracked (torch.nn.BatchNorm*d.forward in training mode) in one launch */
int ds2_add_i64(long long* x, int n, long long v, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DS2HIP_H */
