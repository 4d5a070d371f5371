"""Typed torch-tensor wrappers over the libds2hip C-ABI (device pointers + current HIP stream).

PyTorch is plumbing here: it owns device memory (caching allocator), streams and RCCL; every FLOP of
the DeepSpeech2 step is executed by the hand-written gfx950 kernels behind `asr_amd/_lib.py`.
Nothing in this module has a CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

Tensor = torch.Tensor
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DS2LibraryError("asr_amd kernels need GPU tensors (no CPU fallback exists)")
        if t.dtype != torch.float32:
            raise TypeError(f"expected float32 tensor, got {t.dtype}")


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


class RnnCtx(C.Structure):
    """include/ds2hip.h `ds2_rnn_ctx`: everything the recurrence entry points remember between calls, owned by the CALLER (the library
    keeps no mutable global state).  One per (thread, device): two Python threads driving two streams never see each other's kernel-path
    bits, cooldown, enable switches or starvation record."""
    _fields_ = [("size", C.c_int), ("persist_fwd", C.c_int), ("persist_bwd", C.c_int), ("cooldown", C.c_int), ("rearm_calls", C.c_int),
                ("starved_total", C.c_int), ("last_path", C.c_int), ("last_bwd_kind", C.c_int), ("debug_flags", C.c_int),
                ("reserved", C.c_int * 7), ("status_dev", C.c_void_p), ("poison_host", C.c_void_p), ("poison_dev", C.c_void_p)]


_RNN_TLS = threading.local()
_RNN_REGISTRY = []                      # every context ever created: (ctx, status tensor, pinned word, uid) — kept for the life of the process, so
_RNN_REGISTRY_LOCK = threading.Lock()   # a kernel still queued on some stream can never write into memory the caching allocator has handed on
_RNN_UID = {}                           # ctypes address of a context -> its monotonically increasing id (never reused, unlike thread idents)


def _pinned_word():
    """(tensor, host address, device address) of one pinned, mapped int32 word — or (None, None, None) when the runtime will not map it."""
    try:
        t = torch.zeros(16, dtype=torch.int32).pin_memory()
        hip = C.CDLL("libamdhip64.so")
        dptr = C.c_void_p()
        if hip.hipHostGetDevicePointer(C.byref(dptr), C.c_void_p(t.data_ptr()), 0) == 0 and dptr.value:
            return t, t.data_ptr(), dptr.value
    except (OSError, RuntimeError):
        pass
    return None, None, None


def _dev_key(device=None):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return dev, (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())


def rnn_ctx(device=None) -> RnnCtx:
    """The recurrence context the calling thread uses on `device` (default: the current CUDA device): the one bound with use_rnn_ctx() if any
    (an autograd worker thread running the backward of a forward that another thread issued), else the thread's own, created on first use:
    the struct itself, its 8-int device status record and its pinned poison word are allocated HERE, by the caller of the C ABI."""
    dev, key = _dev_key(device)
    bound = getattr(_RNN_TLS, "bound", None)
    if bound and key in bound[-1]:
        return bound[-1][key]
    table = getattr(_RNN_TLS, "ctx", None)
    if table is None:
        table = _RNN_TLS.ctx = {}
    if key not in table:
        ctx = RnnCtx()
        status = torch.zeros(8, dtype=torch.int32, device=dev)
        pin, phost, pdev = _pinned_word()
        torch.cuda.synchronize(dev)                                   # the status record is zero before the first launch reads it
        _lib.check(_lib.load().ds2_rnn_ctx_init(C.addressof(ctx), status.data_ptr(), phost, pdev), "ds2_rnn_ctx_init")
        assert ctx.size == C.sizeof(RnnCtx), "ds2_rnn_ctx layout mismatch between include/ds2hip.h and asr_amd/ops.py"
        with _RNN_REGISTRY_LOCK:
            uid = len(_RNN_REGISTRY)
            _RNN_REGISTRY.append((ctx, status, pin, uid))
            _RNN_UID[C.addressof(ctx)] = uid
        table[key] = ctx
    return table[key]


class use_rnn_ctx:
    """`with use_rnn_ctx(ctx, device):` — inside the block the CALLING thread's recurrence calls on `device` go through `ctx` instead of the
    thread's own context.  asr_amd.modules.deepspeech binds the context of the thread that ran forward around engine.backward: `loss.backward()`
    runs on PyTorch's autograd worker thread, and the enable switches, debug selectors, starvation record and cooldown that the forward thread
    (the trainer) set and reads must be the ones the backward recurrences see and write."""

    def __init__(self, ctx: RnnCtx, device=None):
        self.ctx, self.key = ctx, _dev_key(device)[1]

    def __enter__(self):
        stack = getattr(_RNN_TLS, "bound", None)
        if stack is None:
            stack = _RNN_TLS.bound = []
        top = dict(stack[-1]) if stack else {}
        top[self.key] = self.ctx
        stack.append(top)
        return self.ctx

    def __exit__(self, *exc):
        _RNN_TLS.bound.pop()
        return False


def _ctxp(device=None) -> int:
    return C.addressof(rnn_ctx(device))


def rnn_ctx_key(device=None):
    """hashable identity of the context in use (host-side caches of "what did the last call of this shape do" are keyed with it): a
    monotonically increasing id, never reused by a later thread or context"""
    return _RNN_UID[_ctxp(device)]


def debug_flags(flags: int, device=None) -> int:
    """ds2_debug_flags on the calling thread's context: kernel-family selectors of the recurrence; returns the previous value."""
    return _lib.load().ds2_debug_flags(_ctxp(device), int(flags))


def _row_pitch(t: Tensor) -> int:
    """pitch (elements) of a 2-D row-major (possibly column-sliced) view."""
    assert t.dim() == 2 and t.stride(1) == 1, "need a row-major 2-D view"
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
def gemm_raw(transA: bool, transB: bool, M: int, N: int, K: int, A_ptr: int, lda: int, sA: int, B_ptr: int, ldb: int, sB: int,
             C_ptr: int, ldc: int, sC: int, device, bias: Optional[Tensor] = None, accumulate: bool = False, batch: int = 1,
             splitk: int = 0):
    lib = _lib.load()
    if splitk <= 0:
        tiles = ((M + 127) // 128) * ((N + 127) // 128) * batch
        splitk = 1
        if M <= 32 and K >= 4096:          # skinny weight gradient (the fc block: dW = dlogits^T Xn, 29 classes, K = T*B): a block's k-loop is
            # one HBM round trip per 16-deep tile with little else resident on its CU - more, shorter blocks hide it; the slabs are tiny
            splitk = max(1, min((1024 + tiles - 1) // tiles, K // 256))
        elif tiles < 400 and K >= 2048:      # under-filled grid with a long reduction: aim at >= 2 blocks per CU
            splitk = max(1, min((512 + tiles - 1) // tiles, K // 1024))
        elif tiles < 128 and K >= 1024:
            splitk = max(1, min((384 + tiles - 1) // tiles, K // 256))
    ws = None
    wsb = 0
    if splitk > 1:
        wsb = lib.ds2_gemm_f32_workspace_bytes(M, N, batch, splitk)
        ws = _ws(wsb, device)
    _lib.check(lib.ds2_gemm_f32(int(transA), int(transB), M, N, K, A_ptr, lda, sA, B_ptr, ldb, sB, C_ptr, ldc, sC, _ptr(bias),
                                int(accumulate), batch, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_f32")


def gemm(A: Tensor, B: Tensor, transA: bool = False, transB: bool = False, bias: Optional[Tensor] = None,
         out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[M,N] (+)= op(A) @ op(B) (+ bias).  A, B, out: 2-D row-major views (column slices allowed)."""
    _chk_f32(A, B, bias, out)
    M, K = (A.size(1), A.size(0)) if transA else (A.size(0), A.size(1))
    N = B.size(0) if transB else B.size(1)
    Kb = B.size(1) if transB else B.size(0)
    assert K == Kb, (A.shape, B.shape, transA, transB)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    gemm_raw(transA, transB, M, N, K, A.data_ptr(), _row_pitch(A), 0, B.data_ptr(), _row_pitch(B), 0, out.data_ptr(),
             _row_pitch(out), 0, A.device, bias, accumulate)
    return out


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def cast_bf16(src: Tensor, ld: Optional[int] = None) -> Tensor:
    """(R, C) fp32 row-major view -> (R, ld or pad8(C)) bf16, pad columns zero."""
    _chk_f32(src)
    R, Cc = src.shape
    ld = _pad8(Cc) if ld is None else ld
    assert ld >= Cc and ld % 8 == 0
    dst = torch.empty(R, ld, dtype=torch.bfloat16, device=src.device)
    _lib.check(_lib.load().ds2_cast_bf16(src.data_ptr(), _row_pitch(src), dst.data_ptr(), dst.size(1), R, Cc, _stream()), "ds2_cast_bf16")
    return dst


def cast_transpose_bf16(src: Tensor, colsum: Optional[Tensor] = None) -> Tensor:
    """(R, C) fp32 row-major view -> (C, pad8(R)) bf16 = src^T, pad columns zero.
    colsum: optional contiguous fp32 tensor of C elements that receives the column sums of src from the same read."""
    _chk_f32(src)
    R, Cc = src.shape
    lib = _lib.load()
    dst = torch.empty(Cc, _pad8(R), dtype=torch.bfloat16, device=src.device)
    if colsum is None:
        _lib.check(lib.ds2_cast_transpose_bf16(src.data_ptr(), _row_pitch(src), dst.data_ptr(), dst.size(1), R, Cc, _stream()),
                   "ds2_cast_transpose_bf16")
        return dst
    assert colsum.dtype == torch.float32 and colsum.is_cuda and colsum.is_contiguous() and colsum.numel() == Cc
    wsb = lib.ds2_cast_bf16_both_workspace_bytes(R, Cc)
    ws = _ws(wsb, src.device)
    _lib.check(lib.ds2_cast_bf16_both(src.data_ptr(), _row_pitch(src), 0, 0, dst.data_ptr(), dst.size(1), R, Cc, colsum.data_ptr(),
                                      ws.data_ptr(), wsb, _stream()), "ds2_cast_bf16_both")
    return dst


def cast_bf16_both(src: Tensor, colsum: bool = False, ld_r: Optional[int] = None):
    """(R, C) fp32 -> (bf16 (R, ld_r or pad8(C)), bf16 (C, pad8(R)) = src^T[, fp32 column sums (C)]) from one read of src; pads zero."""
    _chk_f32(src)
    R, Cc = src.shape
    lib = _lib.load()
    ld_r = _pad8(Cc) if ld_r is None else ld_r
    assert ld_r >= Cc and ld_r % 8 == 0
    dst_r = torch.empty(R, ld_r, dtype=torch.bfloat16, device=src.device)
    dst_t = torch.empty(Cc, _pad8(R), dtype=torch.bfloat16, device=src.device)
    cs, ws, wsb = None, None, 0
    if colsum:
        cs = torch.empty(Cc, dtype=torch.float32, device=src.device)
        wsb = lib.ds2_cast_bf16_both_workspace_bytes(R, Cc)
        ws = _ws(wsb, src.device)
    _lib.check(lib.ds2_cast_bf16_both(src.data_ptr(), _row_pitch(src), dst_r.data_ptr(), dst_r.size(1), dst_t.data_ptr(), dst_t.size(1),
                                      R, Cc, _ptr(cs), _ptr(ws), wsb, _stream()), "ds2_cast_bf16_both")
    return (dst_r, dst_t, cs) if colsum else (dst_r, dst_t)


def transpose_bf16(src: Tensor, colsum=False):
    """(R, C) bf16 row-major -> bf16 (C, pad8(R)) = src^T [, fp32 column sums (C)] from one read; pads zero.
    colsum: False | True (new tensor) | a contiguous fp32 tensor of C elements that receives the sums (e.g. a bias-gradient slice)."""
    assert src.dtype == torch.bfloat16 and src.is_cuda and src.dim() == 2 and src.stride(1) == 1 and src.stride(0) % 8 == 0
    R, Cc = src.shape
    lib = _lib.load()
    dst_t = torch.empty(Cc, _pad8(R), dtype=torch.bfloat16, device=src.device)
    cs, ws, wsb = None, None, 0
    if colsum is not False and colsum is not None:
        cs = torch.empty(Cc, dtype=torch.float32, device=src.device) if colsum is True else colsum
        assert cs.dtype == torch.float32 and cs.is_cuda and cs.is_contiguous() and cs.numel() == Cc
        wsb = lib.ds2_cast_bf16_both_workspace_bytes(R, Cc)
        ws = _ws(wsb, src.device)
    _lib.check(lib.ds2_transpose_bf16(src.data_ptr(), src.stride(0), dst_t.data_ptr(), dst_t.size(1), R, Cc, _ptr(cs), _ptr(ws), wsb,
                                      _stream()), "ds2_transpose_bf16")
    return (dst_t, cs) if cs is not None else dst_t


def _pick_splitk(M: int, N: int, K: int) -> int:
    """Split-K factor for the bf16 GEMM: trade chip fill (256 CUs, one 256x256 tile each per round) against the fp32 partial
    slabs a split writes and re-reads.  Rates are the measured ones (scripts/bench_gemm.py): ~1.1 PF/s per busy CU-round for the
    256-tile kernel, ~3 TB/s for slab traffic."""
    if M >= 256 and N >= 256:
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        best, best_cost = 1, None
        for s in (1, 2, 3, 4, 6, 8, 12, 16):
            if s > 1 and K // s < 1024:
                break
            rounds = -(-tiles * s // 256)
            util = tiles * s / (rounds * 256.0)
            cost = 2.0 * M * N * K / (1.1e15 * util) + (0.0 if s == 1 else (s + 1) * M * N * 4 / 3e12)
            if best_cost is None or cost < best_cost * 0.97:
                best, best_cost = s, cost
        return best
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if tiles < 400 and K >= 4096:
        return max(1, min((768 + tiles - 1) // tiles, K // 2048))
    return 1


def gemm_bf16_nt_obf16(A: Tensor, B: Tensor, bias: Optional[Tensor] = None) -> Optional[Tensor]:
    """bf16 (M, N) = A[M,K] @ B[N,K]^T + bias with fp32 accumulation, ONE rounding at the store — or None where the four-wave kernel does not
    apply (the caller then takes gemm_bf16_nt's fp32 result)."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and A.is_cuda and B.is_cuda and A.stride(1) == 1 and B.stride(1) == 1
    M, K = A.shape
    N, Kb = B.shape
    assert K == Kb and K % 8 == 0, (A.shape, B.shape)
    if N % 8:
        return None
    out = torch.empty(M, N, dtype=torch.bfloat16, device=A.device)
    rc = _lib.load().ds2_gemm_bf16_nt_obf16(M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), N, _ptr(bias), _stream())
    if rc == 1:
        return None
    _lib.check(rc, "ds2_gemm_bf16_nt_obf16")
    return out


def widen_bf16(x: Tensor) -> Tensor:
    """contiguous bf16 -> fp32 (numel % 8 == 0)"""
    assert x.dtype == torch.bfloat16 and x.is_cuda and x.is_contiguous() and x.numel() % 8 == 0
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ds2_cast_f32_from_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "ds2_cast_f32_from_bf16")
    return out


def gemm_bf16_nt(A: Tensor, B: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None, accumulate: bool = False,
                 splitk: int = 0) -> Tensor:
    """out[M,N] fp32 (+)= A[M,K] @ B[N,K]^T, A/B bf16 with K (incl. zero padding) a multiple of 8."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and A.is_cuda and B.is_cuda and A.stride(1) == 1 and B.stride(1) == 1
    lib = _lib.load()
    M, K = A.shape
    N, Kb = B.shape
    assert K == Kb and K % 8 == 0, (A.shape, B.shape)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    if splitk <= 0:
        splitk = _pick_splitk(M, N, K)
    ws, wsb = None, 0
    if splitk > 1:
        wsb = lib.ds2_gemm_bf16_workspace_bytes(M, N, 1, splitk)
        ws = _ws(wsb, A.device)
    _lib.check(lib.ds2_gemm_bf16_nt(M, N, K, A.data_ptr(), A.stride(0), 0, B.data_ptr(), B.stride(0), 0, out.data_ptr(), _row_pitch(out), 0,
                                    _ptr(bias), int(accumulate), 1, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_nt")
    return out


def gemm_bf16_nt_pair(A0: Tensor, A1: Tensor, B0: Tensor, B1: Tensor, out: Tensor):
    """Two equal-shape NT products in ONE launch (batch = 2): out[d] (M, N) = A_d (M, K) @ B_d (N, K)^T.  A0/A1 (and B0/B1) must be
    views of one bf16 buffer with equal pitches; out (2, M, N) fp32 with equal-pitch slices.  Used for the two directions of dW_hh:
    twice the tiles per launch means half the split-K factor (and half the partial-slab traffic) for the same chip fill."""
    for t in (A0, A1, B0, B1):
        assert t.dtype == torch.bfloat16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1
    assert A0.shape == A1.shape and B0.shape == B1.shape and A0.stride(0) == A1.stride(0) and B0.stride(0) == B1.stride(0)
    M, K = A0.shape
    N = B0.size(0)
    assert B0.size(1) == K and K % 8 == 0 and out.dim() == 3 and out.size(0) == 2 and tuple(out.shape[1:]) == (M, N) and out.stride(2) == 1
    sA, sB = (A1.data_ptr() - A0.data_ptr()) // 2, (B1.data_ptr() - B0.data_ptr()) // 2
    assert (A1.data_ptr() - A0.data_ptr()) % 16 == 0 and (B1.data_ptr() - B0.data_ptr()) % 16 == 0
    lib = _lib.load()
    splitk = _pick_splitk(M, 2 * N, K)                 # chip fill is decided by the tiles of both products together
    ws, wsb = None, 0
    if splitk > 1:
        wsb = lib.ds2_gemm_bf16_workspace_bytes(M, N, 2, splitk)
        ws = _ws(wsb, A0.device)
    _lib.check(lib.ds2_gemm_bf16_nt(M, N, K, A0.data_ptr(), A0.stride(0), sA, B0.data_ptr(), B0.stride(0), sB, out.data_ptr(), out.stride(1),
                                    out.stride(0), None, 0, 2, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_nt")
    return out


def gemm_bf16_tn(A: Tensor, B: Tensor, out: Optional[Tensor] = None, accumulate: bool = False, splitk: int = 0) -> Tensor:
    """out[M,N] fp32 (+)= A[K,M]^T @ B[K,N]: A, B bf16 row-major views (column stride 1, any row pitch % 8 == 0) sharing the K rows."""
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and A.is_cuda and B.is_cuda and A.stride(1) == 1 and B.stride(1) == 1
    lib = _lib.load()
    K, M = A.shape
    Kb, N = B.shape
    assert K == Kb, (A.shape, B.shape)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    if splitk <= 0:
        splitk = _pick_splitk(M, N, K)
    ws, wsb = None, 0
    if splitk > 1:
        wsb = lib.ds2_gemm_bf16_workspace_bytes(M, N, 1, splitk)
        ws = _ws(wsb, A.device)
    _lib.check(lib.ds2_gemm_bf16_tn(M, N, K, A.data_ptr(), A.stride(0), 0, B.data_ptr(), B.stride(0), 0, out.data_ptr(), _row_pitch(out), 0,
                                    int(accumulate), 1, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_tn")
    return out


def gemm_bf16_tn_pair(A0: Tensor, A1: Tensor, B0: Tensor, B1: Tensor, out: Tensor, accumulate: bool = False):
    """Two equal-shape TN products in ONE launch: out[d] (M, N) = A_d (K, M)^T @ B_d (K, N).  A0/A1 (and B0/B1) are views of one bf16
    buffer with equal pitches (the two directions of dW_hh: column blocks of dGx / h at row offsets of +-B)."""
    for t in (A0, A1, B0, B1):
        assert t.dtype == torch.bfloat16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1
    assert A0.shape == A1.shape and B0.shape == B1.shape and A0.stride(0) == A1.stride(0) and B0.stride(0) == B1.stride(0)
    K, M = A0.shape
    N = B0.size(1)
    assert B0.size(0) == K and out.dim() == 3 and out.size(0) == 2 and tuple(out.shape[1:]) == (M, N) and out.stride(2) == 1
    dA, dB = A1.data_ptr() - A0.data_ptr(), B1.data_ptr() - B0.data_ptr()
    assert dA % 16 == 0 and dB % 16 == 0
    lib = _lib.load()
    splitk = _pick_splitk(M, 2 * N, K)
    ws, wsb = None, 0
    if splitk > 1:
        wsb = lib.ds2_gemm_bf16_workspace_bytes(M, N, 2, splitk)
        ws = _ws(wsb, A0.device)
    _lib.check(lib.ds2_gemm_bf16_tn(M, N, K, A0.data_ptr(), A0.stride(0), dA // 2, B0.data_ptr(), B0.stride(0), dB // 2, out.data_ptr(),
                                    out.stride(1), out.stride(0), int(accumulate), 2, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_tn")
    return out


def split_bf16(X: Tensor, order: int, pad_rows: int = 0) -> Tensor:
    """fp32 (R, C) row-major view -> its split bf16 operand (R, n * pad8(C)): x = hi + lo, hi = bf16(x), lo = bf16(x - hi); order 0 = [hi | hi | lo]
    (A operand of the fp32 mode's three-term product), 1 = [hi | lo | hi] (B operand), 2 = [hi | lo] (TN products).  See ds2_split_bf16.
    pad_rows: the result has its row count rounded up to a multiple of it, the extra rows ZERO — as the K-row-major operand of a TN product
    (reduction index = rows) it then has a reduction length the four-wave kernel takes (K % 64 == 0), and the zero rows add nothing."""
    _chk_f32(X)
    assert X.dim() == 2 and X.stride(1) == 1 and order in (0, 1, 2)
    R, Cc = X.shape
    Cp = (Cc + 7) // 8 * 8
    Rp = -(-R // pad_rows) * pad_rows if pad_rows else R
    out = torch.empty(Rp, (2 if order == 2 else 3) * Cp, dtype=torch.bfloat16, device=X.device)
    lib = _lib.load()
    if Rp > R:
        _lib.check(lib.ds2_memset_async(out[R:].data_ptr(), 0, (Rp - R) * out.stride(0) * 2, _stream()), "ds2_memset_async")
    _lib.check(lib.ds2_split_bf16(X.data_ptr(), _row_pitch(X), out.data_ptr(), out.stride(0), R, Cc, order, _stream()), "ds2_split_bf16")
    return out


def _tn_problem_array(problems):
    arr = (_lib.TnProblem * len(problems))()
    for q, (A, B, out) in zip(arr, problems):
        assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and out.dtype == torch.float32 and A.is_cuda and B.is_cuda and out.is_cuda
        assert A.dim() == 2 and B.dim() == 2 and out.dim() == 2 and A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
        K, M = A.shape
        assert B.size(0) == K and tuple(out.shape) == (M, B.size(1)), (A.shape, B.shape, out.shape)
        q.A, q.B, q.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, B.size(1), K, _row_pitch(A), _row_pitch(B), _row_pitch(out)
    return arr


def gemm_bf16_tn_splitk_group(problems, splitk: int = 0, epilogue=None):
    """Several TN products `[(A (K, M), B (K, N), out (M, N))]` in ONE launch of the 256 x 256 kernel with a common split-K factor and one reduce
    launch (ds2_gemm_bf16_tn_splitk_group).  splitk 0: chosen so that tiles x splitk fills whole rounds of the chip (the cost model of
    _pick_splitk over the tiles of all products together)."""
    lib = _lib.load()
    arr = _tn_problem_array(problems)
    if splitk <= 0:
        tiles = sum(((q.M + 255) // 256) * ((q.N + 255) // 256) for q in arr)
        kmin = min(q.K for q in arr)
        mn = sum(q.M * q.N for q in arr)
        best, best_cost = 1, None
        for s_ in (1, 2, 3, 4, 5, 6, 8, 12, 16):
            if s_ > 1 and kmin // s_ < 1024:
                break
            rounds = -(-tiles * s_ // 256)
            util = tiles * s_ / (rounds * 256.0)
            cost = 2.0 * mn * kmin / (1.1e15 * util) + (0.0 if s_ == 1 else (s_ + 1) * mn * 4 / 3e12)
            if best_cost is None or cost < best_cost * 0.97:
                best, best_cost = s_, cost
        splitk = best
    ap = C.cast(arr, C.c_void_p)
    wsb = lib.ds2_gemm_bf16_tn_splitk_group_workspace_bytes(len(problems), ap, splitk)
    ws = _ws(wsb, problems[0][0].device) if wsb else None
    if epilogue is not None:
        # epilogue = (index, scale (N), rowv (M), shift (N)): out[index] = (A^T B) diag(scale) + rowv (x) shift, applied by the reduce launch
        idx, scale, rowv, shift = epilogue
        _chk_f32(scale, rowv, shift)
        rc = lib.ds2_gemm_bf16_tn_splitk_group_ep(len(problems), ap, splitk, int(idx), scale.data_ptr(), rowv.data_ptr(), shift.data_ptr(), _ptr(ws), wsb, _stream())
        if rc == 0:
            return splitk
        if rc != 1:
            _lib.check(rc, "ds2_gemm_bf16_tn_splitk_group_ep")
        _lib.check(lib.ds2_gemm_bf16_tn_splitk_group(len(problems), ap, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_tn_splitk_group")
        scale_rank1_(problems[idx][2], scale, rowv, shift)       # (single slab: nothing reduces that product)
        return splitk
    _lib.check(lib.ds2_gemm_bf16_tn_splitk_group(len(problems), ap, splitk, _ptr(ws), wsb, _stream()), "ds2_gemm_bf16_tn_splitk_group")
    return splitk


def gemm_bf16_tn_group(problems, max_workgroups: int = 0):
    """Several TN products in ONE launch of the co-resident kernel (csrc/gemm_tn_group.h): `problems` = [(A (K, M), B (K, N), out (M, N))],
    A / B bf16 row-major views sharing their K rows, out fp32 (row pitch arbitrary, columns contiguous).  out = A^T @ B, every tile a full
    reduction over K (no split-K, no workspace)."""
    lib = _lib.load()
    arr = (_lib.TnProblem * len(problems))()
    for q, (A, B, out) in zip(arr, problems):
        assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and out.dtype == torch.float32 and A.is_cuda and B.is_cuda and out.is_cuda
        assert A.dim() == 2 and B.dim() == 2 and out.dim() == 2 and A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
        K, M = A.shape
        assert B.size(0) == K and tuple(out.shape) == (M, B.size(1)), (A.shape, B.shape, out.shape)
        q.A, q.B, q.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
        q.M, q.N, q.K, q.lda, q.ldb, q.ldc = M, B.size(1), K, _row_pitch(A), _row_pitch(B), _row_pitch(out)
    _lib.check(lib.ds2_gemm_bf16_tn_group(len(problems), C.cast(arr, C.c_void_p), int(max_workgroups), _stream()), "ds2_gemm_bf16_tn_group")


# ------------------------------------------------------------------------------------------------
# BatchNorm1d family on (M, H)
# ------------------------------------------------------------------------------------------------
def colstats(X: Tensor, run_mean: Optional[Tensor] = None, run_var: Optional[Tensor] = None):
    _chk_f32(X, run_mean, run_var)
    lib = _lib.load()
    M, H = X.shape
    mean = torch.empty(H, dtype=torch.float32, device=X.device)
    var = torch.empty_like(mean)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, X.device)
    _lib.check(lib.ds2_colstats_f32(X.data_ptr(), _row_pitch(X), M, H, mean.data_ptr(), var.data_ptr(), _ptr(run_mean),
                                    _ptr(run_var), BN_MOMENTUM, ws.data_ptr(), wsb, _stream()), "ds2_colstats_f32")
    return mean, var


def add_colstats(Xa: Tensor, Xb: Tensor, run_mean: Optional[Tensor] = None, run_var: Optional[Tensor] = None):
    """Y = Xa + Xb with column mean / biased var of Y (and optional running-stat update)."""
    _chk_f32(Xa, Xb, run_mean, run_var)
    lib = _lib.load()
    M, H = Xa.shape
    Y = torch.empty(M, H, dtype=torch.float32, device=Xa.device)
    mean = torch.empty(H, dtype=torch.float32, device=Xa.device)
    var = torch.empty_like(mean)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, Xa.device)
    _lib.check(lib.ds2_add_colstats_f32(Xa.data_ptr(), _row_pitch(Xa), Xb.data_ptr(), _row_pitch(Xb), Y.data_ptr(), H, M, H,
                                        mean.data_ptr(), var.data_ptr(), _ptr(run_mean), _ptr(run_var), BN_MOMENTUM,
                                        ws.data_ptr(), wsb, _stream()), "ds2_add_colstats_f32")
    return Y, mean, var


def center_colstats(Xa: Tensor, Xb: Tensor, hsum: Tensor, run_mean: Optional[Tensor] = None, run_var: Optional[Tensor] = None):
    """(yc bf16 (M, pad8(H)) = (Xa + Xb) - m0 with m0 the column means from `hsum` (2, tiles, H; rnn_fwd), mean, var, delta): the direction
    sum and the BatchNorm1d statistics of a recurrent layer's output in ONE pass that writes only the centred bf16 GEMM operand."""
    _chk_f32(Xa, Xb, hsum, run_mean, run_var)
    lib = _lib.load()
    M, H = Xa.shape
    assert hsum.is_contiguous() and hsum.dim() == 3 and hsum.size(0) == 2 and hsum.size(2) == H
    yc = torch.empty(M, _pad8(H), dtype=torch.bfloat16, device=Xa.device)
    stats = torch.empty(3, H, dtype=torch.float32, device=Xa.device)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H) + 4 * H
    ws = _ws(wsb, Xa.device)
    _lib.check(lib.ds2_center_colstats(Xa.data_ptr(), _row_pitch(Xa), Xb.data_ptr(), _row_pitch(Xb), hsum.data_ptr(), hsum.size(1), yc.data_ptr(), yc.size(1),
                                       M, H, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), _ptr(run_mean), _ptr(run_var), BN_MOMENTUM,
                                       ws.data_ptr(), wsb, _stream()), "ds2_center_colstats")
    return yc, stats[0], stats[1], stats[2]


def wih_fold(W: Tensor, bias: Tensor, var: Tensor, gamma: Tensor, beta: Tensor, delta: Tensor, ld: int):
    """BatchNorm1d folded into the projection behind it: (W2 bf16 (R, ld) = W diag(s), bias2 fp32 = bias + W c, s, c) with
    s = gamma rsqrt(var + eps), c = beta - delta s  (ds2_wih_fold_bf16)."""
    _chk_f32(W, bias, var, gamma, beta, delta)
    R, I = W.shape
    assert ld >= I and ld % 8 == 0 and I % 4 == 0 and W.stride(1) == 1
    W2 = torch.empty(R, ld, dtype=torch.bfloat16, device=W.device)
    bias2 = torch.empty(R, dtype=torch.float32, device=W.device)
    sc = torch.empty(2, I, dtype=torch.float32, device=W.device)
    _lib.check(_lib.load().ds2_wih_fold_bf16(W.data_ptr(), _row_pitch(W), bias.data_ptr(), R, I, var.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                             delta.data_ptr(), BN_EPS, W2.data_ptr(), ld, bias2.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), _stream()),
               "ds2_wih_fold_bf16")
    return W2, bias2, sc[0], sc[1]


def scale_rank1_(Cm: Tensor, scale: Tensor, rowv: Tensor, shift: Tensor) -> Tensor:
    """in place: C[r][c] = C[r][c] * scale[c] + rowv[r] * shift[c]"""
    _chk_f32(Cm, scale, rowv, shift)
    R, N = Cm.shape
    assert Cm.stride(1) == 1 and scale.numel() == N == shift.numel() and rowv.numel() == R and rowv.is_contiguous()
    _lib.check(_lib.load().ds2_scale_rank1_f32(Cm.data_ptr(), _row_pitch(Cm), R, N, scale.data_ptr(), rowv.data_ptr(), shift.data_ptr(), _stream()),
               "ds2_scale_rank1_f32")
    return Cm


def bn1d_bwd_sums_xbf(dY: Tensor, X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """bn1d_bwd_sums with the BatchNorm input X as bf16 (M, >= H): (sum dY, sum dY * xhat) with xhat = (X - mean) rsqrt(var + eps)."""
    _chk_f32(dY, mean, var, gamma)
    assert X.dtype == torch.bfloat16 and X.is_cuda and X.stride(1) == 1
    lib = _lib.load()
    M, H = dY.shape
    if out is None:
        both = torch.empty(2, H, dtype=torch.float32, device=dY.device)
        out = (both[0], both[1])
    s0, s1 = out
    _chk_f32(s0, s1)
    assert s0.is_contiguous() and s1.is_contiguous() and s0.numel() == H == s1.numel()
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, dY.device)
    _lib.check(lib.ds2_bn1d_bwd_xbf16(dY.data_ptr(), _row_pitch(dY), X.data_ptr(), X.stride(0), None, 0, M, H, mean.data_ptr(), var.data_ptr(),
                                      gamma.data_ptr(), BN_EPS, s1.data_ptr(), s0.data_ptr(), ws.data_ptr(), wsb, _stream()), "ds2_bn1d_bwd_xbf16")
    return s0, s1


def bn1d_bwd_xbf(dY: Tensor, X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor) -> Tensor:
    """materialised BatchNorm1d backward with the input as bf16 (the fallback of layers whose recurrence cannot fuse it)"""
    _chk_f32(dY, mean, var, gamma, dgamma, dbeta)
    assert X.dtype == torch.bfloat16 and X.is_cuda and X.stride(1) == 1
    lib = _lib.load()
    M, H = dY.shape
    dX = torch.empty(M, H, dtype=torch.float32, device=dY.device)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, dY.device)
    _lib.check(lib.ds2_bn1d_bwd_xbf16(dY.data_ptr(), _row_pitch(dY), X.data_ptr(), X.stride(0), dX.data_ptr(), H, M, H, mean.data_ptr(), var.data_ptr(),
                                      gamma.data_ptr(), BN_EPS, dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), wsb, _stream()), "ds2_bn1d_bwd_xbf16")
    return dX


def colsum(X: Tensor) -> Tensor:
    _chk_f32(X)
    lib = _lib.load()
    M, H = X.shape
    s = torch.empty(H, dtype=torch.float32, device=X.device)
    s2 = torch.empty_like(s)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, X.device)
    _lib.check(lib.ds2_colsum_f32(X.data_ptr(), _row_pitch(X), M, H, s.data_ptr(), s2.data_ptr(), ws.data_ptr(), wsb, _stream()),
               "ds2_colsum_f32")
    return s


def bn1d_apply(X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor) -> Tensor:
    _chk_f32(X, mean, var, gamma, beta)
    M, H = X.shape
    Y = torch.empty(M, H, dtype=torch.float32, device=X.device)
    _lib.check(_lib.load().ds2_bn1d_apply_f32(X.data_ptr(), _row_pitch(X), Y.data_ptr(), H, M, H, mean.data_ptr(), var.data_ptr(),
                                              gamma.data_ptr(), beta.data_ptr(), BN_EPS, _stream()), "ds2_bn1d_apply_f32")
    return Y


def bn1d_apply_bf16(X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, beta: Tensor) -> Tensor:
    """BN(X) written straight as bf16 (M, pad8(H)), pad columns zero."""
    _chk_f32(X, mean, var, gamma, beta)
    M, H = X.shape
    Y = torch.empty(M, _pad8(H), dtype=torch.bfloat16, device=X.device)
    _lib.check(_lib.load().ds2_bn1d_apply_bf16(X.data_ptr(), _row_pitch(X), Y.data_ptr(), Y.size(1), M, H, mean.data_ptr(), var.data_ptr(),
                                               gamma.data_ptr(), beta.data_ptr(), BN_EPS, _stream()), "ds2_bn1d_apply_bf16")
    return Y


def bn1d_bwd(dY: Tensor, X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor,
             dX: Optional[Tensor] = None) -> Tensor:
    _chk_f32(dY, X, mean, var, gamma, dgamma, dbeta, dX)
    lib = _lib.load()
    M, H = X.shape
    if dX is None:
        dX = torch.empty(M, H, dtype=torch.float32, device=X.device)
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, X.device)
    _lib.check(lib.ds2_bn1d_bwd_f32(dY.data_ptr(), _row_pitch(dY), X.data_ptr(), _row_pitch(X), dX.data_ptr(), _row_pitch(dX), M, H,
                                    mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), BN_EPS, dgamma.data_ptr(), dbeta.data_ptr(),
                                    ws.data_ptr(), wsb, _stream()), "ds2_bn1d_bwd_f32")
    return dX


# ------------------------------------------------------------------------------------------------
# BatchNorm2d + Hardtanh + mask on (B, C, D, T)
# ------------------------------------------------------------------------------------------------
def bn2d_stats(Y: Tensor, run_mean: Optional[Tensor] = None, run_var: Optional[Tensor] = None):
    _chk_f32(Y, run_mean, run_var)
    lib = _lib.load()
    B, Cc, D, T = Y.shape
    mean = torch.empty(Cc, dtype=torch.float32, device=Y.device)
    var = torch.empty_like(mean)
    wsb = lib.ds2_chanreduce_workspace_bytes(Cc)
    ws = _ws(wsb, Y.device)
    _lib.check(lib.ds2_bn2d_stats_f32(Y.data_ptr(), B, Cc, D, T, mean.data_ptr(), var.data_ptr(), _ptr(run_mean), _ptr(run_var),
                                      BN_MOMENTUM, ws.data_ptr(), wsb, _stream()), "ds2_bn2d_stats_f32")
    return mean, var


def bn2d_act_fwd(Y: Tensor, lens_dev: Tensor, mean, var, gamma, beta) -> Tensor:
    _chk_f32(Y, mean, var, gamma, beta)
    B, Cc, D, T = Y.shape
    A = torch.empty_like(Y)
    _lib.check(_lib.load().ds2_bn2d_act_fwd_f32(Y.data_ptr(), A.data_ptr(), B, Cc, D, T, lens_dev.data_ptr(), mean.data_ptr(),
                                                var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), BN_EPS, _stream()),
               "ds2_bn2d_act_fwd_f32")
    return A


def bn2d_act_bwd(Y: Tensor, dA: Tensor, lens_dev: Tensor, mean, var, gamma, beta, dgamma: Tensor, dbeta: Tensor) -> Tensor:
    _chk_f32(Y, dA, mean, var, gamma, beta, dgamma, dbeta)
    lib = _lib.load()
    B, Cc, D, T = Y.shape
    dY = torch.empty_like(Y)
    wsb = lib.ds2_chanreduce_workspace_bytes(Cc)
    ws = _ws(wsb, Y.device)
    _lib.check(lib.ds2_bn2d_act_bwd_f32(Y.data_ptr(), dA.data_ptr(), dY.data_ptr(), B, Cc, D, T, lens_dev.data_ptr(), mean.data_ptr(),
                                        var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), BN_EPS, dgamma.data_ptr(), dbeta.data_ptr(),
                                        ws.data_ptr(), wsb, _stream()), "ds2_bn2d_act_bwd_f32")
    return dY


def bn2d_act_fwd_fused(Y: Tensor, lens_dev: Tensor, mean, var, gamma, beta, want_f32=False, want_pad=False, want_nhwc=False):
    """bf16 mode: BatchNorm2d + Hardtanh + mask with the layout casts fused (csrc/norm.hip: bn2d_tile_kernel).  Returns
    (a_f32 (B,32,D,T) | None, a_pad (B,32,D,Tp) bf16 | None, a_nhwc (B,D,T,32) bf16 | None)."""
    _chk_f32(Y, mean, var, gamma, beta)
    lib = _lib.load()
    B, Cc, D, T = Y.shape
    assert Cc == 32 and Y.is_contiguous() and (want_f32 or want_pad or want_nhwc)
    a32 = torch.empty_like(Y) if want_f32 else None
    apad = torch.empty(B, 32, D, lib.ds2_conv_padded_pitch(T), dtype=torch.bfloat16, device=Y.device) if want_pad else None
    anh = torch.empty(B, D, T, 32, dtype=torch.bfloat16, device=Y.device) if want_nhwc else None
    _lib.check(lib.ds2_bn2d_act_fwd_fused(Y.data_ptr(), B, D, T, lens_dev.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(),
                                          beta.data_ptr(), BN_EPS, _ptr(a32), _ptr(apad), _ptr(anh), _stream()), "ds2_bn2d_act_fwd_fused")
    return a32, apad, anh


def bn2d_act_collapse(Y: Tensor, lens_dev: Tensor, mean, var, gamma, beta, want_f32=False, want_bf16=True, pad_to: int = 8):
    """bf16 mode: BatchNorm2d + Hardtanh + mask + (B,32*D,T) -> (T*B, 32*D) collapse (+ cast) in one pass over the conv output.
    Returns (x fp32 (T*B, 32*D) | None, x bf16 (T*B, 32*D rounded up to a multiple of pad_to, pad columns zero) | None)."""
    _chk_f32(Y, mean, var, gamma, beta)
    B, Cc, D, T = Y.shape
    assert Cc == 32 and Y.is_contiguous() and (want_f32 or want_bf16)
    F = 32 * D
    x32 = torch.empty(T * B, F, dtype=torch.float32, device=Y.device) if want_f32 else None
    xbf = None
    if want_bf16:
        xbf = torch.empty(T * B, -(-F // pad_to) * pad_to, dtype=torch.bfloat16, device=Y.device)      # (the kernel writes the pad columns)
    _lib.check(_lib.load().ds2_bn2d_act_collapse(Y.data_ptr(), B, D, T, lens_dev.data_ptr(), mean.data_ptr(), var.data_ptr(), gamma.data_ptr(),
                                                 beta.data_ptr(), BN_EPS, _ptr(x32), _ptr(xbf), xbf.size(1) if xbf is not None else 0, _stream()),
               "ds2_bn2d_act_collapse")
    return x32, xbf


def bn2d_act_bwd_fused(Y: Tensor, dA: Tensor, lens_dev: Tensor, mean, var, gamma, beta, dgamma: Tensor, dbeta: Tensor, dbias: Tensor,
                       want_f32=False, want_pad=False, want_nhwc=False):
    """bf16 mode: backward of the same block; writes dgamma / dbeta / dbias (the bias gradient of the convolution in front) in place and
    returns dY as (fp32 | None, zero-padded bf16 | None, channels-last bf16 | None)."""
    _chk_f32(Y, dA, mean, var, gamma, beta, dgamma, dbeta, dbias)
    lib = _lib.load()
    B, Cc, D, T = Y.shape
    assert Cc == 32 and Y.is_contiguous() and dA.is_contiguous() and dA.shape == Y.shape
    d32 = torch.empty_like(Y) if want_f32 else None
    dpad = torch.empty(B, 32, D, lib.ds2_conv_padded_pitch(T), dtype=torch.bfloat16, device=Y.device) if want_pad else None
    dnh = torch.empty(B, D, T, 32, dtype=torch.bfloat16, device=Y.device) if want_nhwc else None
    wsb = lib.ds2_bn2d_act_bwd_fused_workspace_bytes(B, D, T)
    ws = _ws(wsb, Y.device)
    _lib.check(lib.ds2_bn2d_act_bwd_fused(Y.data_ptr(), dA.data_ptr(), B, D, T, lens_dev.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                          gamma.data_ptr(), beta.data_ptr(), BN_EPS, dgamma.data_ptr(), dbeta.data_ptr(), dbias.data_ptr(),
                                          _ptr(d32), _ptr(dpad), _ptr(dnh), ws.data_ptr(), wsb, _stream()), "ds2_bn2d_act_bwd_fused")
    return d32, dpad, dnh


def chan_sum(Y: Tensor) -> Tensor:
    """per-channel sum over (B, D, T) of a (B,C,D,T) tensor (bias gradients)."""
    mean, _ = bn2d_stats(Y)
    B, Cc, D, T = Y.shape
    return mean * float(B * D * T)


def transpose_bft(src: Tensor, B: int, F: int, T: int, to_tbf: bool) -> Tensor:
    _chk_f32(src)
    dst = torch.empty((T, B, F) if to_tbf else (B, F, T), dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().ds2_transpose_bft_f32(src.data_ptr(), dst.data_ptr(), B, F, T, 0 if to_tbf else 1, _stream()),
               "ds2_transpose_bft_f32")
    return dst


def transpose_batched(src: Tensor) -> Tensor:
    """(batch, R, C) contiguous -> (batch, C, R) contiguous."""
    _chk_f32(src)
    nb, R, Cc = src.shape
    dst = torch.empty(nb, Cc, R, dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().ds2_transpose2d_f32(src.data_ptr(), Cc, R * Cc, dst.data_ptr(), R, R * Cc, R, Cc, nb, _stream()),
               "ds2_transpose2d_f32")
    return dst


# ------------------------------------------------------------------------------------------------
# conv front-end
# ------------------------------------------------------------------------------------------------
def conv_pack(w1: Tensor, w2: Tensor):
    _chk_f32(w1, w2)
    lib = _lib.load()
    dev = w1.device
    wpk1 = torch.empty(lib.ds2_conv_packed_floats(0), dtype=torch.float32, device=dev)
    wpk2 = torch.empty(lib.ds2_conv_packed_floats(1), dtype=torch.float32, device=dev)
    wpk2d = torch.empty(lib.ds2_conv_packed_floats(2), dtype=torch.float32, device=dev)
    _lib.check(lib.ds2_conv_pack_f32(w1.data_ptr(), w2.data_ptr(), wpk1.data_ptr(), wpk2.data_ptr(), wpk2d.data_ptr(), _stream()),
               "ds2_conv_pack_f32")
    return wpk1, wpk2, wpk2d


def conv1_fwd(x: Tensor, wpk1: Tensor, bias: Tensor, lens_dev: Tensor) -> Tensor:
    _chk_f32(x, wpk1, bias)
    B, _, F, Tin = x.shape
    D1, D2, T = _lib.conv_dims(F, Tin)
    y1 = torch.empty(B, 32, D1, T, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ds2_conv1_fwd_f32(x.data_ptr(), wpk1.data_ptr(), bias.data_ptr(), lens_dev.data_ptr(), y1.data_ptr(), B, F,
                                             Tin, _stream()), "ds2_conv1_fwd_f32")
    return y1


def conv2_fwd(a1: Tensor, wpk2: Tensor, bias: Tensor, lens_dev: Tensor) -> Tensor:
    _chk_f32(a1, wpk2, bias)
    B, _, D1, T = a1.shape
    D2 = (D1 + 20 - 21) // 2 + 1
    y2 = torch.empty(B, 32, D2, T, dtype=torch.float32, device=a1.device)
    _lib.check(_lib.load().ds2_conv2_fwd_f32(a1.data_ptr(), wpk2.data_ptr(), bias.data_ptr(), lens_dev.data_ptr(), y2.data_ptr(), B, D1,
                                             T, _stream()), "ds2_conv2_fwd_f32")
    return y2


def conv2_dgrad(dy2: Tensor, wpk2d: Tensor, D1: int) -> Tensor:
    _chk_f32(dy2, wpk2d)
    B, _, D2, T = dy2.shape
    da1 = torch.empty(B, 32, D1, T, dtype=torch.float32, device=dy2.device)
    _lib.check(_lib.load().ds2_conv2_dgrad_f32(dy2.data_ptr(), wpk2d.data_ptr(), da1.data_ptr(), B, D1, T, _stream()),
               "ds2_conv2_dgrad_f32")
    return da1


def conv1_wgrad(x: Tensor, dy1: Tensor, lens_dev: Tensor, dW1: Tensor):
    _chk_f32(x, dy1, dW1)
    lib = _lib.load()
    B, _, F, Tin = x.shape
    wsb = lib.ds2_conv_wgrad_workspace_bytes(0, B, F)
    ws = _ws(wsb, x.device)
    _lib.check(lib.ds2_conv1_wgrad_f32(x.data_ptr(), dy1.data_ptr(), lens_dev.data_ptr(), dW1.data_ptr(), B, F, Tin, 0, ws.data_ptr(),
                                       wsb, _stream()), "ds2_conv1_wgrad_f32")


def conv2_wgrad(a1: Tensor, dy2: Tensor, lens_dev: Tensor, dW2: Tensor):
    _chk_f32(a1, dy2, dW2)
    lib = _lib.load()
    B, _, D1, T = a1.shape
    wsb = lib.ds2_conv_wgrad_workspace_bytes(1, B, 161)
    ws = _ws(wsb, a1.device)
    _lib.check(lib.ds2_conv2_wgrad_f32(a1.data_ptr(), dy2.data_ptr(), lens_dev.data_ptr(), dW2.data_ptr(), B, D1, T, 0, ws.data_ptr(),
                                       wsb, _stream()), "ds2_conv2_wgrad_f32")


def conv1_pack_bf16(w1: Tensor) -> Tensor:
    _chk_f32(w1)
    lib = _lib.load()
    wp = torch.empty(lib.ds2_conv1_bf16_bytes(0, 0, 0, 0), dtype=torch.uint8, device=w1.device)
    _lib.check(lib.ds2_conv1_pack_bf16(w1.data_ptr(), wp.data_ptr(), _stream()), "ds2_conv1_pack_bf16")
    return wp


def conv1_gather_bf16(x: Tensor, want_fwd: bool = True, want_wgrad: bool = True):
    """x (B,1,F,Tin) fp32 -> (XB (B,F,P) bf16 rows, XB[..., 7 + s] = x[..., s], zero padded | None, X16T (B,F,16,pad64(T)) bf16 | None):
    conv1's forward / weight-gradient operand images."""
    _chk_f32(x)
    assert x.is_contiguous()
    lib = _lib.load()
    B, _, F, Tin = x.shape
    _, _, T = _lib.conv_dims(F, Tin)
    XB = torch.empty(lib.ds2_conv1_bf16_bytes(1, B, F, T) // 2, dtype=torch.bfloat16, device=x.device).view(B, F, lib.ds2_conv1_bf16_row_pitch(T)) if want_fwd else None
    X16T = torch.empty(lib.ds2_conv1_bf16_bytes(2, B, F, T) // 2, dtype=torch.bfloat16, device=x.device).view(B, F, 16, -1) if want_wgrad else None
    _lib.check(lib.ds2_conv1_gather_bf16(x.data_ptr(), _ptr(XB), _ptr(X16T), B, F, Tin, _stream()), "ds2_conv1_gather_bf16")
    return XB, X16T


def conv1_fwd_bf16(XB: Tensor, wp: Tensor, bias: Tensor, lens_dev: Tensor, Tin: int, stats: bool = False):
    """stats=True: also returns the per-block (sum, sum of squares) partials of y1's channels, taken in the epilogue (chanstats_from_partials)."""
    B, F, P = XB.shape
    D1, _, T = _lib.conv_dims(F, Tin)
    lib = _lib.load()
    assert P == lib.ds2_conv1_bf16_row_pitch(T) and XB.is_contiguous()
    y1 = torch.empty(B, 32, D1, T, dtype=torch.float32, device=XB.device)
    part = torch.empty(lib.ds2_conv1_fwd_bf16_stat_blocks(B, F, Tin), 32, 2, dtype=torch.float32, device=XB.device) if stats else None
    _lib.check(lib.ds2_conv1_fwd_bf16_stats(XB.data_ptr(), wp.data_ptr(), bias.data_ptr(), lens_dev.data_ptr(), y1.data_ptr(), B, F, Tin,
                                            _ptr(part), _stream()), "ds2_conv1_fwd_bf16")
    return (y1, part) if stats else y1


def chanstats_from_partials(part: Tensor, count: int, run_mean: Optional[Tensor] = None, run_var: Optional[Tensor] = None):
    """(nblk, C, 2) per-block channel sums of a conv forward epilogue -> (mean, biased var) over `count` elements per channel (+ running stats)."""
    _chk_f32(part, run_mean, run_var)
    nblk, Cc, _ = part.shape
    mean = torch.empty(Cc, dtype=torch.float32, device=part.device)
    var = torch.empty_like(mean)
    lib = _lib.load()
    wsb = lib.ds2_chanstats_from_partials_workspace_bytes()
    ws = _ws(wsb, part.device)
    _lib.check(lib.ds2_chanstats_from_partials(part.data_ptr(), nblk, Cc, float(count), mean.data_ptr(), var.data_ptr(), _ptr(run_mean),
                                               _ptr(run_var), BN_MOMENTUM, ws.data_ptr(), wsb, _stream()), "ds2_chanstats_from_partials")
    return mean, var


def conv1_wgrad_bf16(X16T: Tensor, dy1: Tensor, lens_dev: Tensor, dW1: Tensor, Tin: int):
    _chk_f32(dy1, dW1)
    lib = _lib.load()
    B, F = X16T.shape[0], X16T.shape[1]
    wsb = lib.ds2_conv1_wgrad_bf16_workspace_bytes(B, Tin)
    ws = _ws(wsb, dy1.device)
    _lib.check(lib.ds2_conv1_wgrad_bf16(X16T.data_ptr(), dy1.data_ptr(), lens_dev.data_ptr(), dW1.data_ptr(), B, F, Tin, ws.data_ptr(), wsb,
                                        _stream()), "ds2_conv1_wgrad_bf16")


def conv2_pack_bf16(w2: Tensor):
    _chk_f32(w2)
    lib = _lib.load()
    bufs = [torch.empty(lib.ds2_conv2_bf16_packed_bytes(i), dtype=torch.uint8, device=w2.device) for i in range(3)]
    _lib.check(lib.ds2_conv2_pack_bf16(w2.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), _stream()),
               "ds2_conv2_pack_bf16")
    return tuple(bufs)


def nhwc_bf16(x: Tensor) -> Tensor:
    """(B,32,D,T) fp32 -> (B,D,T,32) bf16 channels-last."""
    _chk_f32(x)
    B, Cc, D, T = x.shape
    assert Cc == 32 and x.is_contiguous()
    out = torch.empty(B, D, T, 32, dtype=torch.bfloat16, device=x.device)
    _lib.check(_lib.load().ds2_nhwc_bf16_f32(x.data_ptr(), out.data_ptr(), B, D, T, _stream()), "ds2_nhwc_bf16_f32")
    return out


def bf16_residual(x: Tensor) -> Tensor:
    """x - float(bf16(x)): what a bf16 operand of x drops (the "lo" term of the fp32 mode's split products on the conv stack)."""
    _chk_f32(x)
    assert x.is_contiguous()
    r = torch.empty_like(x)
    _lib.check(_lib.load().ds2_bf16_residual_f32(x.data_ptr(), r.data_ptr(), x.numel(), _stream()), "ds2_bf16_residual_f32")
    return r


def sum3_(a: Tensor, b: Tensor, c: Optional[Tensor] = None) -> Tensor:
    """a += b (+ c) in place (the partial results of a split product)."""
    _chk_f32(a, b) if c is None else _chk_f32(a, b, c)
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape and (c is None or (c.is_contiguous() and c.shape == a.shape))
    _lib.check(_lib.load().ds2_sum3_f32(a.data_ptr(), b.data_ptr(), _ptr(c), a.data_ptr(), a.numel(), _stream()), "ds2_sum3_f32")
    return a


def conv2_fwd_bf16(a1_nhwc: Tensor, wf: Tensor, bias: Tensor, lens_dev: Tensor, stats: bool = False):
    B, D1, T, _ = a1_nhwc.shape
    D2 = (D1 + 20 - 21) // 2 + 1
    lib = _lib.load()
    y2 = torch.empty(B, 32, D2, T, dtype=torch.float32, device=a1_nhwc.device)
    part = torch.empty(lib.ds2_conv2_fwd_bf16_stat_blocks(B, D1, T), 32, 2, dtype=torch.float32, device=a1_nhwc.device) if stats else None
    _lib.check(lib.ds2_conv2_fwd_bf16_stats(a1_nhwc.data_ptr(), wf.data_ptr(), bias.data_ptr(), lens_dev.data_ptr(), y2.data_ptr(), B, D1, T,
                                            _ptr(part), _stream()), "ds2_conv2_fwd_bf16")
    return (y2, part) if stats else y2


def conv2_dgrad_bf16(dy2_nhwc: Tensor, wd0: Tensor, wd1: Tensor, D1: int) -> Tensor:
    B, D2, T, _ = dy2_nhwc.shape
    da1 = torch.empty(B, 32, D1, T, dtype=torch.float32, device=dy2_nhwc.device)
    _lib.check(_lib.load().ds2_conv2_dgrad_bf16(dy2_nhwc.data_ptr(), wd0.data_ptr(), wd1.data_ptr(), da1.data_ptr(), B, D1, T, _stream()),
               "ds2_conv2_dgrad_bf16")
    return da1


def padcast_bf16(x: Tensor) -> Tensor:
    """(B,C,D,T) fp32 -> (B,C,D,Tp) bf16 with 8 leading zeros per row and a zero tail (operands of conv2_wgrad_bf16)."""
    _chk_f32(x)
    assert x.is_contiguous()
    lib = _lib.load()
    B, Cc, D, T = x.shape
    Tp = lib.ds2_conv_padded_pitch(T)
    out = torch.empty(B, Cc, D, Tp, dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.ds2_padcast_bf16(x.data_ptr(), out.data_ptr(), B * Cc * D, T, _stream()), "ds2_padcast_bf16")
    return out


def conv2_wgrad_bf16(a1p: Tensor, dy2p: Tensor, lens_dev: Tensor, dW2: Tensor, T: int):
    lib = _lib.load()
    B, _, D1, _ = a1p.shape
    wsb = lib.ds2_conv2_wgrad_bf16_workspace_bytes(B, D1)
    ws = _ws(wsb, a1p.device)
    _lib.check(lib.ds2_conv2_wgrad_bf16(a1p.data_ptr(), dy2p.data_ptr(), lens_dev.data_ptr(), dW2.data_ptr(), B, D1, T, ws.data_ptr(), wsb,
                                        _stream()), "ds2_conv2_wgrad_bf16")


def conv2_wgrad_nhwc_bf16(a1n: Tensor, dy2n: Tensor, lens_dev: Tensor, dW2: Tensor):
    """dW2 (32,32,21,11) fp32 from the channels-last bf16 operands a1n (B,D1,T,32), dy2n (B,D2,T,32) (ops.nhwc_bf16 / the fused BatchNorm2d
    kernels' nhwc outputs)."""
    lib = _lib.load()
    B, D1, T, _ = a1n.shape
    assert a1n.dtype == torch.bfloat16 and dy2n.dtype == torch.bfloat16 and a1n.is_contiguous() and dy2n.is_contiguous() and dy2n.shape[2] == T
    wsb = lib.ds2_conv2_wgrad_bf16_workspace_bytes(B, D1)
    ws = _ws(wsb, a1n.device)
    _lib.check(lib.ds2_conv2_wgrad_nhwc_bf16(a1n.data_ptr(), dy2n.data_ptr(), lens_dev.data_ptr(), dW2.data_ptr(), B, D1, T, ws.data_ptr(), wsb,
                                             _stream()), "ds2_conv2_wgrad_nhwc_bf16")


# ------------------------------------------------------------------------------------------------
# recurrence
# ------------------------------------------------------------------------------------------------
def rnn_pack(gates: int, whh: Tensor, bf16=False):
    """W_hh (2, G*H, H) fp32 -> (wp_fwd, wp_bwd) in MFMA-fragment order (fp32 or bf16 fragments; see csrc/rnn.hip).  bf16 = 2: the fp32
    mode with the SPLIT forward recurrence (rnn_fwd(bf16=2)): wp_fwd = [fp32 fragments | bf16 hi fragments | bf16 lo fragments], wp_bwd fp32."""
    _chk_f32(whh)
    assert whh.is_contiguous() and whh.dim() == 3
    lib = _lib.load()
    H = whh.size(2)
    wpf = torch.empty(lib.ds2_rnn_packed_bytes(gates, H, 0, int(bf16)), dtype=torch.uint8, device=whh.device)
    wpb = torch.empty(lib.ds2_rnn_packed_bytes(gates, H, 1, int(bf16)), dtype=torch.uint8, device=whh.device)
    _lib.check(lib.ds2_rnn_pack_whh(gates, whh.data_ptr(), wpf.data_ptr(), wpb.data_ptr(), H, int(bf16), _stream()), "ds2_rnn_pack_whh")
    return wpf, wpb


def weight_prep_bf16(layers):
    """The bf16 weight operands of a recurrent stack in ONE launch.  layers: a list of (gates, whh (2, G*H, H) or None, wih (R, C) or None,
    ld_r or None); returns a list of (wp_fwd, wp_bwd, wihT (C, pad8(R)) bf16, wih_r (R, ld_r) bf16 or None), entries None where the input
    was: the bytes rnn_pack(bf16=True), cast_transpose_bf16 and cast_bf16_both write for each layer on its own."""
    lib = _lib.load()
    tab = (_lib.PrepLayer * len(layers))()
    out = []
    for e, (gates, whh, wih, ld_r) in zip(tab, layers):
        wpf = wpb = wt = wr = None
        if whh is not None:
            _chk_f32(whh)
            assert whh.is_contiguous() and whh.dim() == 3
            dev, H = whh.device, whh.size(2)
            wpf = torch.empty(lib.ds2_rnn_packed_bytes(gates, H, 0, 1), dtype=torch.uint8, device=dev)
            wpb = torch.empty(lib.ds2_rnn_packed_bytes(gates, H, 1, 1), dtype=torch.uint8, device=dev)
            e.whh, e.wp_fwd, e.wp_bwd, e.gates, e.H = whh.data_ptr(), wpf.data_ptr(), wpb.data_ptr(), gates, H
        if wih is not None:
            _chk_f32(wih)
            R, Cc = wih.shape
            wt = torch.empty(Cc, _pad8(R), dtype=torch.bfloat16, device=wih.device)
            e.wih, e.wih_t, e.R, e.Cc, e.ld_wih, e.ld_t = wih.data_ptr(), wt.data_ptr(), R, Cc, _row_pitch(wih), wt.size(1)
            if ld_r is not None:
                assert ld_r >= Cc and ld_r % 8 == 0
                wr = torch.empty(R, ld_r, dtype=torch.bfloat16, device=wih.device)
                e.wih_r, e.ld_r = wr.data_ptr(), ld_r
        out.append((wpf, wpb, wt, wr))
    _lib.check(lib.ds2_weight_prep_bf16(tab, len(layers), _stream()), "ds2_weight_prep_bf16")
    return out


def rnn_ws(kind: str, gates: int, B: int, H: int, bf16, device) -> Tensor:
    """The workspace of ONE rnn_fwd ("fwd") / rnn_bwd / rnn_bwd_bn ("bwd") call, filled with 0xff bytes NOW, in stream order: pass it as `ws=` to
    the call.  A persistent launch needs its exchange buffers armed with that pattern; armed here — ahead of the GEMM in front of the recurrence —
    the fill is no longer a launch of its own between that GEMM and the launch that waits for every CU (the entries' `ws_armed` argument)."""
    lib = _lib.load()
    n = lib.ds2_rnn_fwd_workspace_bytes(B, H, int(bf16)) if kind == "fwd" else lib.ds2_rnn_bwd_workspace_bytes(gates, B, H, int(bf16))
    ws = _ws(n, device)
    _lib.check(lib.ds2_memset_async(ws.data_ptr(), 0xff, ws.numel(), _stream()), "ds2_memset_async")
    return ws


def _take_ws(ws: Optional[Tensor], need: int, device):
    """(workspace, armed): `ws` from rnn_ws (armed: every byte 0xff) or a fresh, un-armed one"""
    if ws is None:
        return _ws(need, device), False
    assert ws.numel() >= need and ws.device == torch.device(device)
    return ws, True


def rnn_persistent_enable(forward: bool = True, backward: bool = True, device=None) -> None:
    """Which bf16 recurrences may run as one persistent launch.  A persistent launch needs all of its workgroups resident at once, so
    the backward one must be off while collectives run on a communication stream during backward (data-parallel training)."""
    _lib.check(_lib.load().ds2_rnn_persistent_enable(_ctxp(device), int(bool(forward)), int(bool(backward))), "ds2_rnn_persistent_enable")


def rnn_persistent_check(device=None) -> None:
    """Raise if a persistent recurrence launch starved since the last call (a workgroup never saw its operand, or the launch never became
    resident: it needs every workgroup on the chip at once).  Call at a point where the device is idle anyway (the train step's loss sync)."""
    rec = (C.c_int * 8)()
    _lib.check(_lib.load().ds2_rnn_persistent_status(_ctxp(device), C.cast(rec, C.c_void_p)), "ds2_rnn_persistent_status")
    if rec[0]:
        starved, left = rnn_persistent_counters(device)
        what = {1: "forward", 2: "backward", 3: "census (launch never resident)"}.get(rec[0], str(rec[0]))
        raise _lib.DS2LibraryError(
            f"persistent recurrence starved ({what}): ids ({rec[1]}, {rec[2]}, {rec[3]}) step {rec[4]} wave {rec[5]} pending chunks {rec[6] & 0xffffffff:08x} "
            f"(L2-local exchange: {rec[7]}); the results of that step are invalid.  The next {left if left >= 0 else 'ALL'} recurrence calls run on the "
            f"one-launch-per-step kernels, then the persistent kernels are armed again (DS2_RNN_REARM_CALLS; DS2_RNN_PERSISTENT=0 selects the step "
            f"kernels from the start).  Starved launches since load: {starved}.")


def rnn_poison_if_starved(buf: Tensor) -> None:
    """In stream order, without a host synchronisation: overwrite `buf` (fp32, contiguous) with NaN if a persistent recurrence launch enqueued
    before this call has recorded starvation.  The record stays for the next rnn_persistent_check()."""
    _chk_f32(buf)
    assert buf.is_contiguous()
    _lib.check(_lib.load().ds2_rnn_poison_if_starved(_ctxp(buf.device), buf.data_ptr(), buf.numel(), _stream()), "ds2_rnn_poison_if_starved")


def rnn_poison_seen(device=None) -> bool:
    """True once a rnn_poison_if_starved kernel has actually overwritten a buffer since the last rnn_persistent_check(): a host memory read
    (no synchronisation).  A caller that sees it should run rnn_persistent_check(), which raises, clears the record and moves the next
    recurrence calls onto the step kernels."""
    return bool(_lib.load().ds2_rnn_poison_seen(_ctxp(device)))


def rnn_persistent_counters(device=None):
    """(launches through the calling thread's context that starved, recurrence calls left on the step kernels before re-arming)."""
    out = (C.c_int * 2)()
    _lib.check(_lib.load().ds2_rnn_persistent_counters(_ctxp(device), C.cast(out, C.c_void_p)), "ds2_rnn_persistent_counters")
    return int(out[0]), int(out[1])


def rnn_fwd(gates: int, gx: Tensor, wp_fwd: Tensor, bhh: Tensor, lens_dev: Tensor, T: int, B: int, H: int, bf16=False,
            packed_gates: bool = False, h_bf16: Optional[Tensor] = None, hsum: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """gx (T*B, 2*G*H) in/out; returns (hbuf (T*B, 2H), aux (T*B, 2H)[, gates_bf (T*B, 2H, 4) bf16]).
    gates = 1 (tanh cell): gx stays the x-projections and h is the whole saved state — aux and gates_bf are returned as None.
    bf16: False / 0 fp32, True / 1 bf16 operands, 2 = fp32 mode with the split persistent kernel (h and W_hh as hi + lo bf16 planes, three MFMAs
    per product: fp32-grade results at the bf16 matrix rate; wp_fwd from rnn_pack(bf16=2); rnn_last_path() & 32 when it took the call).
    packed_gates: the saved-for-backward gates go to one 8-byte bf16 record per hidden unit (gx keeps the x-projections; GRU aux
    is not written) — pass the returned buffer to rnn_bwd.
    h_bf16: optional (T*B, 2H) bf16 buffer that receives a bf16 copy of hbuf — by a persistent launch only (rnn_last_path() & 1).
    hsum: optional (2, ceil(B/16), H) fp32 buffer that receives, per direction and 16-row batch tile, the sums of h over time — by a persistent
    launch only (rnn_last_path() & 1); bf16 training mode (bf16 = 1, packed_gates)."""
    _chk_f32(bhh, hsum)
    assert gx.is_contiguous() and bhh.is_contiguous()
    if h_bf16 is not None:
        assert h_bf16.dtype == torch.bfloat16 and h_bf16.is_contiguous() and h_bf16.numel() == T * B * 2 * H
    lib = _lib.load()
    hbuf = torch.empty(T * B, 2 * H, dtype=torch.float32, device=gx.device)
    aux = torch.empty_like(hbuf) if gates != 1 else None
    rec = torch.empty(T * B, 2 * H, 4, dtype=torch.bfloat16, device=gx.device) if (packed_gates and gates != 1) else None
    wsb = lib.ds2_rnn_fwd_workspace_bytes(B, H, int(bf16))
    ws, armed = _take_ws(ws, wsb, gx.device)
    if gx.dtype == torch.bfloat16 or hsum is not None:
        # the bf16 training mode's entry point: bf16 x-projections (gemm_bf16_nt_obf16) and / or the per-tile column sums of h.  Persistent
        # launches take bf16 x-projections as they are; anything else (a cooldown after a starved launch, a shape without a persistent
        # kernel) gets them widened and runs as before
        assert int(bf16) == 1 and packed_gates, "rnn_fwd: bf16 x-projections / hsum belong to the bf16 training mode with packed gate records"
        gxb = gx if gx.dtype == torch.bfloat16 else None
        gxf = None if gxb is not None else gx
        for _attempt in (0, 1):
            rc = lib.ds2_rnn_fwd_x(
                _ctxp(gx.device), gates, _ptr(gxf), _ptr(gxb), wp_fwd.data_ptr(), bhh.data_ptr(), hbuf.data_ptr(), _ptr(aux),
                lens_dev.data_ptr(), T, B, H, _ptr(rec), _ptr(h_bf16), _ptr(hsum), ws.data_ptr(), wsb, _stream(), int(armed and _attempt == 0))
            if rc != 1:
                break
            gxf, gxb = widen_bf16(gxb), None
        _lib.check(rc, "ds2_rnn_fwd_x")
        return hbuf, aux, rec
    _chk_f32(gx)
    _lib.check(lib.ds2_rnn_fwd_ex(
        _ctxp(gx.device), gates, gx.data_ptr(), wp_fwd.data_ptr(), bhh.data_ptr(), hbuf.data_ptr(), _ptr(aux),
        lens_dev.data_ptr(), T, B, H, int(bf16), _ptr(rec), _ptr(h_bf16), ws.data_ptr(), wsb, _stream(), int(armed)), "ds2_rnn_fwd")
    return (hbuf, aux, rec) if packed_gates else (hbuf, aux)


_CORESIDENT = {}


def wgrad_fits_beside_bwd_recurrence(gates: int, H: int) -> bool:
    """Does a workgroup of the co-resident weight-gradient kernel (gemm_bf16_tn_group: one wave of <= 128 registers per SIMD, 128 KB of LDS)
    fit on a CU that already holds a workgroup of the K-split backward recurrence of this shape (two waves per SIMD)?  Decided from the
    register count of the LOADED kernel (512 registers per SIMD lane, allocated in blocks of 8; 160 KB of LDS per CU)."""
    key = (gates, H)
    if key not in _CORESIDENT:
        out = (C.c_int * 3)()
        has = _lib.load().ds2_rnn_bwd_ksplit_footprint(gates, H, out)
        regs = (out[0] + 7) // 8 * 8
        _CORESIDENT[key] = bool(has == 1 and out[2] == 512 and 2 * regs + 128 <= 512 and out[1] + 128 * 1024 <= 160 * 1024)
    return _CORESIDENT[key]


def rnn_last_path(device=None) -> int:
    """The DS2_RNN_PATH_* bits of include/ds2hip.h.  1 / 2: the last rnn_fwd / rnn_bwd call ran as one persistent launch (and produced its
    optional outputs); 4: that backward launch was the K-split kernel (bf16 partial-dh exchange; results within a stated tolerance of the step
    kernels'); 16: it applied the BatchNorm1d backward on the fly (rnn_bwd_bn); 32 / 64: a split (fp32-mode) forward / backward kernel took
    the call; 256: the 10-unit-slice forward kernel."""
    return _lib.load().ds2_rnn_last_path(_ctxp(device))


def rnn_bwd(gates: int, dy: Tensor, gx: Optional[Tensor], aux: Optional[Tensor], hbuf: Tensor, wp_bwd: Tensor, lens_dev: Tensor, T: int, B: int, H: int,
            bf16: bool = False, dgx_bf16: Optional[Tensor] = None, gates_bf16: Optional[Tensor] = None, dhn_bf16: Optional[Tensor] = None,
            bias_part: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """dgx_bf16: optional (T*B, 2*G*H) bf16 buffer that receives dGx (then `gx` keeps the gates).
    gates_bf16: the packed records of rnn_fwd(packed_gates=True), read instead of gx / GRU aux (gx may then be None).
    dhn_bf16 (GRU, (T*B, 2H) bf16 copy of d(hn)) and bias_part ((B, 2, 4, H) fp32 per-batch-row sums over time of the gate gradients):
    optional outputs of a persistent launch only (rnn_last_path() & 2).
    gates = 1 (tanh cell): aux is None and no gate record exists (h comes from hbuf); gx may be None when dgx_bf16 is given."""
    _chk_f32(dy, gx, aux, hbuf, bias_part)
    if dgx_bf16 is not None:
        assert dgx_bf16.dtype == torch.bfloat16 and dgx_bf16.is_contiguous() and dgx_bf16.numel() == T * B * 2 * gates * H
    if gates_bf16 is not None:
        assert gates_bf16.dtype == torch.bfloat16 and gates_bf16.is_contiguous() and gates_bf16.numel() == T * B * 2 * H * 4
    if dhn_bf16 is not None:
        assert dhn_bf16.dtype == torch.bfloat16 and dhn_bf16.is_contiguous() and dhn_bf16.numel() == T * B * 2 * H
    if bias_part is not None:
        assert bias_part.is_contiguous() and bias_part.numel() == B * 2 * 4 * H
    assert gx is not None or (dgx_bf16 is not None and (gates_bf16 is not None or gates == 1))
    assert aux is not None or gates == 1
    lib = _lib.load()
    wsb = lib.ds2_rnn_bwd_workspace_bytes(gates, B, H, int(bf16))
    ws, armed = _take_ws(ws, wsb, dy.device)
    _lib.check(lib.ds2_rnn_bwd_ex(
        _ctxp(dy.device), gates, dy.data_ptr(), _row_pitch(dy), _ptr(gx), _ptr(aux), hbuf.data_ptr(), wp_bwd.data_ptr(),
        lens_dev.data_ptr(), T, B, H, int(bf16), _ptr(dgx_bf16), _ptr(gates_bf16), _ptr(dhn_bf16), _ptr(bias_part),
        ws.data_ptr(), wsb, _stream(), int(armed)), "ds2_rnn_bwd")


def bn1d_bwd_sums(dY: Tensor, X: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """Column sums of BatchNorm1d backward only: (sum dY, sum dY * xhat) = (dbeta, dgamma), two (H,) fp32 vectors — written into `out` when
    given (e.g. the gradient buffers themselves).  The elementwise half is left to rnn_bwd_bn."""
    _chk_f32(dY, X, mean, var, gamma)
    lib = _lib.load()
    M, H = X.shape
    if out is None:
        both = torch.empty(2, H, dtype=torch.float32, device=X.device)
        out = (both[0], both[1])
    s0, s1 = out
    _chk_f32(s0, s1)
    assert s0.is_contiguous() and s1.is_contiguous() and s0.numel() == H == s1.numel()
    wsb = lib.ds2_colreduce_workspace_bytes(M, H)
    ws = _ws(wsb, X.device)
    _lib.check(lib.ds2_bn1d_bwd_f32(dY.data_ptr(), _row_pitch(dY), X.data_ptr(), _row_pitch(X), None, 0, M, H, mean.data_ptr(), var.data_ptr(),
                                    gamma.data_ptr(), BN_EPS, s1.data_ptr(), s0.data_ptr(), ws.data_ptr(), wsb, _stream()), "ds2_bn1d_bwd_f32")
    return s0, s1


def rnn_bwd_bn(gates: int, dyn: Tensor, bn_x: Tensor, mean: Tensor, var: Tensor, gamma: Tensor, sums: Tensor, gx: Optional[Tensor], aux: Optional[Tensor],
               hbuf: Tensor, wp_bwd: Tensor, lens_dev: Tensor, T: int, B: int, H: int, bf16: bool = False, dgx_bf16: Optional[Tensor] = None,
               gates_bf16: Optional[Tensor] = None, dhn_bf16: Optional[Tensor] = None, bias_part: Optional[Tensor] = None, ws: Optional[Tensor] = None):
    """rnn_bwd for a layer whose output feeds a BatchNorm1d: `dyn` is the gradient wrt the BatchNorm's OUTPUT, `bn_x` its input, `sums` the
    (s0, s1) result of bn1d_bwd_sums.  The K-split kernel applies the elementwise BatchNorm backward on the fly (rnn_last_path() & 16);
    any other kernel family gets it materialised first."""
    s0, s1 = sums
    xbf = bn_x.dtype == torch.bfloat16                  # the centred bf16 operand of center_colstats (mean = its delta): ds2_rnn_bwd_bn_xbf16
    _chk_f32(dyn, None if xbf else bn_x, mean, var, gamma, s0, s1, gx, aux, hbuf, bias_part)
    assert s0.is_contiguous() and s1.is_contiguous() and s0.numel() == H == s1.numel() and bn_x.shape[0] == T * B and bn_x.shape[1] >= H and dyn.shape == (T * B, H)
    assert bn_x.stride(1) == 1 and (not xbf or bn_x.shape[1] == H or bn_x.stride(0) % 2 == 0)
    lib = _lib.load()
    wsb = lib.ds2_rnn_bwd_workspace_bytes(gates, B, H, int(bf16))
    ws, armed = _take_ws(ws, wsb, dyn.device)
    entry = lib.ds2_rnn_bwd_bn_xbf16 if xbf else lib.ds2_rnn_bwd_bn

    def call(scratch):
        return entry(_ctxp(dyn.device), gates, dyn.data_ptr(), _row_pitch(dyn), bn_x.data_ptr(), bn_x.stride(0), mean.data_ptr(), var.data_ptr(),
                     gamma.data_ptr(), s0.data_ptr(), s1.data_ptr(), BN_EPS, _ptr(scratch), _ptr(gx), _ptr(aux),
                     hbuf.data_ptr(), wp_bwd.data_ptr(), lens_dev.data_ptr(), T, B, H, int(bf16), _ptr(dgx_bf16), _ptr(gates_bf16),
                     _ptr(dhn_bf16), _ptr(bias_part), ws.data_ptr(), wsb, _stream(), int(armed and scratch is None))
    rc = call(None)                  # the fused K-split launch needs no scratch: the (T*B, H) fp32 buffer is allocated only on the fallback (rc 1)
    if rc == 1:
        rc = call(torch.empty(T * B, H, dtype=torch.float32, device=dyn.device))
    _lib.check(rc, "ds2_rnn_bwd_bn")


def rnn_bias_grads(gates: int, bias_part: Tensor, dbih: Tensor, dbhh: Tensor):
    """bias_part (B, 2, 4, H) of rnn_bwd -> dbih (2*G*H,) / dbhh (2, G*H) gradient buffers (contiguous)."""
    _chk_f32(bias_part, dbih, dbhh)
    B, _, _, H = bias_part.shape
    assert bias_part.is_contiguous() and dbih.is_contiguous() and dbhh.is_contiguous() and dbih.numel() == 2 * gates * H == dbhh.numel()
    _lib.check(_lib.load().ds2_rnn_bias_grads(gates, bias_part.data_ptr(), B, H, dbih.data_ptr(), dbhh.data_ptr(), _stream()), "ds2_rnn_bias_grads")


# ------------------------------------------------------------------------------------------------
# CTC
# ------------------------------------------------------------------------------------------------
def _ctc_loss(entry, logits, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_tgt, grad_scale, want_grad, lattice, return_ab, star=()):
    """ctc_loss and ctc_star_loss: `entry` is the C entry, star = (star_penalty, flags pointer) the two arguments only the wildcard one takes"""
    _chk_f32(logits)
    lib = _lib.load()
    T, B, Cc = logits.shape
    assert logits.stride(2) == 1 and logits.stride(0) == B * logits.stride(1)
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    grad = torch.empty(T, B, Cc, dtype=torch.float32, device=logits.device) if want_grad else None
    wsb = (lib.ds2_ctc_star_workspace_bytes if star else lib.ds2_ctc_workspace_bytes)(T, B, max_tgt)
    ws = _ws(wsb, logits.device)
    if return_ab:
        ws.zero_()
    _lib.check(getattr(lib, entry)(logits.data_ptr(), logits.stride(1), T, B, Cc, targets_dev.data_ptr(), tgt_off_dev.data_ptr(),
                                   in_lens_dev.data_ptr(), tgt_lens_dev.data_ptr(), int(max_tgt), *star, nll.data_ptr(), _ptr(grad), Cc,
                                   float(grad_scale), int(lattice), ws.data_ptr(), wsb, _stream()), entry)
    if return_ab:                                        # the lattices follow the (T, B) row of the workspace, as the C entries lay it out
        Smax = 2 * int(max_tgt) + 1
        off = (T * B * 4 + 255) // 256 * 256
        return nll, grad, ws[off:off + 2 * B * T * Smax * 4].view(torch.float32).view(2, B, T, Smax).clone()
    return nll, grad


def ctc_loss(logits: Tensor, targets_dev: Tensor, tgt_off_dev: Tensor, in_lens_dev: Tensor, tgt_lens_dev: Tensor, max_tgt: int,
             grad_scale: float, want_grad: bool = True, lattice: int = 0, return_ab: bool = False):
    """logits (T,B,C) (last dim contiguous, uniform row pitch).  Returns (nll (B,), grad (T,B,C) or None).
    lattice: 0 = the library chooses the lattice kernel, 1 = one workgroup per lattice whatever the target length (the two write the same
    bits).  return_ab: also a copy of the alpha / beta lattices (2, B, T, 2 * max_tgt + 1), zero outside an utterance's (T_b, S_b)."""
    return _ctc_loss("ds2_ctc_loss_ex_f32", logits, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_tgt, grad_scale, want_grad, lattice,
                     return_ab)


def ctc_star_loss(logits: Tensor, targets_dev: Tensor, tgt_off_dev: Tensor, in_lens_dev: Tensor, tgt_lens_dev: Tensor, max_tgt: int,
                  grad_scale: float, star_penalty: float = math.log(0.5), flags: Optional[Tensor] = None, want_grad: bool = True,
                  lattice: int = 0, return_ab: bool = False):
    """ctc_loss for imperfect transcripts (contract: include/ds2hip.h, ds2_ctc_star_loss_f32): the label value C = logits.shape[2] is
    the wildcard, whose state emits the constant star_penalty (<= 0, finite, natural log); flags (B) int32 on the device, or None:
    bit 0 = the first token is optional, bit 1 = the last.  Everything else, and what is returned, as ctc_loss; without a wildcard
    and without flags the results are its bits."""
    if flags is not None:
        assert flags.dtype == torch.int32 and flags.numel() == logits.shape[1] and flags.is_contiguous() and flags.device == logits.device
    return _ctc_loss("ds2_ctc_star_loss_f32", logits, targets_dev, tgt_off_dev, in_lens_dev, tgt_lens_dev, max_tgt, grad_scale, want_grad,
                     lattice, return_ab, star=(float(star_penalty), _ptr(flags)))


def ctc_mwer(logits: Tensor, hyps_dev: Tensor, hyp_off_dev: Tensor, hyp_lens_dev: Tensor, hyp_valid_dev: Optional[Tensor], in_lens_dev: Tensor,
             max_hyp_len: int, risk_dev: Tensor, grad_scale: float = 1.0, want_grad: bool = True, grad: Optional[Tensor] = None,
             lattice: int = 0):
    """Minimum-error-rate loss on an n-best list (contract: include/ds2hip.h, ds2_ctc_mwer_f32).  logits (T,B,C) as ctc_loss takes
    them; hyps_dev flat int32 labels, hyp_off_dev (B,K) int64 offsets into it, hyp_lens_dev (B,K) int32, hyp_valid_dev (B,K) int32 or
    None = all valid, risk_dev (B,K) fp32, all on the GPU; max_hyp_len bounds every hypothesis and sizes the workspace (8 B K T
    (2 max_hyp_len + 1) bytes).  Returns (loss (B), nll_hyp (B,K), post (B,K), grad (T,B,C) or None).  With `grad` given (fp32,
    contiguous, (T,B,C)) the gradient is ADDED to it (accumulate = 1) and it is the tensor returned; otherwise want_grad decides."""
    _chk_f32(logits, risk_dev, grad)
    lib = _lib.load()
    T, B, Cc = logits.shape
    dev = logits.device
    assert logits.stride(2) == 1 and logits.stride(0) == B * logits.stride(1)
    if hyp_off_dev.dim() != 2 or hyp_off_dev.shape[0] != B:
        raise ValueError(f"ctc_mwer: hyp_off_dev must be (B, K) with B = {B}, got {tuple(hyp_off_dev.shape)}")
    K = hyp_off_dev.shape[1]
    for name, t, dt in (("hyps_dev", hyps_dev, torch.int32), ("hyp_off_dev", hyp_off_dev, torch.int64), ("hyp_lens_dev", hyp_lens_dev, torch.int32),
                        ("hyp_valid_dev", hyp_valid_dev, torch.int32), ("in_lens_dev", in_lens_dev, torch.int32), ("risk_dev", risk_dev, torch.float32)):
        if t is not None and (t.dtype != dt or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"ctc_mwer: {name} must be a contiguous {dt} tensor on {dev}")
    if any(t is not None and t.numel() != B * K for t in (hyp_lens_dev, hyp_valid_dev, risk_dev)) or in_lens_dev.numel() != B:
        raise ValueError(f"ctc_mwer: lengths / validity / risks do not match (B, K) = ({B}, {K})")
    if grad is not None and (grad.shape != (T, B, Cc) or not grad.is_contiguous() or grad.device != dev):
        raise ValueError("ctc_mwer: grad must be a contiguous (T, B, C) tensor on the logits' device")
    accumulate = grad is not None
    if grad is None and want_grad:
        grad = torch.empty(T, B, Cc, dtype=torch.float32, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    nll_hyp = torch.empty(B, K, dtype=torch.float32, device=dev)
    post = torch.empty(B, K, dtype=torch.float32, device=dev)
    wsb = lib.ds2_ctc_mwer_workspace_bytes(T, B, K, int(max_hyp_len))
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_ctc_mwer_f32(logits.data_ptr(), logits.stride(1), T, B, Cc, K, hyps_dev.data_ptr(), hyp_off_dev.data_ptr(),
                                    hyp_lens_dev.data_ptr(), _ptr(hyp_valid_dev), in_lens_dev.data_ptr(), int(max_hyp_len), risk_dev.data_ptr(),
                                    loss.data_ptr(), nll_hyp.data_ptr(), post.data_ptr(), _ptr(grad), Cc, float(grad_scale), int(accumulate),
                                    int(lattice), ws.data_ptr(), wsb, _stream()), "ds2_ctc_mwer_f32")
    return loss, nll_hyp, post, grad


def ctc_confidence(logits: Tensor, hyps_dev: Tensor, hyp_off_dev: Tensor, hyp_lens_dev: Tensor, in_lens_dev: Tensor, max_hyp_len: int,
                   n_units: Tensor, unit_lo: Tensor, unit_hi: Tensor, win_start: Tensor, win_end: Tensor, lattice: int = 0):
    """Word and character confidences (contract: include/ds2hip.h, ds2_ctc_conf_f32).  logits (T,B,C) as ctc_loss takes them; one
    hypothesis per utterance as ctc_mwer's slots with K = 1: hyps_dev flat int32 labels, hyp_off_dev (B) int64 offsets into it,
    hyp_lens_dev (B) int32; n_units (B) int32 and unit_lo / unit_hi / win_start / win_end (B, W_max) int32: unit w of utterance b covers
    the labels [lo, hi) (at most 63) and the frames [start, end); all on the GPU.  max_hyp_len bounds every hypothesis and sizes the
    workspace (8 B T (2 max_hyp_len + 1) bytes).  Returns (nll (B), logconf (B, W_max)): log of the probability that the utterance
    spells its hypothesis given that the frames outside the unit's window spell the rest; NaN for a slot beyond n_units, a unit out of
    bounds or an impossible context, -inf where the unit cannot be spelled in its window."""
    _chk_f32(logits)
    lib = _lib.load()
    if logits.dim() != 3:
        raise ValueError(f"ctc_confidence: logits must be (T, B, C), got {tuple(logits.shape)}")
    T, B, Cc = logits.shape
    dev = logits.device
    ld = logits.stride(1) if B > 1 else logits.stride(0)     # (the stride of a dimension of one entry says nothing)
    if logits.stride(2) != 1 or logits.stride(0) != B * ld or ld < Cc:
        raise ValueError("ctc_confidence: logits must be (T, B, C) with contiguous classes and a uniform row pitch")
    if unit_lo.dim() != 2 or unit_lo.shape[0] != B or unit_lo.shape[1] < 1:
        raise ValueError(f"ctc_confidence: unit_lo must be (B, W_max) with B = {B} and W_max >= 1, got {tuple(unit_lo.shape)}")
    W = unit_lo.shape[1]
    _chk_on_dev("ctc_confidence", dev, torch.int32, dict(hyps_dev=hyps_dev, hyp_lens_dev=hyp_lens_dev, in_lens_dev=in_lens_dev, n_units=n_units,
                                                        unit_lo=unit_lo, unit_hi=unit_hi, win_start=win_start, win_end=win_end))
    _chk_on_dev("ctc_confidence", dev, torch.int64, dict(hyp_off_dev=hyp_off_dev))
    if any(t.numel() != B for t in (hyp_off_dev, hyp_lens_dev, in_lens_dev, n_units)):
        raise ValueError(f"ctc_confidence: offsets / lengths / unit counts do not match B = {B}")
    if any(tuple(t.shape) != (B, W) for t in (unit_hi, win_start, win_end)):
        raise ValueError(f"ctc_confidence: the unit arrays do not match (B, W_max) = ({B}, {W})")
    if not _is_int(max_hyp_len, 0):
        raise ValueError(f"ctc_confidence: max_hyp_len must be an integer >= 0, got {max_hyp_len!r}")
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    logconf = torch.empty(B, W, dtype=torch.float32, device=dev)
    wsb = lib.ds2_ctc_conf_workspace_bytes(T, B, int(max_hyp_len))
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_ctc_conf_f32(logits.data_ptr(), ld, T, B, Cc, hyps_dev.data_ptr(), hyp_off_dev.data_ptr(),
                                    hyp_lens_dev.data_ptr(), in_lens_dev.data_ptr(), int(max_hyp_len), n_units.data_ptr(), unit_lo.data_ptr(),
                                    unit_hi.data_ptr(), win_start.data_ptr(), win_end.data_ptr(), W, nll.data_ptr(), logconf.data_ptr(),
                                    int(lattice), ws.data_ptr(), wsb, _stream()), "ds2_ctc_conf_f32")
    return nll, logconf


def ctc_batch_mean(nll: Tensor) -> Tensor:
    """(1,) fp32 = nll.sum() / B, on the device in a fixed order (trainers/deepspeech_trainer.py:110-112)."""
    _chk_f32(nll)
    assert nll.dim() == 1 and nll.is_contiguous()
    out = torch.empty(1, dtype=torch.float32, device=nll.device)
    _lib.check(_lib.load().ds2_ctc_batch_mean_f32(nll.data_ptr(), nll.numel(), out.data_ptr(), _stream()), "ds2_ctc_batch_mean_f32")
    return out


def add_i64(x: Tensor, v: int = 1):
    """x += v for a small contiguous int64 vector (the BatchNorm num_batches_tracked counters)."""
    assert x.dtype == torch.int64 and x.is_contiguous() and x.is_cuda
    _lib.check(_lib.load().ds2_add_i64(x.data_ptr(), x.numel(), int(v), _stream()), "ds2_add_i64")


def softmax_rows(x: Tensor) -> Tensor:
    """softmax over the last dim of a (rows, C) row-major view."""
    _chk_f32(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ds2_softmax_rows_f32(x.data_ptr(), _row_pitch(x), y.data_ptr(), x.size(1), x.size(0), x.size(1), _stream()),
               "ds2_softmax_rows_f32")
    return y


def _sizes_i32(sizes, B: int, dev):
    """the decoders' optional per-utterance frame counts (any integer dtype, any device) as (B) int32 on dev, or None"""
    if sizes is None:
        return None
    if sizes.numel() != B:
        raise ValueError(f"sizes has {sizes.numel()} entries for a batch of {B}")
    return sizes.to(device=dev, dtype=torch.int32).contiguous().view(-1)


def _posteriors(who, x, name="probs", off_gpu=ValueError, what="(B,T,C)", empty=None):
    """The host path of every consumer of posteriors: x is (B,T,C) fp32 on the GPU with contiguous classes -> (B, T, C, device, ld_b,
    ld_t), the strides as the C entries take them (a dimension of one entry may carry the stride 0, which they refuse: it becomes 1).
    off_gpu: how a tensor off the GPU is refused.  ValueError: by name, like a non-tensor, before the shape; DS2LibraryError: with
    _chk_f32's text; None: not here, the caller does it after its other checks (_chk_align_args).  what: the shape as the refusal
    spells it.  empty: the refusal of an empty dimension ({shape}: x's), None = left to the C entry."""
    if off_gpu is ValueError:
        if not torch.is_tensor(x):
            raise ValueError(f"{who}: {name} must be a tensor")
        if not x.is_cuda:
            raise ValueError(f"{who}: {name} must be a GPU tensor (no CPU fallback exists)")
    if x.dim() != 3 or x.stride(2) != 1:
        raise ValueError(f"{who}: {name} must be {what} with a contiguous class dim")
    B, T, Cc = x.shape
    if empty is not None and min(B, T, Cc) < 1:
        raise ValueError(f"{who}: " + empty.format(shape=(B, T, Cc)))
    if off_gpu is not None:
        _chk_f32(x)
    ld_b, ld_t = x.stride(0), x.stride(1)
    if B <= 1 or T <= 1:                                 # (the common case costs nothing: these wrappers front kernels of 20 us)
        ld_b, ld_t = ld_b if B > 1 else max(ld_b, 1), ld_t if T > 1 else max(ld_t, 1)
    return B, T, Cc, x.device, ld_b, ld_t


def _chk_on_dev(who, dev, dtype, tensors):
    """tensors: name -> tensor or None; each one given must be contiguous, of `dtype` and on `dev`"""
    for name, t in tensors.items():
        if t is not None and (t.dtype != dtype or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous {str(dtype).replace('torch.', '')} tensor on {dev}")


def _is_int(v, lo, hi=None) -> bool:
    """v is an integer (an int, or a float or array scalar that equals one; not a bool) in [lo, hi]"""
    return not (isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi))


def greedy_decode(probs: Tensor, sizes: Tensor | None = None, blank: int = 0):
    """probs (B,T,C) fp32 on the GPU -> (ids (B,T) i32, offsets (B,T) i32, lengths (B) i32), all on the GPU."""
    B, T, C, dev, ld_b, ld_t = _posteriors("greedy_decode", probs, off_gpu=_lib.DS2LibraryError)
    sizes = _sizes_i32(sizes, B, dev)
    ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    offs = torch.empty((B, T), dtype=torch.int32, device=dev)
    lens = torch.empty((B,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    n = lib.ds2_greedy_decode_workspace_bytes(B, T)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.check(lib.ds2_greedy_decode_f32(probs.data_ptr(), ld_b, ld_t, B, T, C,
                                         _ptr(sizes), blank, ids.data_ptr(), offs.data_ptr(),
                                         lens.data_ptr(), ws.data_ptr(), n, _stream()), "ds2_greedy_decode_f32")
    return ids, offs, lens


def _edit_problems(who, seq, a_off, a_len, b_off, b_len, max_len):
    """The host path of edit_distance and edit_align: seq flat int32 on the GPU, offsets (int64) and lengths (int32) on the host or the
    GPU, host ones checked against seq -> (seq, device, a_off, a_len, b_off, b_len on the device, P, max_len).  With P == 0 the four
    arrays come back as they are: nothing is launched."""
    if not torch.is_tensor(seq) or not seq.is_cuda:
        raise _lib.DS2LibraryError(f"{who}: seq must be a GPU tensor (no CPU fallback exists)")
    if seq.dtype != torch.int32:
        raise TypeError(f"{who}: expected int32 symbols, got {seq.dtype}")
    seq = seq.contiguous().view(-1)
    dev = seq.device
    a_off, a_len, b_off, b_len = (torch.as_tensor(t).reshape(-1) for t in (a_off, a_len, b_off, b_len))
    P = a_len.numel()
    if not a_off.numel() == b_off.numel() == b_len.numel() == P:
        raise ValueError(f"{who}: {a_off.numel()} / {P} / {b_off.numel()} / {b_len.numel()} offsets and lengths")
    host = not any(t.is_cuda for t in (a_off, a_len, b_off, b_len))
    if host and P:
        lo = torch.stack((a_off.long(), b_off.long())).min()
        ln = torch.stack((a_len.long(), b_len.long()))
        hi = (torch.stack((a_off.long(), b_off.long())) + ln).max()
        if int(lo) < 0 or int(ln.min()) < 0 or int(hi) > seq.numel():
            raise ValueError(f"{who}: a pair lies outside the symbol buffer")
    if max_len is None:
        max_len = 0 if P == 0 else int(torch.maximum(a_len.max(), b_len.max()))
    if P:
        a_off, b_off = (t.to(device=dev, dtype=torch.int64).contiguous() for t in (a_off, b_off))
        a_len, b_len = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (a_len, b_len))
    return seq, dev, a_off, a_len, b_off, b_len, P, int(max_len)


def edit_distance(seq: Tensor, a_off, a_len, b_off, b_len, max_len: int | None = None) -> Tensor:
    """Levenshtein distances (unit costs) of P pairs of int32 symbol sequences, one launch -> dist (P) int32 on the GPU (contract:
    include/ds2hip.h, ds2_edit_distance_i32).  seq: flat int32 symbols on the GPU; pair p compares seq[a_off[p]:][:a_len[p]] with
    seq[b_off[p]:][:b_len[p]].  Offsets (int64) and lengths (int32) may live on the host or the GPU.  max_len bounds every pair's
    longer side and sizes the workspace; when omitted it is taken from host lengths, or from device lengths at the cost of one
    synchronising reduction.  Host lengths and offsets are checked against seq here; a device-side pair outside seq gets -1."""
    seq, dev, a_off, a_len, b_off, b_len, P, max_len = _edit_problems("edit_distance", seq, a_off, a_len, b_off, b_len, max_len)
    dist = torch.empty((P,), dtype=torch.int32, device=dev)
    if P == 0:
        return dist
    lib = _lib.load()
    ws = _ws(lib.ds2_edit_distance_workspace_bytes(P, max_len), dev)
    _lib.check(lib.ds2_edit_distance_i32(seq.data_ptr(), seq.numel(), a_off.data_ptr(), a_len.data_ptr(), b_off.data_ptr(), b_len.data_ptr(),
                                         P, max_len, dist.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "ds2_edit_distance_i32")
    return dist


def edit_align(seq: Tensor, a_off, a_len, b_off, b_len, max_len: int | None = None):
    """Edit alignments (unit costs) of P pairs of int32 symbol sequences, one launch -> (counts (P,4), a_map (P,max_len), b_map
    (P,max_len)), int32 on the GPU (contract and tie rule: include/ds2hip.h, ds2_edit_align_i32).  Side a is the hypothesis, side b the
    reference; counts[p] = (hits, substitutions, deletions, insertions); a_map[p][i] is the index in b paired with a[i] or -1 (an
    insertion), b_map[p][j] the index in a paired with b[j] or -1 (a deletion); -1 beyond a side's length.  The arguments are
    edit_distance's, checked the same way; a device-side pair outside seq, or with a side above max_len, gets -1 everywhere.  The
    workspace grows with max_len squared (16 bytes per 64 DP cells and problem)."""
    seq, dev, a_off, a_len, b_off, b_len, P, max_len = _edit_problems("edit_align", seq, a_off, a_len, b_off, b_len, max_len)
    counts = torch.empty((P, 4), dtype=torch.int32, device=dev)
    a_map = torch.empty((P, max_len), dtype=torch.int32, device=dev)
    b_map = torch.empty((P, max_len), dtype=torch.int32, device=dev)
    if P == 0:
        return counts, a_map, b_map
    lib = _lib.load()
    ws = _ws(lib.ds2_edit_align_workspace_bytes(P, max_len), dev)
    _lib.check(lib.ds2_edit_align_i32(seq.data_ptr(), seq.numel(), a_off.data_ptr(), a_len.data_ptr(), b_off.data_ptr(), b_len.data_ptr(),
                                      P, max_len, counts.data_ptr(), a_map.data_ptr(), b_map.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "ds2_edit_align_i32")
    return counts, a_map, b_map


def _chk_align_args(who, x, ints, star_penalty=None, off_gpu=None):
    """The checks of the aligner wrappers, a malformed argument before a tensor off the GPU (off_gpu None; else as _posteriors takes it).
    ints: name -> int32 tensor or None, all of them but `targets` with one entry per utterance.  Returns _posteriors' six and
    star_penalty as a float (None without one)."""
    geo = _posteriors(who, x, "x", off_gpu)
    B, dev = geo[0], geo[3]
    _chk_on_dev(who, dev, torch.int32, ints)
    if any(t is not None and t.numel() != B for name, t in ints.items() if name != "targets"):
        raise ValueError(f"{who}: offsets / lengths{' / flags' if 'flags' in ints else ''} do not match the batch of {B}")
    p = None if star_penalty is None else float(star_penalty)
    if p is not None and not (p <= 0.0 and math.isfinite(p)):
        raise ValueError(f"{who}: star_penalty must be finite and <= 0, got {star_penalty}")
    if off_gpu is None:
        _chk_f32(x)
    return (*geo, p)


def _ctc_align(who, entry, x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log, shape, star=None):
    """The four aligner wrappers.  entry: the C entry, sized by its own *_workspace_bytes; shape: (variant,) or (tile_frames, tile_pairs),
    of which only a tile shape sizes the workspace (an illegal one sizes nothing: the entry refuses it); star: (star_penalty, flags)."""
    ints = dict(targets=targets, tgt_off=tgt_off, tgt_lens=tgt_lens, in_lens=in_lens)
    if star is not None:
        ints["flags"] = star[1]
    B, T, Cc, dev, ld_b, ld_t, p = _chk_align_args(who, x, ints, star[0] if star is not None else None)
    shape = tuple(int(v) for v in shape)
    n_tok = targets.numel()
    score = torch.empty(B, dtype=torch.float32, device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    tok_start = torch.empty(n_tok, dtype=torch.int32, device=dev)
    tok_end = torch.empty(n_tok, dtype=torch.int32, device=dev)
    tok_logp = torch.empty(n_tok, dtype=torch.float32, device=dev)
    tok = _ptr if n_tok else (lambda t: None)            # no token: null pointers, which the entries accept with max_u == 0 only
    lib = _lib.load()
    wsb = getattr(lib, entry[:-len("f32")] + "workspace_bytes")(B, T, int(max_u), *(shape if len(shape) == 2 else ()))
    ws = _ws(wsb, dev)
    _lib.check(getattr(lib, entry)(x.data_ptr(), ld_b, ld_t, B, T, Cc, 1 if is_log else 0, tok(targets), tgt_off.data_ptr(),
                                   _ptr(in_lens), tgt_lens.data_ptr(), int(max_u), *shape, *(() if star is None else (p, _ptr(star[1]))),
                                   score.data_ptr(), states.data_ptr(), tok(tok_start), tok(tok_end), tok(tok_logp), ws.data_ptr(), wsb,
                                   _stream()), entry)
    return score, states, tok_start, tok_end, tok_logp


def ctc_forced_align(x: Tensor, targets: Tensor, tgt_off: Tensor, in_lens: Tensor | None, tgt_lens: Tensor, max_u: int, is_log: bool,
                     variant: int = 0):
    """CTC forced alignment of x (B,T,C) fp32 on the GPU (any batch / frame strides, classes contiguous: the model's (T,B,C)-backed eval
    output needs no copy) against known targets -> (score (B) f32, states (B,T) i32, tok_start, tok_end (sum U) i32, tok_logp (sum U)
    f32), all on the GPU (contract: include/ds2hip.h, ds2_ctc_align_f32).  targets (flat), tgt_off, tgt_lens, in_lens (or None = T
    frames each) are int32 device tensors; max_u >= every target length (host-known: nothing is copied back to size anything).
    is_log: x holds log-probabilities (else probabilities).  variant: 0 = the library chooses, 1 = one wavefront per utterance
    (2 * max_u + 1 <= 128), 2 = one workgroup per utterance.  One launch on the current stream."""
    return _ctc_align("ctc_forced_align", "ds2_ctc_align_f32", x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log, (variant,))


def ctc_forced_align_tiled(x: Tensor, targets: Tensor, tgt_off: Tensor, in_lens: Tensor | None, tgt_lens: Tensor, max_u: int, is_log: bool,
                           tile_frames: int = 0, tile_pairs: int = 0):
    """ctc_forced_align for long recordings: the same tensors in, the same five results out and the same bits, with the lattice tiled
    over (frames x state pairs) and spread over the GPU, one launch per anti-diagonal of tiles (contract: include/ds2hip.h,
    ds2_ctc_align_tiled_f32).  No limit on T or max_u beyond the workspace (back-pointers: B * ceil(T/8) * (max_u+1) dwords).
    tile_frames / tile_pairs: 0 = the library's default, else a positive multiple of 8 / of 64 up to 1024 (DS2LibraryError otherwise)."""
    return _ctc_align("ctc_forced_align_tiled", "ds2_ctc_align_tiled_f32", x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log,
                      (tile_frames, tile_pairs))


def ctc_star_row(x: Tensor, in_lens: Tensor | None, is_log: bool, star_penalty: float):
    """The wildcard's emission of ctc_forced_align_star alone: g (B,T) f32 with g[b,t] = max_c e[b,t,c] + star_penalty for t < T_b and
    -inf beyond (the library leaves those frames unwritten).  One launch that reads x once (ds2_ctc_align_star_row_f32)."""
    B, T, Cc, dev, ld_b, ld_t, p = _chk_align_args("ctc_star_row", x, dict(in_lens=in_lens), star_penalty)
    g = torch.full((B, T), float("-inf"), dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.ds2_ctc_align_star_row_f32(x.data_ptr(), ld_b, ld_t, B, T, Cc, 1 if is_log else 0, _ptr(in_lens), p,
                                              g.data_ptr(), _stream()), "ds2_ctc_align_star_row_f32")
    return g


def ctc_forced_align_star(x: Tensor, targets: Tensor, tgt_off: Tensor, in_lens: Tensor | None, tgt_lens: Tensor, max_u: int, is_log: bool,
                          variant: int = 0, star_penalty: float = math.log(0.5), flags: Tensor | None = None):
    """ctc_forced_align for imperfect transcripts (contract: include/ds2hip.h, ds2_ctc_align_star_f32): the label value C = x.shape[2]
    in `targets` is a wildcard that emits max_c e[t][c] + star_penalty (star_penalty <= 0, finite), and flags (B) int32 or None opens,
    per utterance, the start in the second token's states (bit 0) and the end in the last but one token's (bit 1).  The same five
    results; a skipped first / last token has the span (-1, -1) and tok_logp 0.  Two launches (the wildcard row, the lattice) on the
    current stream.  With flags None and no wildcard label: the bits of ctc_forced_align."""
    return _ctc_align("ctc_forced_align_star", "ds2_ctc_align_star_f32", x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log, (variant,),
                      star=(star_penalty, flags))


def ctc_forced_align_star_tiled(x: Tensor, targets: Tensor, tgt_off: Tensor, in_lens: Tensor | None, tgt_lens: Tensor, max_u: int,
                                is_log: bool, tile_frames: int = 0, tile_pairs: int = 0, star_penalty: float = math.log(0.5),
                                flags: Tensor | None = None):
    """ctc_forced_align_star for long recordings: the same tensors in, the same five results out and the same bits, on the tiled lattice
    of ctc_forced_align_tiled (contract: include/ds2hip.h, ds2_ctc_align_star_tiled_f32).  tile_frames / tile_pairs as there."""
    return _ctc_align("ctc_forced_align_star_tiled", "ds2_ctc_align_star_tiled_f32", x, targets, tgt_off, in_lens, tgt_lens, max_u, is_log,
                      (tile_frames, tile_pairs), star=(star_penalty, flags))


KWS_MAX_LEN, KWS_MAX_HITS = 63, 1024


def ctc_keyword_search(x: Tensor, kw_labels: Tensor, kw_off: Tensor, kw_lens: Tensor, max_kw_len: int, thr: Tensor,
                       in_lens: Tensor | None = None, is_log: bool = False, max_hits: int = 32):
    """Keyword search over CTC posteriors x (B,T,C) fp32 on the GPU (any batch / frame strides, classes contiguous), K keywords against
    every utterance (contract: include/ds2hip.h, ds2_ctc_kws_f32) -> (frame_score (B,K,T) f32, frame_start (B,K,T) i32, hit_start,
    hit_end (B,K,max_hits) i32, hit_score (B,K,max_hits) f32, n_hits (B,K) i32), all on the GPU.  kw_labels (flat), kw_off (K),
    kw_lens (K) are int32 device tensors, thr (K) fp32 on the device, in_lens (B) int32 or None (= T frames each); max_kw_len >= every
    keyword length, at most 63; max_hits in [1, 1024] (n_hits == max_hits + 1: more detections than slots).  No limit on T: the
    workspace is 4 B T (1 + K) bytes.  Three launches on the current stream, nothing is copied back."""
    who = "ctc_keyword_search"
    if not all(torch.is_tensor(t) for t in (x, kw_labels, kw_off, kw_lens, thr)):
        raise ValueError(f"{who}: x, kw_labels, kw_off, kw_lens and thr must be tensors")
    if not 0 <= int(max_kw_len) <= KWS_MAX_LEN:
        raise ValueError(f"{who}: max_kw_len must lie in [0, {KWS_MAX_LEN}] (one wavefront holds a keyword), got {max_kw_len}")
    if not 1 <= int(max_hits) <= KWS_MAX_HITS:
        raise ValueError(f"{who}: max_hits must lie in [1, {KWS_MAX_HITS}], got {max_hits}")
    B, T, Cc, dev, ld_b, ld_t, _ = _chk_align_args(who, x, dict(in_lens=in_lens), off_gpu=ValueError)
    K = kw_lens.numel()
    if K < 1 or kw_off.numel() != K or thr.numel() != K:
        raise ValueError(f"{who}: {kw_off.numel()} offsets / {K} lengths / {thr.numel()} thresholds (one each per keyword, at least one)")
    _chk_on_dev(who, dev, torch.int32, dict(kw_labels=kw_labels, kw_off=kw_off, kw_lens=kw_lens))
    _chk_on_dev(who, dev, torch.float32, dict(thr=thr))
    max_hits = int(max_hits)
    fscore = torch.empty((B, K, T), dtype=torch.float32, device=dev)
    fstart = torch.empty((B, K, T), dtype=torch.int32, device=dev)
    hstart = torch.empty((B, K, max_hits), dtype=torch.int32, device=dev)
    hend = torch.empty((B, K, max_hits), dtype=torch.int32, device=dev)
    hscore = torch.empty((B, K, max_hits), dtype=torch.float32, device=dev)
    nhits = torch.empty((B, K), dtype=torch.int32, device=dev)
    lib = _lib.load()
    wsb = lib.ds2_ctc_kws_workspace_bytes(B, T, K, max_hits)
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_ctc_kws_f32(x.data_ptr(), ld_b, ld_t, B, T, Cc, 1 if is_log else 0, _ptr(in_lens),
                                   _ptr(kw_labels) if kw_labels.numel() else None, kw_off.data_ptr(), kw_lens.data_ptr(), K, int(max_kw_len),
                                   thr.data_ptr(), max_hits, fscore.data_ptr(), fstart.data_ptr(), hstart.data_ptr(), hend.data_ptr(),
                                   hscore.data_ptr(), nhits.data_ptr(), ws.data_ptr(), wsb, _stream()), "ds2_ctc_kws_f32")
    return fscore, fstart, hstart, hend, hscore, nhits


KWS_MAX_PENDING = 65536


def ctc_kws_stream_state(B: int, K: int, pending: int, dev) -> Tensor:
    """The state of B freshly opened keyword streams of K keywords for ctc_kws_stream_feed: zero bytes on dev
    (ds2_ctc_kws_stream_state_bytes: 4 * (264 + 3 * pending) per utterance and keyword)."""
    if not (_is_int(B, 1) and _is_int(K, 1) and _is_int(pending, 1, KWS_MAX_PENDING)):
        raise ValueError(f"ctc_kws_stream_state: B and K must be positive integers and pending one in [1, {KWS_MAX_PENDING}], "
                         f"got {B!r}, {K!r}, {pending!r}")
    n = _lib.load().ds2_ctc_kws_stream_state_bytes(int(B), int(K), int(pending))
    if n == 0:
        raise ValueError(f"ctc_kws_stream_state: {B} utterances x {K} keywords outside the supported sizes")
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def ctc_kws_stream_feed(probs: Tensor | None, sizes: Tensor | None, state: Tensor, kw_labels: Tensor, kw_off: Tensor, kw_lens: Tensor,
                        max_kw_len: int, thr: Tensor, pending: int, frames_bound: int, is_log: bool = False, max_hits: int = 32,
                        max_lag: int | None = None, finish: bool = False, return_frames: bool = False, classes: int | None = None,
                        batch: int | None = None):
    """One chunk of frames into B running keyword searches (contract: include/ds2hip.h, ds2_ctc_kws_stream_feed_f32): probs (B,T,C) fp32
    on the GPU (any batch / frame strides, classes contiguous), or None for a call without frames (`classes` and `batch` then give C and
    B): a flush with finish=True, a second look at the tentative detections without.  sizes (B) the chunk's valid frames per utterance,
    any integer dtype and device, or None; state as ctc_kws_stream_state made it for (B, K, pending); the packed keywords and thr as
    ctc_keyword_search takes them.  The keywords, thr, pending and max_lag must not change within a stream.  frames_bound: an upper bound
    of the frames consumed so far.  max_lag: the most frames the tail may lie behind the frames consumed after a feed (None: no limit, and the stream's detections
    are exactly the one-call search's).  -> (hit_start, hit_end (B,K,max_hits) i32, hit_score (B,K,max_hits) f32, hit_final
    (B,K,max_hits) i32, n_hits, tail, frames, forced, dropped (B,K) i32, frame_score (B,K,T) f32 and frame_start (B,K,T) i32 or None,
    None without return_frames), all on the GPU, frames absolute.  Two launches for the lattice, one for the pick, on the current
    stream; nothing is copied back."""
    who = "ctc_kws_stream_feed"
    if not all(torch.is_tensor(t) for t in (state, kw_labels, kw_off, kw_lens, thr)):
        raise ValueError(f"{who}: state, kw_labels, kw_off, kw_lens and thr must be tensors")
    if not 0 <= int(max_kw_len) <= KWS_MAX_LEN:
        raise ValueError(f"{who}: max_kw_len must lie in [0, {KWS_MAX_LEN}] (one wavefront holds a keyword), got {max_kw_len}")
    if not _is_int(max_hits, 1, KWS_MAX_HITS):
        raise ValueError(f"{who}: max_hits must lie in [1, {KWS_MAX_HITS}], got {max_hits}")
    if not _is_int(pending, 1, KWS_MAX_PENDING):
        raise ValueError(f"{who}: pending must lie in [1, {KWS_MAX_PENDING}], got {pending}")
    if max_lag is not None and not _is_int(max_lag, 0, 0x7fffffff):
        raise ValueError(f"{who}: max_lag must be None or an integer >= 0, got {max_lag!r}")
    dev = state.device
    if probs is None:
        if classes is None or batch is None:
            raise ValueError(f"{who}: a call without probs needs the number of classes and the batch")
        B, T, Cc, ld_b, ld_t = int(batch), 0, int(classes), 1, 1
    else:
        B, T, Cc, pdev, ld_b, ld_t = _posteriors(who, probs)
        if pdev != dev:
            raise ValueError(f"{who}: probs on {pdev}, the state on {dev}")
    K = kw_lens.numel()
    if K < 1 or kw_off.numel() != K or thr.numel() != K:
        raise ValueError(f"{who}: {kw_off.numel()} offsets / {K} lengths / {thr.numel()} thresholds (one each per keyword, at least one)")
    _chk_on_dev(who, dev, torch.uint8, dict(state=state))
    _chk_on_dev(who, dev, torch.int32, dict(kw_labels=kw_labels, kw_off=kw_off, kw_lens=kw_lens))
    _chk_on_dev(who, dev, torch.float32, dict(thr=thr))
    if int(frames_bound) < 0 or int(frames_bound) + T > 0x7fffffff:
        raise ValueError(f"{who}: {frames_bound} frames so far + {T} now pass 2^31 - 1")
    sizes = _sizes_i32(sizes, B, dev)
    max_hits = int(max_hits)
    hits = torch.empty((4, B, K, max_hits), dtype=torch.int32, device=dev)
    tail = torch.empty((5, B, K), dtype=torch.int32, device=dev)
    fscore = torch.empty((B, K, T), dtype=torch.float32, device=dev) if return_frames else None
    fstart = torch.empty((B, K, T), dtype=torch.int32, device=dev) if return_frames else None
    lib = _lib.load()
    wsb = lib.ds2_ctc_kws_stream_workspace_bytes(B, T, K, 1 if return_frames else 0)
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_ctc_kws_stream_feed_f32(_ptr(probs), ld_b, ld_t, B, T, Cc, 1 if is_log else 0, _ptr(sizes),
                                               _ptr(kw_labels) if kw_labels.numel() else None, kw_off.data_ptr(), kw_lens.data_ptr(), K,
                                               int(max_kw_len), thr.data_ptr(), max_hits, -1 if max_lag is None else int(max_lag),
                                               1 if finish else 0, int(pending), int(frames_bound), state.data_ptr(), state.numel(),
                                               _ptr(fscore), _ptr(fstart), hits[0].data_ptr(), hits[1].data_ptr(), hits[2].data_ptr(),
                                               hits[3].data_ptr(), tail[0].data_ptr(), tail[1].data_ptr(), tail[2].data_ptr(),
                                               tail[3].data_ptr(), tail[4].data_ptr(), ws.data_ptr(), wsb, _stream()),
               "ds2_ctc_kws_stream_feed_f32")
    return hits[0], hits[1], hits[2].view(torch.float32), hits[3], tail[0], tail[1], tail[2], tail[3], tail[4], fscore, fstart


def segment_max_segs(T: int, min_gap: int, max_len: int) -> int:
    """The most segments ctc_segment can give an utterance of T frames: at most (T + min_gap) // (min_gap + 1) regions (two regions are
    min_gap silent frames and a frame apart, an end's pause may be shorter) and at most T // ((max_len + 1) // 2) forced cuts (a piece
    that ends at one has that many frames)."""
    return max(1, (T + min_gap) // (min_gap + 1) + T // ((max_len + 1) // 2))


def ctc_segment(probs: Tensor, sizes: Tensor | None = None, blank: int = 0, threshold: float = 0.9, min_gap: int = 25, pad: int = 5,
                max_len: int = 1000, is_log: bool = False, max_segs: int | None = None):
    """Pause segmentation of CTC posteriors probs (B,T,C) fp32 on the GPU (any batch / frame strides, classes contiguous; contract:
    include/ds2hip.h, ds2_ctc_segment_f32) -> (seg_start, seg_end (B, max_segs) i32, seg_flags (B, max_segs) i32, n_segs (B) i32), all
    on the GPU.  A frame is silent when its blank probability is >= threshold (in (0, 1]; with is_log the input holds log-probabilities
    and log(threshold) is compared); silent runs of at least min_gap frames, and those at either end, are pauses; what lies between them,
    padded by up to `pad` frames into the pauses, is a segment; one longer than max_len is cut at its most silent frame in the second
    half of each max_len frames (flags: 1 = starts at such a cut, 2 = ends at one).  sizes (B) valid frames, any integer dtype and
    device, or None.  max_segs: None = segment_max_segs(T, min_gap, max_len), which no utterance exceeds; a smaller value keeps the
    first max_segs segments while n_segs still reports the full count.  Unused slots hold (-1, -1, 0).  Two launches on the current
    stream, nothing is copied back."""
    who = "ctc_segment"
    for name, v, lo in (("min_gap", min_gap, 1), ("pad", pad, 0), ("max_len", max_len, 2)):
        if not _is_int(v, lo, 0x7fffffff):
            raise ValueError(f"{who}: {name} must be an integer >= {lo}, got {v!r}")
    thr = float(threshold)
    if not (0.0 < thr <= 1.0):                           # (NaN fails too)
        raise ValueError(f"{who}: threshold must lie in (0, 1], got {threshold!r}")
    B, T, Cc, dev, ld_b, ld_t = _posteriors(who, probs, empty="empty probs {shape}")
    if not 0 <= int(blank) < Cc:
        raise ValueError(f"{who}: blank {blank} outside the {Cc} classes")
    sizes = _sizes_i32(sizes, B, dev)
    min_gap, pad, max_len = int(min_gap), int(pad), int(max_len)
    max_segs = segment_max_segs(T, min_gap, max_len) if max_segs is None else int(max_segs)
    if max_segs < 1:
        raise ValueError(f"{who}: max_segs must be positive, got {max_segs}")
    seg = torch.empty((3, B, max_segs), dtype=torch.int32, device=dev)
    n_segs = torch.empty((B,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    wsb = lib.ds2_ctc_segment_workspace_bytes(B, T)
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_ctc_segment_f32(probs.data_ptr(), ld_b, ld_t, B, T, Cc, _ptr(sizes), int(blank), math.log(thr) if is_log else thr,
                                       min_gap, pad, max_len, max_segs, seg[0].data_ptr(), seg[1].data_ptr(), seg[2].data_ptr(),
                                       n_segs.data_ptr(), ws.data_ptr(), wsb, _stream()), "ds2_ctc_segment_f32")
    return seg[0], seg[1], seg[2], n_segs


def ctc_segment_gather(probs: Tensor, seg_b: Tensor, seg_start: Tensor, seg_len: Tensor, t_max: int):
    """Packs S segments of probs (B,T,C) fp32 on the GPU (strides as ctc_segment takes them) into one padded batch, one launch (contract:
    include/ds2hip.h, ds2_ctc_segment_gather_f32) -> (out (S, t_max, C) fp32: row s = probs[seg_b[s], seg_start[s]:][:seg_len[s]], then
    zeros; out_sizes (S) i32 = seg_len).  seg_b, seg_start, seg_len: (S) int32 tensors on the GPU.  A segment outside probs or longer
    than t_max gives a zero row and the size 0."""
    who = "ctc_segment_gather"
    if not all(torch.is_tensor(t) for t in (probs, seg_b, seg_start, seg_len)):
        raise ValueError(f"{who}: probs, seg_b, seg_start and seg_len must be tensors")
    if not _is_int(t_max, 1, 0x7fffffff):
        raise ValueError(f"{who}: t_max must be a positive integer, got {t_max!r}")
    what = "a non-empty (B,T,C)"
    B, T, Cc, dev, ld_b, ld_t = _posteriors(who, probs, what=what, empty=f"probs must be {what} with a contiguous class dim")
    S = seg_b.numel()
    if seg_start.numel() != S or seg_len.numel() != S:
        raise ValueError(f"{who}: {S} / {seg_start.numel()} / {seg_len.numel()} utterances, starts and lengths")
    _chk_on_dev(who, dev, torch.int32, dict(seg_b=seg_b, seg_start=seg_start, seg_len=seg_len))
    out = torch.empty((S, int(t_max), Cc), dtype=torch.float32, device=dev)
    out_sizes = torch.empty((S,), dtype=torch.int32, device=dev)
    if S == 0:
        return out, out_sizes
    _lib.check(_lib.load().ds2_ctc_segment_gather_f32(probs.data_ptr(), ld_b, ld_t, B, T, Cc, seg_b.data_ptr(), seg_start.data_ptr(),
                                                      seg_len.data_ptr(), S, int(t_max), out.data_ptr(), out_sizes.data_ptr(), _stream()),
               "ds2_ctc_segment_gather_f32")
    return out, out_sizes


def _beam_search_args(who, lib, C, blank, beam_width, cutoff_top_n, lm, hotwords) -> int:
    """What ctc_beam_decode and ctc_beam_stream_feed check of the search's arguments before anything is allocated -> the beam width"""
    K = int(beam_width)
    if not 1 <= K <= lib.ds2_ctc_beam_max_width():
        raise ValueError(f"{who}: beam_width {K} outside the supported 1..{lib.ds2_ctc_beam_max_width()}")
    if hotwords is not None and hotwords.C != C:
        raise ValueError(f"{who}: the hotwords were bound to {hotwords.C} classes, probs have {C}")
    if hotwords is not None and hotwords.blank != int(blank):
        raise ValueError(f"{who}: the hotwords were bound to blank {hotwords.blank}, the decode has blank {int(blank)}")
    if lm is not None and lm.C != C:
        raise ValueError(f"{who}: the language model was bound to {lm.C} classes, probs have {C}")
    grid, cap = K * (min(int(cutoff_top_n), C - 1) + 2), lib.ds2_ctc_beam_lm_max_candidates()
    if (lm is not None or hotwords is not None) and grid > cap:          # (the plain search has its staircase: no full grid, no limit)
        why = "with a language model " if hotwords is None else \
            "with hotwords every beam is extended by every kept class, with or without a language model: "
        raise ValueError(f"{who}: {why}beam_width * (min(cutoff_top_n, C - 1) + 2) = {grid} exceeds the {cap} candidate slots")
    return K


def _beam_arm_args(lm, alpha, beta, hotwords, dev):
    """The language-model and hotword arguments of the beam entries: (lm_dev, lm_bytes, order, mode, space, alpha, beta), (hot_dev,
    hot_host, hot_bytes) and the device tensors that must outlive the call"""
    tab = lm.device_tables(dev) if lm is not None else None
    lm_args = (None, 0, 0, 0, -1) if lm is None else (tab.data_ptr(), tab.numel(), lm.order, lm.mode, lm.space if lm.space is not None else -1)
    lm_args += (float(alpha), float(beta))
    hot = hotwords.device_tables(dev) if hotwords is not None else None
    hot_args = (None, None, 0) if hotwords is None else (hot.data_ptr(), hotwords.packed.ctypes.data, hotwords.packed.nbytes)
    return lm_args, hot_args, (tab, hot)


def ctc_beam_decode(probs: Tensor, sizes: Tensor | None = None, blank: int = 0, beam_width: int = 100, cutoff_top_n: int = 40,
                    cutoff_prob: float = 1.0, lm=None, alpha: float = 0.0, beta: float = 0.0, hotwords=None, labels_out: Tensor | None = None):
    """CTC prefix beam search of probs (B,T,C) fp32 on the GPU -> (labels (B,K,T) i32, offsets (B,K,T) i32, lengths (B,K) i32,
    scores (B,K) fp32), all on the GPU, best beam first (contract: include/ds2hip.h).  With `lm` (a decoders.lm.NgramLM bound to these
    classes) the search fuses alpha * log10 LM scores + beta per scored token (ds2_ctc_beam_decode_lm_f32).  With `hotwords` (a
    decoders.hotwords.Hotwords bound to these classes) it also prefers prefixes that spell those phrases, with or without `lm`
    (ds2_ctc_beam_decode_hot_f32); the language model's candidate limit then applies without a language model too.
    labels_out: a contiguous (B,K,T) int32 GPU tensor to receive the labels instead of a fresh one (MWERLoss passes the front of the
    buffer that also holds the references, so that one edit-distance launch sees both)."""
    B, T, C, dev, ld_b, ld_t = _posteriors("ctc_beam_decode", probs, off_gpu=_lib.DS2LibraryError)
    lib = _lib.load()
    K = _beam_search_args("ctc_beam_decode", lib, C, blank, beam_width, cutoff_top_n, lm, hotwords)
    sizes = _sizes_i32(sizes, B, dev)
    if labels_out is not None and (labels_out.shape != (B, K, T) or labels_out.dtype != torch.int32 or labels_out.device != dev
                                   or not labels_out.is_contiguous()):
        raise ValueError(f"ctc_beam_decode: labels_out must be a contiguous ({B}, {K}, {T}) int32 tensor on {dev}")
    labels = labels_out if labels_out is not None else torch.empty((B, K, T), dtype=torch.int32, device=dev)
    offs = torch.empty((B, K, T), dtype=torch.int32, device=dev)
    lens = torch.empty((B, K), dtype=torch.int32, device=dev)
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    n = lib.ds2_ctc_beam_workspace_bytes(B, T, K)
    ws = _ws(n, dev)
    search = (probs.data_ptr(), ld_b, ld_t, B, T, C, _ptr(sizes), int(blank), K, int(cutoff_top_n), float(cutoff_prob))
    out = (labels.data_ptr(), offs.data_ptr(), lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), n, _stream())
    lm_args, hot_args, _keep = _beam_arm_args(lm, alpha, beta, hotwords, dev)
    if hotwords is not None:
        _lib.check(lib.ds2_ctc_beam_decode_hot_f32(*search, *lm_args, *hot_args, *out), "ds2_ctc_beam_decode_hot_f32")
    elif lm is not None:
        _lib.check(lib.ds2_ctc_beam_decode_lm_f32(*search, *lm_args, *out), "ds2_ctc_beam_decode_lm_f32")
    else:
        _lib.check(lib.ds2_ctc_beam_decode_f32(*search, *out), "ds2_ctc_beam_decode_f32")
    return labels, offs, lens, scores


def ctc_beam_stream_state(B: int, beam_width: int, lm, hotwords, dev) -> Tensor:
    """The state of B freshly opened streams for ctc_beam_stream_feed: zero bytes on dev (ds2_ctc_beam_stream_state_bytes)."""
    n = _lib.load().ds2_ctc_beam_stream_state_bytes(int(B), int(beam_width), int(lm is not None), int(hotwords is not None))
    if n == 0:
        raise ValueError(f"ctc_beam_stream_state: batch {B} or beam_width {beam_width} outside the supported sizes")
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def ctc_beam_stream_nodes(B: int, cap_frames: int, beam_width: int, dev, old: Tensor | None = None, old_cap: int = 0) -> Tensor:
    """Node storage for ctc_beam_stream_feed with room for cap_frames frames per utterance: (B, 3, cap_frames * beam_width) int32 on dev.
    With `old` (the storage of capacity old_cap <= cap_frames) every utterance's three arrays are copied to the front of their new
    places: node ids do not depend on the capacity."""
    nodes = torch.empty((int(B), 3, int(cap_frames) * int(beam_width)), dtype=torch.int32, device=dev)
    if old is not None:
        nodes[:, :, :int(old_cap) * int(beam_width)] = old.view(int(B), 3, -1)
    return nodes


def ctc_beam_stream_feed(probs: Tensor | None, sizes: Tensor | None, state: Tensor, nodes: Tensor, cap_frames: int, frames_bound: int,
                         n_out: int, blank: int = 0, beam_width: int = 100, cutoff_top_n: int = 40, cutoff_prob: float = 1.0, lm=None,
                         alpha: float = 0.0, beta: float = 0.0, hotwords=None, classes: int | None = None):
    """One chunk of frames into B running beam searches (contract: include/ds2hip.h, ds2_ctc_beam_stream_feed_f32): probs (B,T,C) fp32 on
    the GPU, or None for a pure read-out (`classes` then gives C); sizes (B) the chunk's valid frames per utterance or None; state and
    nodes as ctc_beam_stream_state / ctc_beam_stream_nodes make them (the batch is nodes.shape[0]), nodes with room for cap_frames >=
    frames_bound + T frames; frames_bound an upper bound of the frames consumed so far.  The search's arguments are ctc_beam_decode's
    and must not change within a stream.  n_out in 0..beam_width slots are read out -> (labels (B,n_out,W) i32, offsets (B,n_out,W) i32,
    lengths (B,n_out) i32, scores (B,n_out) fp32, stable_len (B) i32, frames (B) i32), all on the GPU, W = max(frames_bound + T, 1); the
    first four are None when n_out == 0.  A read-out has the bits of ctc_beam_decode on the frames so far; stable_len labels and offsets
    of every beam are final.  One launch on the current stream, nothing is copied back."""
    return _beam_stream_feed("ctc_beam_stream_feed", probs, sizes, state, nodes, cap_frames, frames_bound, None, n_out, blank, beam_width,
                             cutoff_top_n, cutoff_prob, lm, alpha, beta, hotwords, classes)


def ctc_beam_stream_feed_committed(probs: Tensor | None, sizes: Tensor | None, state: Tensor, nodes: Tensor, cap_rows: int, rows_bound: int,
                                   labels_bound: int, n_out: int, blank: int = 0, beam_width: int = 100, cutoff_top_n: int = 40,
                                   cutoff_prob: float = 1.0, lm=None, alpha: float = 0.0, beta: float = 0.0, hotwords=None,
                                   classes: int | None = None):
    """ctc_beam_stream_feed for a state that ctc_beam_stream_commit has compacted (contract: include/ds2hip.h,
    ds2_ctc_beam_stream_feed_committed_f32): the node capacity and rows_bound count rows of beam_width nodes (rows_bound: at least
    ceil(M / beam_width) of the last commit plus the frames fed since, for every utterance), and the read-out rows hold the pairs from
    each utterance's committed length on, in rows of W = max(labels_bound + T, 1) (labels_bound: at least the last commit's info[b][2]
    plus the frames fed since); lengths, scores and stable_len stay absolute.  Same outputs as ctc_beam_stream_feed."""
    if not _is_int(labels_bound, 0, 0x7fffffff):
        raise ValueError(f"ctc_beam_stream_feed_committed: labels_bound must be a non-negative integer, got {labels_bound!r}")
    return _beam_stream_feed("ctc_beam_stream_feed_committed", probs, sizes, state, nodes, cap_rows, rows_bound, int(labels_bound), n_out,
                             blank, beam_width, cutoff_top_n, cutoff_prob, lm, alpha, beta, hotwords, classes)


def _beam_stream_feed(who, probs, sizes, state, nodes, cap, bound, labels_bound, n_out, blank, beam_width, cutoff_top_n, cutoff_prob, lm, alpha,
                      beta, hotwords, classes):
    """The host path of the two feed entries: labels_bound None is the uncommitted one, whose read-out rows hold every frame"""
    lib = _lib.load()
    dev = state.device
    if probs is None:
        if classes is None:
            raise ValueError(f"{who}: a call without probs needs the number of classes")
        B, T, C, ld_b, ld_t = nodes.shape[0], 0, int(classes), 1, 1
    else:
        B, T, C, pdev, ld_b, ld_t = _posteriors(who, probs, off_gpu=_lib.DS2LibraryError)
        if pdev != dev:
            raise ValueError(f"{who}: probs on {pdev}, the state on {dev}")
    K = _beam_search_args(who, lib, C, blank, beam_width, cutoff_top_n, lm, hotwords)
    if not _is_int(n_out, 0, K):
        raise ValueError(f"{who}: n_out must be an integer in 0..beam_width ({K}), got {n_out!r}")
    _chk_on_dev(who, dev, torch.uint8, {"state": state})
    _chk_on_dev(who, dev, torch.int32, {"nodes": nodes})
    sizes = _sizes_i32(sizes, B, dev)
    n_out, W = int(n_out), max((int(bound) if labels_bound is None else labels_bound) + T, 1)
    labels = offs = lens = scores = None
    if n_out:
        labels = torch.empty((B, n_out, W), dtype=torch.int32, device=dev)
        offs = torch.empty((B, n_out, W), dtype=torch.int32, device=dev)
        lens = torch.empty((B, n_out), dtype=torch.int32, device=dev)
        scores = torch.empty((B, n_out), dtype=torch.float32, device=dev)
    tail = torch.empty((2, B), dtype=torch.int32, device=dev)
    lm_args, hot_args, _keep = _beam_arm_args(lm, alpha, beta, hotwords, dev)
    head = (_ptr(probs), ld_b, ld_t, B, T, C, _ptr(sizes), int(blank), K, int(cutoff_top_n), float(cutoff_prob), *lm_args, *hot_args,
            state.data_ptr(), state.numel(), nodes.data_ptr(), nodes.numel() * 4, int(cap), int(bound))
    outs = (n_out, W, _ptr(labels), _ptr(offs), _ptr(lens), _ptr(scores), tail[0].data_ptr(), tail[1].data_ptr(), _stream())
    if labels_bound is None:
        _lib.check(lib.ds2_ctc_beam_stream_feed_f32(*head, *outs), "ds2_ctc_beam_stream_feed_f32")
    else:
        _lib.check(lib.ds2_ctc_beam_stream_feed_committed_f32(*head, labels_bound, *outs), "ds2_ctc_beam_stream_feed_committed_f32")
    return labels, offs, lens, scores, tail[0], tail[1]


def ctc_beam_stream_commit(state: Tensor, nodes: Tensor, cap_rows: int, nodes_out: Tensor, cap_rows_out: int, beam_width: int, lm, hotwords,
                           width: int, cut_frame: Tensor | None = None):
    """Commit and compaction of B running beam searches' back-pointers, one launch (contract: include/ds2hip.h,
    ds2_ctc_beam_stream_commit): the stable (label, offset) pairs that have not left yet go to rows of `width` cells, the live tree of
    `nodes` (capacity cap_rows rows of beam_width nodes) is renumbered into nodes_out, a distinct buffer of cap_rows_out >= cap_rows rows
    as ctc_beam_stream_nodes makes them, and the state is rewritten to match; feed it through ctc_beam_stream_feed_committed from then
    on.  cut_frame: (B) int32 on the GPU or None; where >= 0 the forced cut of the contract runs first.  lm / hotwords: what the stream
    was opened with.  -> (info (B, 4): pairs committed now, M live nodes, longest live beam - committed length, frame of the last
    committed pair; dropped (B): the beams the cut dropped; labels, offsets (B, width): the committed pairs, zero past info[b][0];
    packed), all int32 on the GPU: the first four are views of `packed`, in that order, so one copy of it brings everything to the host
    (commit_unpack splits the copy)."""
    who = "ctc_beam_stream_commit"
    lib = _lib.load()
    dev = state.device
    _chk_on_dev(who, dev, torch.uint8, {"state": state})
    _chk_on_dev(who, dev, torch.int32, {"nodes": nodes, "nodes_out": nodes_out})
    if cut_frame is not None:
        _chk_on_dev(who, dev, torch.int32, {"cut_frame": cut_frame})
    B, K = nodes.shape[0], int(beam_width)
    if not _is_int(width, 0, 0x7fffffff):
        raise ValueError(f"{who}: width must be a non-negative integer, got {width!r}")
    if nodes_out.shape[0] != B or (cut_frame is not None and cut_frame.numel() != B):
        raise ValueError(f"{who}: nodes of {B} utterances, nodes_out of {nodes_out.shape[0]}"
                         + (f", cut_frame of {cut_frame.numel()}" if cut_frame is not None else ""))
    Wc = int(width)
    packed = torch.zeros((B * (5 + 2 * Wc),), dtype=torch.int32, device=dev)
    info, dropped, lab, off = commit_unpack(packed, B, Wc)
    wsb = lib.ds2_ctc_beam_stream_commit_workspace_bytes(B, int(cap_rows), K)
    ws = _ws(wsb, dev) if wsb else None
    _lib.check(lib.ds2_ctc_beam_stream_commit(state.data_ptr(), state.numel(), B, K, int(lm is not None), int(hotwords is not None),
                                              nodes.data_ptr(), nodes.numel() * 4, int(cap_rows), nodes_out.data_ptr(), nodes_out.numel() * 4,
                                              int(cap_rows_out), _ptr(cut_frame), Wc, _ptr(lab) if Wc else None, _ptr(off) if Wc else None,
                                              info.data_ptr(), dropped.data_ptr(), _ptr(ws), wsb, _stream()), "ds2_ctc_beam_stream_commit")
    return info, dropped, lab, off, packed


def commit_unpack(packed: Tensor, B: int, width: int):
    """ctc_beam_stream_commit's packed result, on any device -> views (info (B, 4), dropped (B), labels (B, width), offsets (B, width))"""
    B, Wc = int(B), int(width)
    if packed.numel() != B * (5 + 2 * Wc):
        raise ValueError(f"commit_unpack: {packed.numel()} values for {B} utterances and rows of {Wc}")
    return (packed[:4 * B].view(B, 4), packed[4 * B:5 * B], packed[5 * B:5 * B + B * Wc].view(B, Wc), packed[5 * B + B * Wc:].view(B, Wc))


def lm_score(labels: Tensor, off: Tensor, lens: Tensor, lm, max_len: int):
    """The LM term of P finished label sequences, one launch -> (lm_sum (P) fp32 log10, n_tok (P) i32, n_oov (P) i32) on the GPU
    (contract: include/ds2hip.h, ds2_lm_score_seqs).  labels: int32 on the GPU, any shape, read flat; sequence p is
    labels.view(-1)[off[p]:][:lens[p]]; off (P) int64 and lens (P) int32 on the GPU; lm a decoders.lm.NgramLM (its classes, blank and
    space are the call's); max_len bounds every length.  A sequence longer than max_len, outside the buffer, or holding the blank or a
    label outside the classes gets NaN, -1, -1.  lm_sum leaves OOV tokens out and n_oov counts them: lm_sum - 1000 * n_oov is the beam
    search's LM total."""
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise ValueError("lm_score: labels must be a GPU tensor (no CPU fallback exists)")
    dev = labels.device
    _chk_on_dev("lm_score", dev, torch.int32, {"labels": labels, "lens": lens})
    _chk_on_dev("lm_score", dev, torch.int64, {"off": off})
    if off.dim() != 1 or lens.dim() != 1 or off.numel() != lens.numel():
        raise ValueError("lm_score: off and lens must be one-dimensional and of one length")
    if lm is None or not hasattr(lm, "packed"):
        raise ValueError("lm_score: lm must be an NgramLM")
    if not _is_int(max_len, 0, 2 ** 31 - 65):
        raise ValueError(f"lm_score: max_len must be an integer in [0, 2^31 - 65], got {max_len!r}")
    P = lens.numel()
    lm_sum = torch.empty((P,), dtype=torch.float32, device=dev)
    n_tok = torch.empty((P,), dtype=torch.int32, device=dev)
    n_oov = torch.empty((P,), dtype=torch.int32, device=dev)
    tab = lm.device_tables(dev)
    _lib.check(_lib.load().ds2_lm_score_seqs(labels.data_ptr(), labels.numel(), off.data_ptr(), lens.data_ptr(), P, int(max_len), tab.data_ptr(),
                                             lm.packed.ctypes.data, lm.packed.nbytes, lm.order, lm.mode, lm.space if lm.space is not None else -1,
                                             lm.C, lm.blank, lm_sum.data_ptr(), n_tok.data_ptr(), n_oov.data_ptr(), _stream()),
               "ds2_lm_score_seqs")
    return lm_sum, n_tok, n_oov


def nbest_sweep(ac: Tensor, lm_sum: Tensor, n_tok: Tensor, n_oov: Tensor, err: Tensor, alphas, betas, oov_score: float = -1000.0,
                want_pick: bool = True):
    """Which slot of every n-best list wins at every point of an (alpha, beta) grid, and the winners' summed errors, one launch ->
    (pick (Ga,Gb,N) i32 or None, total (Ga,Gb,R) i64) on the GPU (contract: include/ds2hip.h, ds2_nbest_sweep).  ac, lm_sum (N,K) fp32,
    n_tok, n_oov (N,K) i32, err (N,K,R) i32, all contiguous on the GPU; alphas / betas: sequences or tensors of Ga / Gb weights.
    Slot k scores (ac + alpha * (lm_sum + oov_score * n_oov)) + beta * n_tok in fp32; NaN counts as -inf, ties go to the lowest k."""
    if not torch.is_tensor(ac) or not ac.is_cuda:
        raise ValueError("nbest_sweep: ac must be a GPU tensor (no CPU fallback exists)")
    dev = ac.device
    _chk_on_dev("nbest_sweep", dev, torch.float32, {"ac": ac, "lm_sum": lm_sum})
    _chk_on_dev("nbest_sweep", dev, torch.int32, {"n_tok": n_tok, "n_oov": n_oov, "err": err})
    if ac.dim() != 2 or ac.shape[1] < 1 or any(t.shape != ac.shape for t in (lm_sum, n_tok, n_oov)):
        raise ValueError("nbest_sweep: ac, lm_sum, n_tok and n_oov must be (N, K) with K >= 1")
    N, K = ac.shape
    if err.dim() != 3 or err.shape[:2] != (N, K) or not 1 <= err.shape[2] <= 64:
        raise ValueError(f"nbest_sweep: err must be ({N}, {K}, R) with 1 <= R <= 64, got {tuple(err.shape)}")
    R = err.shape[2]
    grid = [torch.as_tensor(g, dtype=torch.float32).reshape(-1).to(dev).contiguous() for g in (alphas, betas)]
    Ga, Gb = grid[0].numel(), grid[1].numel()
    if Ga < 1 or Gb < 1:
        raise ValueError("nbest_sweep: alphas and betas must not be empty")
    if math.isnan(float(oov_score)):
        raise ValueError("nbest_sweep: oov_score is NaN")
    pick = torch.empty((Ga, Gb, N), dtype=torch.int32, device=dev) if want_pick else None
    total = torch.empty((Ga, Gb, R), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().ds2_nbest_sweep(ac.data_ptr(), lm_sum.data_ptr(), n_tok.data_ptr(), n_oov.data_ptr(), err.data_ptr(), N, K, R,
                                           float(oov_score), grid[0].data_ptr(), Ga, grid[1].data_ptr(), Gb, _ptr(pick), total.data_ptr(),
                                           _stream()), "ds2_nbest_sweep")
    return pick, total


NGRAM_FALLBACK = (0.5, 1.0, 1.5)


def ngram_max_order(n_vocab: int) -> int:
    """the largest order whose n-grams over n_vocab ids (the three specials included) fit the 64-bit key, at most 6"""
    return int(_lib.load().ds2_ngram_max_order(int(n_vocab)))


def ngram_positions(lengths, order: int):
    """how many n-grams of each order 1..order the framed sentences hold: a sentence of L > 0 tokens has L + 3 - n of order n"""
    L = np.asarray(lengths, dtype=np.int64)
    L = L[L > 0]
    return [int(np.maximum(L + 3 - n, 0).sum()) for n in range(1, order + 1)]


def ngram_slots(positions, n_vocab: int, order: int):
    """the slots of each order's counting table: a power of two of at least twice min(positions, n_vocab^n), so never more than half full"""
    return [max(2, 1 << (2 * min(int(positions[n - 1]), int(n_vocab) ** n) - 1).bit_length()) for n in range(1, order + 1)]


def _ngram_args(who, n_tokens, lengths, n_vocab, order, discount_fallback):
    """The host path of both estimators: the checks every entry shares -> (order, n_vocab, fallback (3) float64).  lengths: the sentence
    lengths on the host (offsets' differences)."""
    if not _is_int(order, 1, 6):
        raise ValueError(f"{who}: order must be an integer in [1, 6], got {order!r}")
    if not _is_int(n_vocab, 4, 2 ** 31 - 1):
        raise ValueError(f"{who}: n_vocab must be an integer of at least 4 (<unk>, <s>, </s> and one token), got {n_vocab!r}")
    order, n_vocab = int(order), int(n_vocab)
    top = ngram_max_order(n_vocab)
    if order > top:
        raise ValueError(f"{who}: order {order} over {n_vocab} ids does not fit the 64-bit n-gram key: "
                         f"this vocabulary admits order {top} at most")
    fb = np.asarray(discount_fallback, dtype=np.float64).reshape(-1)
    if fb.shape != (3,) or not all(0.0 <= fb[k] <= k + 1 for k in range(3)):
        raise ValueError(f"{who}: discount_fallback must be three discounts with D_k in [0, k], got {discount_fallback!r}")
    lengths = np.asarray(lengths)
    if lengths.size < 1 or lengths.min() < 0 or int(lengths.sum()) != n_tokens or n_tokens < 1:
        raise ValueError(f"{who}: offsets must ascend from 0 to the number of tokens, and there must be at least one token")
    if n_tokens + 2 * lengths.size >= 2 ** 31 - 1:
        raise ValueError(f"{who}: {n_tokens} tokens in {lengths.size} sentences exceed the 2^31 framed positions of one call")
    return order, n_vocab, np.ascontiguousarray(fb)


def _ngram_discounts(order, glob_host, fb):
    """ds2_ngram_discounts on a host copy of glob -> (D (order,4), fell_back (order), coc (order,4), log10 p(<unk>))"""
    D, fell, coc = np.zeros((order, 4), np.float64), np.zeros(order, np.int32), np.zeros((order, 4), np.int64)
    unk = C.c_double()
    _lib.check(_lib.load().ds2_ngram_discounts(order, glob_host.ctypes.data, fb.ctypes.data, D.ctypes.data, fell.ctypes.data, coc.ctypes.data,
                                               C.byref(unk)), "ds2_ngram_discounts")
    return D, fell, coc, unk.value


def _ngram_result(order, n_vocab, per_order, D, fell, coc, unk):
    return {"order": order, "n_vocab": n_vocab, "bits": (n_vocab - 1).bit_length(), "orders": per_order, "discounts": D[:, 1:].copy(),
            "count_of_counts": coc, "fallback_orders": [n + 1 for n in range(order) if fell[n]], "unk_log10": float(unk)}


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def ngram_count(tokens: Tensor, offsets: Tensor, n_vocab: int, order: int = 3, discount_fallback=NGRAM_FALLBACK, slots=None):
    """The counting launch of ngram_estimate (contract: include/ds2hip.h, ds2_ngram_count): tokens flat int32 and offsets int64 on the
    GPU -> the state ngram_solve and ngram_collect take: per-order tables keys (slots) i64, vals (slots, 8) i32, prob (slots, 2) f64, and
    glob.  slots: per-order table sizes (powers of two) instead of ngram_slots', for the tests."""
    if not torch.is_tensor(tokens) or not tokens.is_cuda:
        raise ValueError("ngram_count: tokens must be a GPU tensor (ngram_estimate_host is the estimator without one)")
    dev = tokens.device
    _chk_on_dev("ngram_count", dev, torch.int32, {"tokens": tokens})
    _chk_on_dev("ngram_count", dev, torch.int64, {"offsets": offsets})
    if tokens.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError("ngram_count: tokens and offsets must be one-dimensional, offsets with one entry per sentence and one more")
    lengths = offsets.diff().cpu().numpy()
    if int(offsets[0]) != 0:
        raise ValueError("ngram_count: offsets must start at 0")
    order, n_vocab, fb = _ngram_args("ngram_count", tokens.numel(), lengths, n_vocab, order, discount_fallback)
    slots = ngram_slots(ngram_positions(lengths, order), n_vocab, order) if slots is None else [int(s) for s in slots]
    if len(slots) != order or any(s < 2 or s > 2 ** 30 or s & (s - 1) for s in slots):
        raise ValueError(f"ngram_count: slots must be {order} powers of two in [2, 2^30], got {slots}")
    lib = _lib.load()
    st = {"order": order, "n_vocab": n_vocab, "fallback": fb, "slots": slots, "device": dev,
          "keys": [torch.empty(s, dtype=torch.int64, device=dev) for s in slots],
          "vals": [torch.empty((s, 8), dtype=torch.int32, device=dev) for s in slots],
          "prob": [torch.empty((s, 2), dtype=torch.float64, device=dev) for s in slots],
          "glob": torch.empty(lib.ds2_ngram_glob_words(), dtype=torch.int64, device=dev)}
    st["c_slots"] = np.array(slots, dtype=np.int64)
    st["c_keys"], st["c_vals"], st["c_prob"] = (_ptr_array([t.data_ptr() for t in st[k]]) for k in ("keys", "vals", "prob"))
    _lib.check(lib.ds2_ngram_count(tokens.data_ptr(), tokens.numel(), offsets.data_ptr(), offsets.numel() - 1, n_vocab, order,
                                   st["c_slots"].ctypes.data, st["c_keys"], st["c_vals"], st["glob"].data_ptr(), _stream()), "ds2_ngram_count")
    return st


def ngram_solve(st):
    """The adjusted-count launches, the discounts (on the host, from the 4 x order count-of-counts: one small download) and the
    probability launches on ngram_count's state; a flag the kernels set (a full table, a bad token id) raises here."""
    lib = _lib.load()
    order, n_vocab = st["order"], st["n_vocab"]
    _lib.check(lib.ds2_ngram_adjust(n_vocab, order, st["c_slots"].ctypes.data, st["c_keys"], st["c_vals"], st["glob"].data_ptr(), _stream()),
               "ds2_ngram_adjust")
    glob_host = np.ascontiguousarray(st["glob"].cpu().numpy().view(np.uint64))
    st["D"], st["fell"], st["coc"], st["unk"] = _ngram_discounts(order, glob_host, st["fallback"])
    _lib.check(lib.ds2_ngram_probs(n_vocab, order, st["c_slots"].ctypes.data, st["c_keys"], st["c_vals"], st["c_prob"], st["glob"].data_ptr(),
                                   st["D"].ctypes.data, _stream()), "ds2_ngram_probs")
    glob_host = st["glob"].cpu().numpy().view(np.uint64)
    if glob_host[6]:
        raise _lib.DS2LibraryError("ngram_solve: internal error: a context or suffix of a counted n-gram is in no table")
    return st


def _ngram_sorted(st):
    """the distinct entries of every order of a solved state, sorted by key, still on the device: (keys i64, vals (rows, 3), prob (rows, 2))"""
    out = []
    for keys, vals, prob in zip(st["keys"], st["vals"], st["prob"]):
        idx = torch.nonzero(keys).view(-1)
        k = keys[idx]
        srt = torch.sort(k ^ torch.iinfo(torch.int64).min)          # unsigned order of the 64-bit keys
        idx = idx[srt.indices]
        out.append((k[srt.indices], vals[idx][:, :3], prob[idx]))
    return out


def ngram_collect(st):
    """The distinct entries of every order of a solved state, sorted by key on the device (which slot a key took varies from run to run;
    the sorted arrays do not), on the host: the dictionary ngram_estimate returns."""
    per_order = []
    for k, v, p in _ngram_sorted(st):
        v, p = v.cpu().numpy(), p.cpu().numpy()
        per_order.append((k.cpu().numpy().view(np.uint64), v[:, 0].astype(np.int64), v[:, 2].astype(np.int64),
                          np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])))
    return _ngram_result(st["order"], st["n_vocab"], per_order, st["D"], st["fell"], st["coc"], st["unk"])


def ngram_collect_model(st):
    """ngram_collect without the download: the model ngram_eval and ngram_prune take (see ngram_model), its arrays left on the device,
    with what the estimator's dictionary holds beside its arrays under "meta"."""
    dev = st["device"]
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)   # noqa: E731   (the <unk> row: key 0 sorts first)
    keys, lp, lb, count, adj = [], [], [], [], []
    for n, (k, v, p) in enumerate(_ngram_sorted(st), 1):
        c, a, x, y = v[:, 0].to(torch.int64), v[:, 2].to(torch.int64), p[:, 0].contiguous(), p[:, 1].contiguous()
        if n == 1:
            k, c, a = torch.cat([one(0, torch.int64), k]), torch.cat([one(0, torch.int64), c]), torch.cat([one(0, torch.int64), a])
            x, y = torch.cat([one(st["unk"], torch.float64), x]), torch.cat([one(math.nan, torch.float64), y])
        keys.append(k.contiguous()), lp.append(x), lb.append(y), count.append(c), adj.append(a)
    meta = _ngram_result(st["order"], st["n_vocab"], [], st["D"], st["fell"], st["coc"], st["unk"])
    return {"order": st["order"], "n_vocab": st["n_vocab"], "bits": meta["bits"], "keys": keys, "lp": lp, "lb": lb, "count": count,
            "adjusted": adj, "meta": meta}


def ngram_model(raw, device):
    """The model ngram_eval and ngram_prune take, from the dictionary ngram_estimate returns (or one of the same layout whose counts are
    None and whose "unk_log10" is None when the model lists no <unk>): per order, torch tensors on `device` (a GPU, or "cpu" for the host
    twins): keys int64 (the u64 keys' bits, ascending as unsigned), lp, lb float64 (NaN: no backoff), count / adjusted int64 or None.
    <unk> is row 0 of the 1-grams."""
    dev = torch.device(device)
    keys, lp, lb, count, adj = [], [], [], [], []
    for n, (k, c, a, x, y) in enumerate(raw["orders"], 1):
        k, x, y = np.asarray(k).view(np.int64), np.asarray(x, np.float64), np.asarray(y, np.float64)
        if n == 1 and raw["unk_log10"] is not None:
            k, x, y = np.concatenate([[0], k]), np.concatenate([[raw["unk_log10"]], x]), np.concatenate([[np.nan], y])
            c, a = (None if v is None else np.concatenate([[0], v]) for v in (c, a))
        keys.append(torch.from_numpy(np.ascontiguousarray(k, np.int64)).to(dev))
        lp.append(torch.from_numpy(np.ascontiguousarray(x)).to(dev)), lb.append(torch.from_numpy(np.ascontiguousarray(y)).to(dev))
        count.append(None if c is None else torch.from_numpy(np.ascontiguousarray(c, np.int64)).to(dev))
        adj.append(None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev))
    meta = {k: v for k, v in raw.items() if k != "orders"}
    return {"order": raw["order"], "n_vocab": raw["n_vocab"], "bits": raw["bits"], "keys": keys, "lp": lp, "lb": lb, "count": count,
            "adjusted": adj, "meta": meta}


def ngram_model_download(model):
    """a model's arrays on the host in the layout of ngram_estimate's dictionary: the <unk> row leaves the 1-grams for "unk_log10" (None
    when there is none), and "order" is the model's"""
    per_order, unk = [], None
    host = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    for n in range(model["order"]):
        k, x, y, c, a = (host(model[f][n]) for f in ("keys", "lp", "lb", "count", "adjusted"))
        if n == 0 and len(k) and k[0] == 0:
            unk = float(x[0])
            k, x, y, c, a = (None if v is None else v[1:] for v in (k, x, y, c, a))
        per_order.append((np.ascontiguousarray(k).view(np.uint64), c, a, np.ascontiguousarray(x), np.ascontiguousarray(y)))
    return {**model["meta"], "order": model["order"], "n_vocab": model["n_vocab"], "bits": model["bits"], "orders": per_order,
            "unk_log10": unk}


def _ngram_model_args(who, model):
    """The host path of every entry that reads a model: its checks -> (device, the arguments every ds2_ngram_eval / _prune_* entry starts
    or continues with: n_vocab, order, cnt, keys, lp, lb; keep `hold` alive across the call)"""
    order, n_vocab = model["order"], model["n_vocab"]
    if not _is_int(order, 1, 6) or len(model["keys"]) != order or len(model["lp"]) != order or len(model["lb"]) != order:
        raise ValueError(f"{who}: the model must list keys, lp and lb for each of its {order!r} orders (1..6)")
    if order * model["bits"] > 64 or model["bits"] != (n_vocab - 1).bit_length():
        raise ValueError(f"{who}: order {order} over {n_vocab} ids does not fit the 64-bit n-gram key")
    dev = model["keys"][0].device
    for n in range(order):
        k, x, y = model["keys"][n], model["lp"][n], model["lb"][n]
        if not (k.dtype == torch.int64 and x.dtype == y.dtype == torch.float64 and k.dim() == 1 and k.shape == x.shape == y.shape):
            raise ValueError(f"{who}: order {n + 1}: keys int64, lp and lb float64, one-dimensional and of one length")
        if not (k.device == x.device == y.device == dev and k.is_contiguous() and x.is_contiguous() and y.is_contiguous()):
            raise ValueError(f"{who}: order {n + 1}: the arrays must be contiguous and on one device")
    hold = np.array([k.numel() for k in model["keys"]], dtype=np.int64)
    args = (n_vocab, order, hold.ctypes.data, *(_ptr_array([t.data_ptr() for t in model[f]]) for f in ("keys", "lp", "lb")))
    return dev, args, hold


def _ngram_call(name, dev, *args):
    """one ds2_ngram_eval / _prune_* entry: the kernels on a GPU (the stream is the last argument), the host twin for CPU tensors"""
    lib = _lib.load()
    if dev.type == "cpu":
        _lib.check(getattr(lib, name + "_host")(*args), name + "_host")
    else:
        _lib.check(getattr(lib, name)(*args, _stream()), name)


def ngram_eval(model, tokens: Tensor, offsets: Tensor):
    """log10 p of every position of sentences of token ids under a model (contract: include/ds2hip.h, ds2_ngram_eval; ngram_model makes
    the model): tokens flat int32 (0 = <unk>), offsets int64, both on the model's device.  -> (log10_prob float64, order int32), each of
    tokens.numel() + n_sent positions: sentence s owns offsets[s] + s .. offsets[s+1] + s, its tokens and then </s>.  order is that of
    the n-gram that was listed; 0, with NaN, where the token is no 1-gram of the model."""
    dev, args, hold = _ngram_model_args("ngram_eval", model)
    if not torch.is_tensor(tokens) or not torch.is_tensor(offsets) or tokens.device != dev or offsets.device != dev:
        raise ValueError(f"ngram_eval: tokens and offsets must be tensors on the model's device ({dev})")
    if tokens.dtype != torch.int32 or offsets.dtype != torch.int64 or tokens.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError("ngram_eval: tokens must be one-dimensional int32, offsets int64 with one entry per sentence and one more")
    tokens, offsets = tokens.contiguous(), offsets.contiguous()
    if int(offsets[0]) != 0 or int(offsets[-1]) != tokens.numel() or bool((offsets.diff() < 0).any()):
        raise ValueError("ngram_eval: offsets must ascend from 0 to the number of tokens")
    if tokens.numel() and (int(tokens.min()) < 0 or int(tokens.max()) >= model["n_vocab"]):
        raise ValueError(f"ngram_eval: a token id outside [0, {model['n_vocab']})")
    P = tokens.numel() + offsets.numel() - 1
    if P >= 2 ** 31 - 1:
        raise ValueError(f"ngram_eval: {P} positions exceed the 2^31 of one call")
    lp = torch.empty(P, dtype=torch.float64, device=dev)
    order = torch.empty(P, dtype=torch.int32, device=dev)
    _ngram_call("ds2_ngram_eval", dev, tokens.data_ptr(), tokens.numel(), offsets.data_ptr(), offsets.numel() - 1, *args, lp.data_ptr(),
                order.data_ptr())
    return lp, order


def _ngram_sums(model, n, want_q=False):
    """ds2_ngram_prune_sums for the children of order n -> (sp, sq per row of order n - 1, q per row of order n or None)"""
    dev, args, hold = _ngram_model_args("ngram_prune", model)
    rows, ctx = model["keys"][n - 1].numel(), model["keys"][n - 2].numel()
    sp, sq = torch.empty(ctx, dtype=torch.float64, device=dev), torch.empty(ctx, dtype=torch.float64, device=dev)
    q = torch.empty(rows, dtype=torch.float64, device=dev) if want_q else None
    tail = ()
    if dev.type != "cpu":
        scratch = torch.empty(4 * ((rows + 63) // 64), dtype=torch.float64, device=dev)
        tail = (scratch.data_ptr(), scratch.numel())
    _ngram_call("ds2_ngram_prune_sums", dev, *args, n, _ptr(q), sp.data_ptr(), sq.data_ptr(), *tail)
    return sp, sq, q


def ngram_prune_values(model, threshold: float):
    """The entropy launch on a model (contract: include/ds2hip.h, ds2_ngram_prune_sums / _entropy) -> (val, mark): per order n (entry
    n - 1; entry 0 is None) exp(dH) - 1 of removing each n-gram alone, float64, and whether it is below the threshold, bool."""
    dev, args, hold = _ngram_model_args("ngram_prune", model)
    try:                                                                 # (any real number: a NumPy scalar or a 0-d tensor as well)
        theta = math.nan if isinstance(threshold, (bool, str, bytes)) else float(threshold)
    except (TypeError, ValueError):
        theta = math.nan
    if not 0.0 < theta < math.inf:
        raise ValueError(f"ngram_prune: threshold must be a positive number, got {threshold!r}")
    threshold = theta
    N = model["order"]
    q, sp, sq, val, mark = ([None] * N for _ in range(5))
    for n in range(2, N + 1):
        sp[n - 1], sq[n - 1], q[n - 1] = _ngram_sums(model, n, want_q=True)
        val[n - 1] = torch.empty_like(q[n - 1])
        mark[n - 1] = torch.empty(q[n - 1].numel(), dtype=torch.uint8, device=dev)
    arr = lambda ts: _ptr_array([0 if t is None else t.data_ptr() for t in ts])   # noqa: E731
    _ngram_call("ds2_ngram_prune_entropy", dev, *args, arr(q), arr(sp), arr(sq), float(threshold), arr(val), arr(mark))
    return val, [None if m is None else m.bool() for m in mark]


def ngram_prune(model, threshold=None, min_count=None):
    """Prune a model (contract: include/ds2hip.h, ds2_ngram_prune_*) -> a model of the same layout, or `model` itself when nothing is
    marked.  min_count: `order` integers >= 1, non-decreasing, the first ignored: an n-gram of order n >= 2 whose raw count is below
    min_count[n-1] is marked (the model must have counts).  threshold > 0: an n-gram of order >= 2 is marked when removing it alone
    raises the model's perplexity by less than that fraction (on the model after the count cut, when both are given).  Then marked
    n-grams that are the context of a kept one are kept, the kept rows are gathered (their lp bit for bit), and the backoffs of every
    context that still has a child are recomputed bottom up; an order left empty is dropped."""
    dev, _, _ = _ngram_model_args("ngram_prune", model)
    N = model["order"]
    if min_count is not None:
        try:
            mc = [int(c) for c in min_count]
            ok = len(mc) == N and all(int(c) == c and not isinstance(c, bool) for c in min_count)
        except (TypeError, ValueError):
            mc, ok = [], False
        if not ok or any(c < 1 for c in mc) or any(a > b for a, b in zip(mc[1:], mc[2:])):
            raise ValueError(f"ngram_prune: min_count must be {N} integers >= 1 that do not decrease (the first is ignored), got {min_count!r}")
        if any(c is None for c in model["count"]):
            raise ValueError("ngram_prune: min_count needs a model that has counts (one estimated here, not one read from a file)")
        marks = [None] + [model["count"][n - 1] < mc[n - 1] for n in range(2, N + 1)]
        model = _ngram_cut(model, marks)
    if threshold is None:
        return model
    _, marks = ngram_prune_values(model, threshold)
    return _ngram_cut(model, marks[:model["order"]])


def _ngram_cut(model, marks):
    """closure, gathering of the kept rows and the new backoffs for the marks of one pruning mode (entry n - 1 for order n, bool)"""
    dev, args, hold = _ngram_model_args("ngram_prune", model)
    N = model["order"]
    marks = [None if m is None else m.to(torch.uint8).contiguous() for m in marks]
    for n in range(N, 2, -1):
        _ngram_call("ds2_ngram_prune_closure", dev, *args, n, marks[n - 1].data_ptr(), marks[n - 2].data_ptr())
    if not any(m is not None and bool(m.any()) for m in marks):
        return model
    keep = [None] + [m == 0 for m in marks[1:]]
    take = lambda ts: [t if k is None or t is None else t[k].contiguous() for t, k in zip(ts, keep)]   # noqa: E731
    new = {**model, **{f: take(model[f]) for f in ("keys", "lp", "lb", "count", "adjusted")}}
    top = max(n for n in range(1, N + 1) if new["keys"][n - 1].numel() or n == 1)
    new["order"] = top
    for f in ("keys", "lp", "lb", "count", "adjusted"):
        new[f] = new[f][:top]
    new["lb"][top - 1] = torch.full_like(new["lb"][top - 1], math.nan)      # the highest order lists no backoff
    for n in range(1, top):
        # the contexts of order n from their kept children of order n + 1; q reads the orders up to n, whose backoffs below n are done
        sp, sq, _ = _ngram_sums(new, n + 1)
        lb = torch.empty_like(sp)
        _ngram_call("ds2_ngram_prune_backoff", dev, sp.numel(), sp.data_ptr(), sq.data_ptr(), lb.data_ptr())
        new["lb"][n - 1] = lb
    return new


def ngram_estimate(tokens: Tensor, offsets: Tensor, n_vocab: int, order: int = 3, discount_fallback=NGRAM_FALLBACK, slots=None):
    """An interpolated modified-Kneser-Ney model from sentences of token ids, on the GPU (contract: include/ds2hip.h, ds2_ngram_*):
    tokens flat int32 with ids in [3, n_vocab) (0 <unk>, 1 <s>, 2 </s> are the kernel's), sentence s is tokens[offsets[s]:offsets[s+1]].
    -> {"orders": per order n, sorted by key: (keys u64, count, adjusted, log10_prob, log10_backoff (NaN: none)), "discounts" (order, 3),
    "count_of_counts" (order, 4), "fallback_orders", "unk_log10", "bits": the bits of one token in a key (the oldest token highest)}."""
    return ngram_collect(ngram_solve(ngram_count(tokens, offsets, n_vocab, order, discount_fallback, slots)))


def ngram_estimate_host(tokens, offsets, n_vocab: int, order: int = 3, discount_fallback=NGRAM_FALLBACK):
    """ngram_estimate's host twin (ds2_ngram_estimate_host: std::unordered_map and the same formula routines): tokens int32 and offsets
    int64 NumPy arrays -> the same dictionary.  No GPU is needed."""
    tokens = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32).reshape(-1))
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if offsets.size < 2 or offsets[0] != 0:
        raise ValueError("ngram_estimate_host: offsets must start at 0 and have one entry per sentence and one more")
    lengths = np.diff(offsets)
    order, n_vocab, fb = _ngram_args("ngram_estimate_host", tokens.size, lengths, n_vocab, order, discount_fallback)
    cap = np.array([max(1, min(p, n_vocab ** n)) for n, p in enumerate(ngram_positions(lengths, order), 1)], dtype=np.int64)
    keys = [np.zeros(c, np.uint64) for c in cap]
    count, adj = [np.zeros(c, np.uint32) for c in cap], [np.zeros(c, np.uint32) for c in cap]
    lp, lb = [np.zeros(c, np.float64) for c in cap], [np.zeros(c, np.float64) for c in cap]
    n_distinct = np.zeros(order, np.int64)
    D, fell, coc = np.zeros((order, 4), np.float64), np.zeros(order, np.int32), np.zeros((order, 4), np.int64)
    unk = C.c_double()
    arr = lambda xs: _ptr_array([x.ctypes.data for x in xs])   # noqa: E731
    _lib.check(_lib.load().ds2_ngram_estimate_host(tokens.ctypes.data, tokens.size, offsets.ctypes.data, offsets.size - 1, n_vocab, order,
                                                   fb.ctypes.data, cap.ctypes.data, arr(keys), arr(count), arr(adj), arr(lp), arr(lb),
                                                   n_distinct.ctypes.data, coc.ctypes.data, D.ctypes.data, fell.ctypes.data, C.byref(unk)),
               "ds2_ngram_estimate_host")
    per_order = [(keys[n][:d].copy(), count[n][:d].astype(np.int64), adj[n][:d].astype(np.int64), lp[n][:d].copy(), lb[n][:d].copy())
                 for n, d in enumerate(n_distinct.tolist())]
    return _ngram_result(order, n_vocab, per_order, D, fell, coc, unk.value)


_BASIS_CACHE = {}


def dft_basis_host(n_fft: int, window: str):
    """The numpy half of `dft_basis` (no device needed): the (n_fft, 2*(n_fft/2+1)) float32 array, computed in float64 and rounded once."""
    from scipy.signal import get_window
    w = get_window(window, n_fft, fftbins=True).astype(np.float64)
    k = np.arange(n_fft)[:, None]
    j = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((k * j) % n_fft) / n_fft
    basis = np.empty((n_fft, 2 * (n_fft // 2 + 1)))
    basis[:, 0::2] = w[:, None] * np.cos(ang)
    basis[:, 1::2] = -w[:, None] * np.sin(ang)
    return basis.astype(np.float32)


def dft_basis(n_fft: int, window: str, device) -> Tensor:
    """(n_fft, 2*(n_fft/2+1)) fp32: column 2j = w[k] cos(2 pi k j / n_fft), column 2j+1 = -w[k] sin(...); w = scipy's periodic window
    (what librosa.filters.get_window returns for a name), computed in float64 once per (n_fft, window, device)."""
    key = (n_fft, window, str(device))
    if key not in _BASIS_CACHE:
        _BASIS_CACHE[key] = torch.from_numpy(dft_basis_host(n_fft, window)).to(device)
    return _BASIS_CACHE[key]


def _spectrogram(entry, audio, n_samples, n_fft, hop, window, pad_mode, normalize, frames, aug=None):
    """spectrogram and spectrogram_augmented.  entry: the C entry, sized by its own *_workspace_bytes; aug: what the second one adds,
    (noise, (noise_base, noise_period, noise_start, noise_level), (freq_masks, time_masks))."""
    _chk_f32(audio)
    assert audio.dim() == 2 and audio.stride(1) == 1
    lib = _lib.load()
    B, dev = audio.size(0), audio.device
    n_host = [int(v) for v in n_samples.tolist()]
    fr = [lib.ds2_spectrogram_frames(n, hop) for n in n_host]
    T = frames or max(max(fr), 1)
    n_dev = torch.as_tensor(n_host, dtype=torch.int32).to(dev)
    extra, keep = (), []                                 # device copies stay alive until the call is enqueued
    if aug is not None:
        noise, nz, masks = aug

        def per_utt(x, dtype, shape):
            t = torch.as_tensor(x, dtype=dtype).to(dev).contiguous()
            assert tuple(t.shape) == shape, f"expected shape {shape}, got {tuple(t.shape)}"
            return t
        extra = (None, 0, None, None, None, None)
        if any(a is not None for a in nz):
            assert all(a is not None for a in nz) and noise is not None, "noise_base, noise_period, noise_start, noise_level and noise go together"
            _chk_f32(noise)
            assert noise.dim() == 1 and noise.device == dev
            keep = [per_utt(a, dtype, (B,)) for a, dtype in zip(nz, (torch.int64, torch.int32, torch.int32, torch.float32))]
            extra = (noise.data_ptr(), noise.numel(), *[t.data_ptr() for t in keep])
        for m in masks:
            if m is None:
                extra += (None, 0)
            else:
                mt = torch.as_tensor(m, dtype=torch.int32).to(dev).contiguous()
                assert mt.dim() == 3 and mt.size(0) == B and mt.size(2) == 2, f"masks: expected (B, M, 2), got {tuple(mt.shape)}"
                keep.append(mt)
                extra += (mt.data_ptr() if mt.size(1) else None, mt.size(1))
    out = torch.empty((B, 1, n_fft // 2 + 1, T), dtype=torch.float32, device=dev)
    wsb = getattr(lib, entry[:-len("f32")] + "workspace_bytes")(B, T, n_fft, hop)
    ws = _ws(wsb, dev)
    _lib.check(getattr(lib, entry)(audio.data_ptr(), audio.stride(0), n_dev.data_ptr(), B, T, n_fft, hop, dft_basis(n_fft, window, dev).data_ptr(),
                                   {"constant": 0, "reflect": 1}[pad_mode], int(bool(normalize)), *extra, out.data_ptr(), ws.data_ptr(), wsb,
                                   _stream()), entry)
    return out, torch.tensor([min(f, T) for f in fr], dtype=torch.int32)


def spectrogram(audio: Tensor, n_samples: Tensor, n_fft: int, hop: int, window: str = "hamming", pad_mode: str = "constant",
                normalize: bool = False, frames: int = 0):
    """audio (B, L) fp32 GPU waveforms (rows zero/garbage beyond n_samples) -> (spect (B,1,n_fft/2+1,T), frames (B,) int32 CPU)."""
    return _spectrogram("ds2_spectrogram_f32", audio, n_samples, n_fft, hop, window, pad_mode, normalize, frames)


def spectrogram_augmented(audio: Tensor, n_samples: Tensor, n_fft: int, hop: int, window: str = "hamming", pad_mode: str = "constant",
                          normalize: bool = False, noise: Optional[Tensor] = None, noise_base=None, noise_period=None, noise_start=None,
                          noise_level=None, freq_masks=None, time_masks=None, frames: int = 0):
    """`spectrogram` with noise injection before the STFT and SpecAugment masks after the statistics (ds2_spectrogram_aug_f32, contract in
    include/ds2hip.h).  noise: 1-D fp32 GPU noise bank (or None); noise_base (B) int64, noise_period / noise_start (B) int32, noise_level
    (B) fp32 (0 = no noise for that utterance), all four given or none; freq_masks / time_masks: (B, M, 2) int32 [lo, hi) bin / frame ranges,
    M <= 8, or None.  Per-utterance arrays may live on the host: they are copied to audio's device.  Returns (spect, frames) as `spectrogram`."""
    return _spectrogram("ds2_spectrogram_aug_f32", audio, n_samples, n_fft, hop, window, pad_mode, normalize, frames,
                        aug=(noise, (noise_base, noise_period, noise_start, noise_level), (freq_masks, time_masks)))


TEMPO_SEGMENT_MS, TEMPO_SEARCH_MS, TEMPO_OVERLAP_MS = 82.0, 14.68, 12.0


def tempo_sizes(sample_rate: int, segment_ms: float = TEMPO_SEGMENT_MS, search_ms: float = TEMPO_SEARCH_MS,
                overlap_ms: float = TEMPO_OVERLAP_MS) -> Tuple[int, int, int]:
    """(S, R, O): segment, search and overlap lengths in samples (ds2_tempo_sizes; a host function, no GPU needed)."""
    S, R, O = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().ds2_tempo_sizes(int(sample_rate), float(segment_ms), float(search_ms), float(overlap_ms), C.byref(S), C.byref(R),
                                           C.byref(O)), "ds2_tempo_sizes")
    return S.value, R.value, O.value


def tempo_out_samples(n: int, tempo: float) -> int:
    """floor(n / tempo + 0.5): the length of a tempo-perturbed utterance (ds2_tempo_out_samples; a host function, no GPU needed)."""
    n_out = _lib.load().ds2_tempo_out_samples(int(n), float(tempo))
    if n_out < 0:
        raise _lib.DS2LibraryError(f"tempo_out_samples: n = {n} (0 .. 2^29), tempo = {tempo} (0.5 .. 2) outside the contract")
    return n_out


def _host_array(x, dtype=np.int64):
    """A per-utterance host description (a list, a numpy array or a tensor of any device) as a contiguous numpy array: int64, or float64
    for tempo_gain's factors and gains."""
    return np.ascontiguousarray(x.tolist() if isinstance(x, Tensor) else x, dtype=dtype)


def tempo_gain(audio: Tensor, n_samples, tempo, gain, sample_rate: int, segment_ms: float = TEMPO_SEGMENT_MS,
               search_ms: float = TEMPO_SEARCH_MS, overlap_ms: float = TEMPO_OVERLAP_MS):
    """Tempo (WSOLA time-stretch, pitch kept) and gain perturbation of a waveform batch (ds2_tempo_gain_f32, contract in include/ds2hip.h;
    modelled on sox's `tempo` / `gain` effects, parity with sox itself unpinned; sox's 16-bit requantisation with dither is not reproduced).
    audio (B, L) fp32 GPU rows (garbage allowed beyond n_samples); n_samples (B) ints, tempo (B) factors in [0.5, 2], gain (B) in dB —
    host values; the kernel is given G = float32(10 ** (gain / 20)).
    Returns (out (B, max n_out) fp32 GPU, exact zeros beyond each n_out; n_out (B) int32 GPU; offsets (B, Kmax) int32 GPU: the search
    result d_k of every segment, 0 beyond an utterance's own segments).  The host-side lengths are `tempo_out_samples(n, tempo)`."""
    _chk_f32(audio)
    assert audio.dim() == 2 and audio.stride(1) == 1
    lib = _lib.load()
    B, dev = audio.size(0), audio.device
    n_host, f_host, g_db = _host_array(n_samples), _host_array(tempo, np.float64), _host_array(gain, np.float64)
    assert n_host.shape == f_host.shape == g_db.shape == (B,), f"n_samples, tempo and gain: one value per utterance ({B})"
    assert B == 0 or int(n_host.max()) <= audio.size(1), "n_samples exceeds the batch's row length"
    n_host = n_host.astype(np.int32)
    g_host = np.ascontiguousarray(np.float32(10.0 ** (g_db / 20.0)))
    S, _, O = tempo_sizes(sample_rate, segment_ms, search_ms, overlap_ms)
    n_out = [tempo_out_samples(n, f) for n, f in zip(n_host.tolist(), f_host.tolist())]
    ld_out = max(max(n_out), 1)
    ld_off = max(-(-max(n_out) // (S - O)), 1)
    out = torch.empty((B, ld_out), dtype=torch.float32, device=dev)
    n_out_dev = torch.empty(B, dtype=torch.int32, device=dev)
    offsets = torch.empty((B, ld_off), dtype=torch.int32, device=dev)
    wsb = lib.ds2_tempo_workspace_bytes(B)
    ws = _ws(wsb, dev)
    _lib.check(lib.ds2_tempo_gain_f32(audio.data_ptr(), audio.stride(0), n_host.ctypes.data, f_host.ctypes.data, g_host.ctypes.data, B,
                                      int(sample_rate), float(segment_ms), float(search_ms), float(overlap_ms), out.data_ptr(), ld_out,
                                      n_out_dev.data_ptr(), offsets.data_ptr(), ld_off, ws.data_ptr(), wsb, _stream()), "ds2_tempo_gain_f32")
    return out, n_out_dev, offsets


WAVE_ALIGN = 8                     # every utterance of a packed waveform buffer starts at a multiple of this many ELEMENTS: 128-bit loads
WAVE_MAX_ELEMS = 2 ** 31 - 1       # offsets are int64 on the host and int32 on the device (asr_amd.data lays batches out by these two)


def _packed_description(who, packed, offsets, lengths, src_index, rates=None):
    """The checks that wave_unpack and wave_resample share: the packed buffer and its host description -> (offsets, lengths, src_index as
    (B) int64 arrays, B, the buffer's elements).  rates: wave_resample's, a list that is counted with the others.  The lengths' own
    bounds are the caller's: they differ."""
    if packed.dtype not in (torch.int16, torch.float32) or not packed.is_cuda or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError(f"{who}: packed must be a contiguous 1-D int16 or fp32 GPU tensor")
    off, ln = _host_array(offsets).reshape(-1), _host_array(lengths).reshape(-1)
    B, total = int(ln.size), int(packed.numel())
    src = np.arange(B, dtype=np.int64) if src_index is None else _host_array(src_index).reshape(-1)
    counts = [("offsets", off.size), ("lengths", B)] + ([] if rates is None else [("rates", len(rates))])
    if B == 0 or any(n != B for _, n in counts) or src.size != B:
        raise ValueError(f"{who}: " + ", ".join(f"{k} ({n})" for k, n in counts) + f" and src_index ({src.size}): one value per utterance, "
                         "at least one")
    if total % WAVE_ALIGN or total > WAVE_MAX_ELEMS:
        raise ValueError(f"{who}: packed holds {total} elements: a multiple of {WAVE_ALIGN}, at most 2^31 - 1")
    if (off < 0).any() or (off % WAVE_ALIGN).any():
        raise ValueError(f"{who}: every offset is a non-negative multiple of {WAVE_ALIGN} elements, got {off.tolist()}")
    if (off + (ln + WAVE_ALIGN - 1) // WAVE_ALIGN * WAVE_ALIGN > total).any():
        raise ValueError(f"{who}: an utterance (rounded up to {WAVE_ALIGN} elements) ends beyond the {total} packed elements")
    if (src < 0).any() or (src >= B).any():
        raise ValueError(f"{who}: src_index outside [0, {B})")
    return off, ln, src, B, total


def _upload_i32(dev, rows, wide=None):
    """Per-utterance host integers for a kernel: rows (B values each) -> one (len(rows), B) int32 image on dev, from pinned memory with
    one asynchronous copy.  wide: a (B) int64 array that travels whole, as int32 pairs, in two more rows."""
    img = np.stack([np.asarray(r, dtype=np.int64) for r in rows]).astype(np.int32)
    if wide is not None:
        img = np.concatenate([img, wide.view(np.int32).reshape(2, -1)])
    return torch.from_numpy(img).pin_memory().to(dev, non_blocking=True)


def wave_unpack(packed: Tensor, offsets, lengths, src_index=None, n_max: Optional[int] = None) -> Tensor:
    """A packed ragged waveform buffer -> the zero-padded (B, n_max) fp32 batch of the front-end (ds2_wave_unpack_f32, contract in
    include/ds2hip.h).  packed: 1-D int16 (raw PCM, scaled by 2^-15: exact) or fp32 GPU tensor, a multiple of 8 elements long; offsets,
    lengths, src_index: (B) HOST integers — utterance u is packed[offsets[u] : offsets[u] + lengths[u]], row b of the result is utterance
    src_index[b] (default: b); n_max defaults to max(lengths).  The description is checked here, on the host (ValueError: an offset that
    is negative or not a multiple of 8, a length below 0 or above n_max, an utterance whose 8-aligned end passes the buffer, an index outside
    [0, B)), then uploaded from pinned memory with one asynchronous copy: the call does not block the host."""
    off, ln, src, B, total = _packed_description("wave_unpack", packed, offsets, lengths, src_index)
    if n_max is None:
        n_max = int(ln.max())
    n_max = int(n_max)
    if (ln < 0).any() or (ln > n_max).any():
        raise ValueError(f"wave_unpack: lengths lie in [0, n_max = {n_max}], got {ln.tolist()}")
    dev = packed.device
    if n_max == 0:
        return torch.zeros((B, 0), dtype=torch.float32, device=dev)
    meta = _upload_i32(dev, (off, ln, src))
    out = torch.empty((B, n_max), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ds2_wave_unpack_f32(packed.data_ptr() if total else None, total, 0 if packed.dtype == torch.int16 else 1,
                                               meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), B, n_max, out.data_ptr(),
                                               out.stride(0), _stream()), "ds2_wave_unpack_f32")
    return out


RESAMPLE_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA = 32, 0.945, 9.0
RESAMPLE_MAX_RATIO = 8             # fs / ft and ft / fs
RESAMPLE_MAX_TAPS = 2 ** 18        # L * P of one rate pair (1 MiB of fp32)
RESAMPLE_MAX_TABLE = 2 ** 22       # the concatenated tables of one call (the C ABI's limit)

_TAPS_CACHE = {}
_TAPS_DEVICE_CACHE = {}


def resample_ratio(fs: int, ft: int, zeros: int = RESAMPLE_ZEROS, rolloff: float = RESAMPLE_ROLLOFF) -> Tuple[int, int, int]:
    """(L, M, J) of a rate pair: L = ft / gcd, M = fs / gcd, J = ceil(zeros / (rolloff * min(1, L / M))) taps per side.  ValueError for a
    pair outside what the resampler supports: a ratio outside [1/8, 8] or a table of more than RESAMPLE_MAX_TAPS taps."""
    if not (_is_int(fs, 1) and _is_int(ft, 1)):
        raise ValueError(f"resample: sample rates are positive integers, got {fs!r} -> {ft!r}")
    fs, ft = int(fs), int(ft)
    g = math.gcd(fs, ft)
    L, M = ft // g, fs // g
    if M > RESAMPLE_MAX_RATIO * L or L > RESAMPLE_MAX_RATIO * M:
        raise ValueError(f"resample: {fs} Hz -> {ft} Hz is outside the supported ratios [1/{RESAMPLE_MAX_RATIO}, {RESAMPLE_MAX_RATIO}]")
    if L == 1 and M == 1:
        return 1, 1, 0
    J = int(math.ceil(zeros / (rolloff * min(1.0, L / M))))
    if L * 2 * J > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resample: {fs} Hz -> {ft} Hz needs a table of {L} x {2 * J} taps, more than the {RESAMPLE_MAX_TAPS} supported "
                         "(rates with a large common divisor, such as 48000, 44100, 22050 or 8000 Hz against 16000 Hz, are)")
    return L, M, J


def resample_taps(fs: int, ft: int, zeros: int = RESAMPLE_ZEROS, rolloff: float = RESAMPLE_ROLLOFF, beta: float = RESAMPLE_BETA):
    """The (L, P = 2 J) fp32 polyphase table of the contract in include/ds2hip.h (a host numpy array, cached per argument tuple):
    tab[p][j] = fp32(s sinc(s tau) w(tau)), tau = p / L + J - 1 - j, s = rolloff min(1, L / M), w the Kaiser window of half-width
    zeros / s — computed in fp64, rounded once.  fs == ft has no table: ValueError."""
    key = (int(fs), int(ft), int(zeros), float(rolloff), float(beta))
    if key not in _TAPS_CACHE:
        L, M, J = resample_ratio(fs, ft, zeros, rolloff)
        if L == 1 and M == 1:
            raise ValueError("resample_taps: equal rates are copied, there is no table")
        s = rolloff * min(1.0, L / M)
        tau = np.arange(L, dtype=np.float64)[:, None] / L + (J - 1 - np.arange(2 * J, dtype=np.float64))[None, :]
        r = tau * s / zeros
        w = np.where(np.abs(r) <= 1.0, np.i0(beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / np.i0(beta), 0.0)
        tab = np.ascontiguousarray((s * np.sinc(s * tau) * w).astype(np.float32))
        tab.setflags(write=False)
        _TAPS_CACHE[key] = tab
    return _TAPS_CACHE[key]


def resample_out_samples(n: int, fs: int, ft: int) -> int:
    """ceil(n L / M): the length of an n-sample utterance at fs after conversion to ft (ds2_resample_out_samples; a host function)."""
    g = math.gcd(int(fs), int(ft))
    n_out = _lib.load().ds2_resample_out_samples(int(n), int(ft) // g, int(fs) // g)
    if n_out < 0:
        raise _lib.DS2LibraryError(f"resample_out_samples: n = {n} (0 .. 2^31), {fs} Hz -> {ft} Hz outside the contract")
    return int(n_out)


def _resample_tables(pairs, device):
    """(table buffer, {pair: base}) on `device` covering the rate pairs of one call.  ONE buffer per device holds the tables of every
    pair seen so far, in order of first use (so it is bounded by RESAMPLE_MAX_TABLE taps = 16 MiB however the rates mix in the batches);
    a new pair makes a longer buffer, the old one stays alive for the launches that hold it.  No pair: (None, {})."""
    key = str(device)
    buf, bases = _TAPS_DEVICE_CACHE.get(key, (None, {}))
    new = [p for p in pairs if p not in bases]
    if new:
        order = list(bases) + new
        tabs = [resample_taps(fs, ft) for fs, ft in order]
        starts = np.concatenate([[0], np.cumsum([t.size for t in tabs])]).astype(np.int64)
        if int(starts[-1]) > RESAMPLE_MAX_TABLE:
            raise ValueError(f"wave_resample: the tables of the {len(order)} rate pairs seen on {key} hold {int(starts[-1])} taps, "
                             f"at most {RESAMPLE_MAX_TABLE}")
        buf = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tabs])).to(device)
        bases = {p: int(b) for p, b in zip(order, starts[:-1])}
        _TAPS_DEVICE_CACHE[key] = (buf, bases)
    return buf, bases


def wave_resample(packed: Tensor, offsets, lengths, rates, src_index=None, target_rate: int = 16000, n_out_max: Optional[int] = None,
                  n_out=None):
    """`wave_unpack` with a sample-rate conversion in it (ds2_wave_resample_f32, contract in include/ds2hip.h): utterance u, `lengths[u]`
    samples at `rates[u]` Hz, becomes ceil(n L / M) samples at `target_rate` by Kaiser-windowed sinc interpolation; an utterance already
    at the target rate is copied bit for bit.  packed, offsets, lengths, src_index as in `wave_unpack`; rates: (B) HOST integers.
    The description is checked here, on the host (ValueError, wave_unpack's cases plus an unsupported rate pair), the tables are built
    once per rate pair and device, everything is sized on the host and uploaded from pinned memory with one asynchronous copy: nothing is
    copied back.  `n_out`: the resampled lengths when the caller has them already (resample_out_samples per utterance; the loader has).
    Returns (batch (B, n_out_max) fp32 GPU in src_index order, n_out: a list of B ints in UTTERANCE order)."""
    fs = _host_array(rates).reshape(-1).tolist()
    off, ln, src, B, total = _packed_description("wave_resample", packed, offsets, lengths, src_index, fs)
    if (ln < 0).any():
        raise ValueError(f"wave_resample: negative length in {ln.tolist()}")
    target_rate = int(target_rate)
    lmj = {r: resample_ratio(r, target_rate) for r in sorted(set(fs))}
    if n_out is None:
        n_out = [resample_out_samples(n, r, target_rate) for n, r in zip(ln.tolist(), fs)]
    n_out = [int(v) for v in n_out]
    if len(n_out) != B or any(v != -(-n * lmj[r][0] // lmj[r][1]) for v, n, r in zip(n_out, ln.tolist(), fs)):
        raise ValueError("wave_resample: n_out must be ceil(n L / M) per utterance")
    if n_out_max is None:
        n_out_max = max(n_out)
    n_out_max = int(n_out_max)
    if max(n_out) > n_out_max or n_out_max > 2 ** 30:
        raise ValueError(f"wave_resample: resampled lengths lie in [0, n_out_max = {n_out_max}] and n_out_max <= 2^30, got {n_out}")
    dev = packed.device
    if n_out_max == 0:
        return torch.zeros((B, 0), dtype=torch.float32, device=dev), n_out
    tab, bases = _resample_tables(tuple((r, target_rate) for r in lmj if lmj[r][:2] != (1, 1)), dev)
    rows = [off, ln, src, [lmj[r][0] for r in fs], [lmj[r][1] for r in fs], [lmj[r][2] for r in fs],
            [bases.get((r, target_rate), 0) for r in fs]]
    meta = _upload_i32(dev, rows)
    out = torch.empty((B, n_out_max), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ds2_wave_resample_f32(packed.data_ptr() if total else None, total, 0 if packed.dtype == torch.int16 else 1,
                                                 *[meta[i].data_ptr() for i in range(7)], tab.data_ptr() if tab is not None else None,
                                                 tab.numel() if tab is not None else 0, B, n_out_max, out.data_ptr(), out.stride(0),
                                                 _stream()), "ds2_wave_resample_f32")
    return out, n_out


def reverb_max_taps() -> int:
    """The longest impulse response ops.reverb takes (ds2_reverb_max_taps; a host function, no GPU needed)."""
    return int(_lib.load().ds2_reverb_max_taps())


def reverb(audio: Tensor, n_samples, rir: Optional[Tensor], rir_base, rir_taps, n_max: Optional[int] = None) -> Tensor:
    """Reverberation of a waveform batch (ds2_reverb_f32, contract in include/ds2hip.h): row b becomes the truncated causal convolution
    y[i] = sum_{k <= min(i, P - 1)} h[k] x[i - k], i < n_b, of its n_b samples with the P_b = rir_taps[b] taps at rir[rir_base[b]:]; the tail
    beyond n_b is dropped, so every utterance keeps its length.  rir_taps[b] == 0 copies the row bit for bit.
    audio (B, L) fp32 GPU rows (garbage allowed beyond n_samples); rir: ONE 1-D fp32 GPU bank of concatenated responses (None: no bank,
    every rir_taps is then 0); n_samples, rir_base, rir_taps: (B) HOST integers.  The description is checked here, on the host (ValueError:
    a length outside [0, n_max], taps outside [0, reverb_max_taps()], a slice outside the bank), then uploaded from pinned memory as one
    int32 image with one asynchronous copy.  Returns a new (B, n_max) fp32 GPU tensor, exact zeros beyond each n_b; n_max defaults to
    max(n_samples)."""
    if audio.dtype != torch.float32 or not audio.is_cuda or audio.dim() != 2 or audio.stride(1) != 1 or audio.size(0) == 0:
        raise ValueError("reverb: audio must be a (B >= 1, L) fp32 GPU tensor with contiguous rows")
    if rir is not None and (rir.dtype != torch.float32 or not rir.is_cuda or rir.dim() != 1 or not rir.is_contiguous()):
        raise ValueError("reverb: rir must be a contiguous 1-D fp32 GPU tensor")
    B, dev = audio.size(0), audio.device
    n, base, taps = (_host_array(v).reshape(-1) for v in (n_samples, rir_base, rir_taps))
    if n.size != B or base.size != B or taps.size != B:
        raise ValueError(f"reverb: n_samples ({n.size}), rir_base ({base.size}) and rir_taps ({taps.size}): one value per row ({B})")
    if n_max is None:
        n_max = int(n.max())
    n_max = int(n_max)
    elems = 0 if rir is None else int(rir.numel())
    if (n < 0).any() or (n > n_max).any() or n_max > audio.size(1) or n_max > 2 ** 30:
        raise ValueError(f"reverb: lengths lie in [0, n_max = {n_max}], n_max within the rows ({audio.size(1)}) and 2^30, got {n.tolist()}")
    if (taps < 0).any() or (taps > reverb_max_taps()).any():
        raise ValueError(f"reverb: taps lie in [0, {reverb_max_taps()}], got {taps.tolist()}")
    if elems > 2 ** 31 - 1 or (base < 0).any() or (base + taps > elems).any():
        raise ValueError(f"reverb: an impulse response lies outside the bank of {elems} taps (at most 2^31 - 1)")
    if n_max == 0:
        return torch.zeros((B, 0), dtype=torch.float32, device=dev)
    meta = _upload_i32(dev, (n, taps), wide=base)                # rows: n, taps, and base's int32 pairs in two
    out = torch.empty((B, n_max), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ds2_reverb_f32(audio.data_ptr(), audio.stride(0), meta[0].data_ptr(), rir.data_ptr() if elems else None, elems,
                                          meta[2].data_ptr(), meta[1].data_ptr(), B, n_max, out.data_ptr(), out.stride(0),
                                          _stream()), "ds2_reverb_f32")
    return out


# ------------------------------------------------------------------------------------------------
# optimizer
# ------------------------------------------------------------------------------------------------
def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
          weight_decay: float = 1e-5, grad_scale: float = 1.0, apply_flag: Optional[Tensor] = None):
    """apply_flag: optional int32 GPU tensor read by the kernel when it runs (0 = leave p, m, v untouched): step_gate()."""
    _chk_f32(p, g, m, v)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert apply_flag is None or (apply_flag.dtype == torch.int32 and apply_flag.is_cuda)
    _lib.check(_lib.load().ds2_adamw_gated_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, betas[0], betas[1],
                                               eps, weight_decay, int(step), grad_scale, _ptr(apply_flag), _stream()), "ds2_adamw_gated_f32")


def step_gate(loss: Tensor) -> Tensor:
    """int32 GPU tensor [1]: 1 if, when the stream gets there, `loss` (0-d / 1-element fp32 GPU tensor) is finite and non-negative and no
    persistent recurrence launch has recorded starvation — the device-side form of check_loss + rnn_persistent_check."""
    _chk_f32(loss)
    flag = torch.empty(1, dtype=torch.int32, device=loss.device)
    _lib.check(_lib.load().ds2_rnn_step_gate(_ctxp(loss.device), loss.data_ptr(), flag.data_ptr(), _stream()), "ds2_rnn_step_gate")
    return flag
