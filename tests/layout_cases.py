"""Shape lists, input builders, plain references and checkers for the layout, cast and step-scalar kernels — TEST INFRASTRUCTURE ONLY,
shared by tests/test_gpu_layout.py and tests/test_gpu_step_scalars.py (the GPU comparisons) and tests/test_cpu_layout_refs.py (which runs
every checker on a float32 numpy restatement of the kernel's own statement order, and on planted mistakes, without a GPU).

numpy / torch on the CPU only; nothing here imports asr_amd.

Conventions
  * bf16 data travels as torch.bfloat16 (references) or as numpy uint16 bit patterns (restatements); `bits()` maps either to unsigned bits.
  * `assert_same_bits` is THE comparison of every exact kernel: equal bit patterns everywhere, except where the reference is a NaN, where
    the other side only has to be a NaN too (the payload is not part of any contract here).
  * U = 2^-24 is the unit round-off of fp32 (half an ulp of a value in [1, 2)); a correctly rounded operation has relative error <= U, an
    operation documented with an error of 1 ulp has relative error <= 2 U.
"""
from __future__ import annotations

import numpy as np
import torch

import det

U = 2.0 ** -24
TINY = 2.0 ** -149            # the smallest fp32 subnormal: an operation whose result underflows is off by at most half of it


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------------------
# bits and the exact comparison
# ------------------------------------------------------------------------------------------------------------------------------
def bits(a) -> np.ndarray:
    """unsigned bit patterns of a torch (bf16 / fp32) tensor or a numpy (uint16 / uint32 / float32) array, same shape"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        if a.dtype == torch.bfloat16:
            return a.view(torch.int16).numpy().view(np.uint16)
        assert a.dtype == torch.float32, a.dtype
        return a.view(torch.int32).numpy().view(np.uint32)
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    assert a.dtype in (np.uint16, np.uint32), a.dtype
    return a


def _is_nan_bits(b: np.ndarray) -> np.ndarray:
    if b.dtype == np.uint16:
        return (b & np.uint16(0x7FFF)) > np.uint16(0x7F80)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def assert_same_bits(got, ref, what: str = ""):
    """got == ref bit for bit; at the reference's NaNs got must be a NaN (any payload)"""
    gb, rb = bits(got), bits(ref)
    assert gb.shape == rb.shape and gb.dtype == rb.dtype, (what, gb.shape, rb.shape, gb.dtype, rb.dtype)
    ok = np.where(_is_nan_bits(rb), _is_nan_bits(gb), gb == rb)
    if not ok.all():
        bad = np.argwhere(~ok)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} elements differ, first at {first}: got {int(gb[first]):#x} want {int(rb[first]):#x}")


# ------------------------------------------------------------------------------------------------------------------------------
# special values (every cast test)
# ------------------------------------------------------------------------------------------------------------------------------
SPECIAL_BITS = [
    0x3F808000,   # tie above an even upper half (0x3F80): rounds DOWN to 0x3F80            } one of the ties sits on the first element,
    0x00000000, 0x80000000,                       # +0, -0
    0x7F800000, 0xFF800000, 0x7FC00000,           # +inf, -inf, quiet NaN
    0x7F7FFFFF,                                   # the largest finite float: rounds to +inf under round-to-nearest-even
    0x3F818000,   # tie above an odd upper half (0x3F81): rounds UP to 0x3F82
    0xBF808000, 0xBF818000,                       # the same two ties, negative
    0x3F807FFF, 0x3F808001,                       # just below a tie (-> 0x3F80), just above (-> 0x3F81)
    0x00000001, 0x007FFFFF, 0x80012345,           # fp32 subnormals: the smallest, the largest (rounds up to the normal 0x0080), a negative one
    0x00408000, 0x00018000, 0x00008000,           # subnormal ties: even upper half (-> 0x0040), odd (-> 0x0002), below the smallest bf16 (-> +0)
    0xC0490FDB,   # an ordinary value (-pi)
    0xBF818000,   # ... and a tie sits on the last element
]
_NONFINITE = {0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF}


def special_f32(shape, seed: int, finite: bool = False) -> np.ndarray:
    """det.unitvar data with SPECIAL_BITS scattered over it at evenly spaced flat positions, the first and the last element included (so:
    the first element of the first row and the last element of the last row of a 2-D case).  A tensor smaller than the list holds a seed-
    dependent run of the list.  finite: leave out +-inf, NaN and the float that rounds to inf (the column-sum inputs)."""
    x = det.unitvar(tuple(shape), seed).reshape(-1).copy()
    sp = [b for b in SPECIAL_BITS if not (finite and b in _NONFINITE)]
    n, k = x.size, len(sp)
    xb = x.view(np.uint32)
    if n >= k:
        pos = [(i * (n - 1)) // (k - 1) for i in range(k)]
        for p_, b in zip(pos, sp):
            xb[p_] = b
    else:
        for i in range(n):
            xb[i] = sp[(i + seed) % k]
    return x.reshape(shape)


def subnormal_mask(x: np.ndarray) -> np.ndarray:
    b = bits(np.asarray(x, np.float32))
    return ((b & np.uint32(0x7F800000)) == 0) & ((b & np.uint32(0x007FFFFF)) != 0)


def unaligned_view(shape2d, seed: int, finite: bool = False):
    """(big, col0): an (R, W) tensor with ODD pitch W >= C + 2 and the column offset 1: big[:, 1:1+C] has a pitch that is no multiple of 4 and
    a base that is not 16-byte aligned (the kernels' vec == 0 path), and real data on either side of it."""
    R, Cc = shape2d
    W = Cc + 3 - (Cc % 2)          # C + 2 or C + 3, odd
    assert W % 2 == 1
    return special_f32((R, W), seed, finite), 1


# ------------------------------------------------------------------------------------------------------------------------------
# bf16 rounding: the reference is torch's x.bfloat16(); the numpy form below is its restatement (and the carrier of planted mistakes)
# ------------------------------------------------------------------------------------------------------------------------------
def ref_bf16(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, np.float32)).bfloat16()


def np_bf16_bits(x, mode: str = "rne") -> np.ndarray:
    """uint16 bf16 bit patterns of float32 x.  mode: 'rne' round-to-nearest-even (the contract) | 'trunc' | 'away' (ties away from zero)."""
    b = bits(np.asarray(x, np.float32)).astype(np.uint64)
    if mode == "rne":
        r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    elif mode == "away":
        r = (b + np.uint64(0x8000)) >> np.uint64(16)
    else:
        assert mode == "trunc"
        r = b >> np.uint64(16)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, np.uint64(0x7FC0), r).astype(np.uint16)


def np_bf16_to_f32(h: np.ndarray) -> np.ndarray:
    return (h.astype(np.uint32) << np.uint32(16)).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# cast_bf16 / cast_transpose_bf16 / cast_bf16_both / transpose_bf16
# ------------------------------------------------------------------------------------------------------------------------------
CAST_R = [1, 3, 64, 65]
CAST_C = [1, 7, 8, 9, 63, 64, 65, 130]
CAST_BIG = (1030, 8196)            # R * ld / 4 = 1030 * 8200 / 4 = 2 111 500 > 8192 * 256: the stride loop takes a second trip; C % 8 == 4
T_SHAPES = [(1, 1), (7, 9), (63, 65), (64, 64), (65, 63), (129, 70), (200, 8)]
COLSUM_ROWS = 64                   # rows one fp32 partial sum covers in cast_transpose_bf16_kernel / transpose_bf16_kernel (one 64-row tile)


def cast_lds(Cc: int):
    return [None, pad8(Cc) + 8, pad8(Cc) + 64]


def both_ld_r(Cc: int):
    """ld_r values of cast_bf16_both: the default, and pad8(C) + 8 where the entry still accepts it (ld_r <= the next multiple of 64)"""
    wide = pad8(Cc) + 8
    return [None] + ([wide] if wide <= -(-Cc // 64) * 64 else [])


def ref_cast(x, ld=None) -> torch.Tensor:
    """(R, C) fp32 -> (R, ld or pad8(C)) bf16, pad columns zero"""
    x = torch.as_tensor(np.asarray(x, np.float32))
    R, Cc = x.shape
    out = torch.zeros(R, pad8(Cc) if ld is None else ld, dtype=torch.bfloat16)
    out[:, :Cc] = x.bfloat16()
    return out


def ref_cast_t(x) -> torch.Tensor:
    """(R, C) fp32 or bf16 -> (C, pad8(R)) bf16 = x^T, pad columns zero"""
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float32))
    R, Cc = x.shape
    out = torch.zeros(Cc, pad8(R), dtype=torch.bfloat16)
    out[:, :R] = x.bfloat16().t()
    return out


def np_cast(big: np.ndarray, col0: int, Cc: int, ld=None, mode="rne", pad="zero") -> np.ndarray:
    """cast_bf16_kernel's statement on the view big[:, col0:col0+C], as uint16 bits.  pad='input': the planted mistake "pad columns left at the
    input's value" (the columns of big behind the view, as far as big has them)."""
    R = big.shape[0]
    ld = pad8(Cc) if ld is None else ld
    out = np.zeros((R, ld), np.uint16)
    out[:, :Cc] = np_bf16_bits(big[:, col0:col0 + Cc], mode)
    if pad == "input":
        w = min(ld, big.shape[1] - col0)
        out[:, Cc:w] = np_bf16_bits(big[:, col0 + Cc:col0 + w], mode)
    return out


def np_cast_t(big: np.ndarray, col0: int, Cc: int, mode="rne") -> np.ndarray:
    R = big.shape[0]
    out = np.zeros((Cc, pad8(R)), np.uint16)
    out[:, :R] = np_bf16_bits(big[:, col0:col0 + Cc], mode).T
    return out


def np_colsum_tiles(x: np.ndarray) -> np.ndarray:
    """the kernels' column sums: per 64-row tile a sequential fp32 sum from 0.f, the tiles' partials added in fp64, stored as fp32"""
    x = np.asarray(x, np.float32)
    R, Cc = x.shape
    tot = np.zeros(Cc, np.float64)
    for r0 in range(0, R, COLSUM_ROWS):
        s = np.zeros(Cc, np.float32)
        for r in range(r0, min(R, r0 + COLSUM_ROWS)):
            s = (s + x[r]).astype(np.float32)
        tot += s.astype(np.float64)
    return tot.astype(np.float32)


def check_colsum(got, x, what: str = ""):
    """Column sums of x (the SOURCE values: fp32, or bf16 widened) against their fp64 sums:  |got - ref| <= n * 2^-24 * sum_r |x[r, c]|,
    n = COLSUM_ROWS = 64: the kernels sum one 64-row tile sequentially in fp32 — 63 rounded additions behind an exact first one — the
    tiles' partials are added in fp64 (ds2i_col_finalize_sums) and the result is rounded to fp32 once: 64 roundings, each at most
    2^-24 of a partial that is itself at most sum |x| (first order, the textbook bound for a length-n sum; nothing here is measured)."""
    x64 = np.asarray(x, np.float64)
    got = np.asarray(got, np.float64).reshape(-1)
    ref = x64.sum(0)
    bound = COLSUM_ROWS * U * np.abs(x64).sum(0)
    bad = ~(np.abs(got - ref) <= bound)
    assert got.shape == ref.shape and not bad.any(), f"{what}: column sums off at {np.flatnonzero(bad)[:5]}: worst {np.abs(got - ref).max():.3e}"


# ------------------------------------------------------------------------------------------------------------------------------
# split_bf16
# ------------------------------------------------------------------------------------------------------------------------------
SPLIT_R = [1, 5, 64, 70]
SPLIT_C = [1, 7, 8, 9, 64, 65]
SPLIT_ORDERS = {0: "hhl", 1: "hlh", 2: "hl"}     # ops.split_bf16's docstring: 0 = [hi | hi | lo], 1 = [hi | lo | hi], 2 = [hi | lo]


def ref_split(x, order: int, pad_rows: int = 0) -> torch.Tensor:
    """hi = bf16(x), lo = bf16(x - float(hi)) (the subtraction is exact in fp32), blocks pad8(C) wide in the docstring's order, pads zero"""
    x = torch.as_tensor(np.asarray(x, np.float32))
    R, Cc = x.shape
    Cp = pad8(Cc)
    Rp = -(-R // pad_rows) * pad_rows if pad_rows else R
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    blocks = SPLIT_ORDERS[order]
    out = torch.zeros(Rp, len(blocks) * Cp, dtype=torch.bfloat16)
    for i, ch in enumerate(blocks):
        out[:R, i * Cp:i * Cp + Cc] = hi if ch == "h" else lo
    return out


def np_split(x: np.ndarray, order: int, pad_rows: int = 0, lo_from_x: bool = False, swap01: bool = False) -> np.ndarray:
    """split_bf16_kernel's statement (uint16 bits).  Planted: lo_from_x (lo = bf16(x)), swap01 (orders 0 and 1 exchanged)."""
    x = np.asarray(x, np.float32)
    R, Cc = x.shape
    Cp = pad8(Cc)
    Rp = -(-R // pad_rows) * pad_rows if pad_rows else R
    if swap01 and order in (0, 1):
        order = 1 - order
    hi = np_bf16_bits(x)
    with np.errstate(invalid="ignore"):
        lo = np_bf16_bits(x if lo_from_x else (x - np_bf16_to_f32(hi)).astype(np.float32))
    blocks = SPLIT_ORDERS[order]
    out = np.zeros((Rp, len(blocks) * Cp), np.uint16)
    for i, ch in enumerate(blocks):
        out[:R, i * Cp:i * Cp + Cc] = hi if ch == "h" else lo
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# widen / residual / sum3 / scale
# ------------------------------------------------------------------------------------------------------------------------------
WIDEN_N = [8, 2040, 8 * (8192 * 256) + 8]                  # the last: one 8-element group past the 8192-block grid's first trip
FLAT_N = [1, 2, 3, 4, 5, 1023, 8192 * 256 * 4 + 3]         # bf16_residual / sum3_: n < 4, the n % 4 tail, second trip of the stride loop
SCALE_N = [1, 255, 256, 257, 4096 * 256 + 1]


def ref_residual(x) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(x, np.float32))
    return x - x.bfloat16().float()


# ------------------------------------------------------------------------------------------------------------------------------
# transposes, nhwc, padcast
# ------------------------------------------------------------------------------------------------------------------------------
BFT_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 63, 65), (2, 64, 64), (2, 65, 63), (1, 161, 130), (2, 1312, 7)]
BATCHED_SHAPES = [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 33, 31), (1, 100, 7)]
NHWC_SHAPES = [(1, 32, 1, 1), (2, 32, 3, 5), (1, 32, 2, 63), (1, 32, 2, 64), (1, 32, 2, 65), (3, 32, 2, 130)]
PADCAST_BCD = [(1, 1, 1), (2, 32, 3)]
PADCAST_T = [1, 7, 8, 9, 63, 64, 65, 130]
PAD_LEAD = 8


def padded_pitch(T: int) -> int:
    """ds2_conv_padded_pitch restated: eight leading zeros, T values, at least eight trailing zeros, rounded up to a multiple of 8"""
    return (T + 16 + 7) // 8 * 8


def ref_nhwc(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, np.float32)).permute(0, 2, 3, 1).contiguous().bfloat16()


def ref_padcast(x) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(x, np.float32))
    T = x.shape[-1]
    out = torch.zeros(*x.shape[:-1], padded_pitch(T), dtype=torch.bfloat16)
    out[..., PAD_LEAD:PAD_LEAD + T] = x.bfloat16()      # rounded once
    return out


def np_padcast(x: np.ndarray, lead: int = PAD_LEAD, clear_tail: bool = True, fill: int = 0x7FC0) -> np.ndarray:
    """padcast_kernel's statement (uint16 bits).  Planted: lead = 7; clear_tail = False leaves the tail at `fill` (whatever the buffer held)."""
    x = np.asarray(x, np.float32)
    T = x.shape[-1]
    out = np.zeros(x.shape[:-1] + (padded_pitch(T),), np.uint16)
    if not clear_tail:
        out[..., lead + T:] = fill
    out[..., lead:lead + T] = np_bf16_bits(x)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# softmax_rows
# ------------------------------------------------------------------------------------------------------------------------------
SOFTMAX_ROWS = [1, 3, 4, 5, 77]
SOFTMAX_C = [1, 2, 29, 63, 64, 65, 80, 200]
SOFTMAX_SHIFTS = [0.0, 80.0, -80.0]
SOFTMAX_K = 17


def softmax_logits(rows: int, Cc: int, kind: str = "plain") -> np.ndarray:
    """unit-variance logits x 3.
    kind 'grid'   : the same, rounded to multiples of 2^-10, so that adding +-80 is exact in fp32 and a shifted row has EXACTLY the
                    probabilities of the unshifted one (one fp64 reference serves all three shifts);
         'neginf' : -inf scattered over every row (every third entry from a row-dependent start) — and, where C > 64, the last row has -inf
                    in ALL of its first 64 columns (its maximum lies behind them);
         'single' : every row keeps ONE finite entry (at a row-dependent column), all others are -inf."""
    x = (det.unitvar((rows, Cc), 500 + 7 * rows + Cc) * np.float32(3.0)).astype(np.float32)
    if kind == "grid":
        x = (np.round(x * 1024.0) / 1024.0).astype(np.float32)
    elif kind == "neginf":
        for r in range(rows):
            x[r, (r % 3)::3] = -np.inf
            if not np.isfinite(x[r]).any():
                x[r, (r * 5) % Cc] = np.float32(0.25 * r - 1.0)
        if Cc > 64:
            x[rows - 1, :64] = -np.inf
            x[rows - 1, 64] = np.float32(1.5)
    elif kind == "single":
        keep = [(r * 37 + 11) % Cc for r in range(rows)]
        vals = x[np.arange(rows), keep].copy()
        x[:] = -np.inf
        x[np.arange(rows), keep] = vals
    else:
        assert kind == "plain"
    return x


def ref_softmax(x: np.ndarray) -> np.ndarray:
    """fp64 softmax of the fp32 inputs"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        d = x - x.max(1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(1, keepdims=True)


def _exp_f32(d: np.ndarray) -> np.ndarray:
    """expf on float32 arguments, correctly rounded (through fp64): inside any 1-ulp expf"""
    return np.exp(d.astype(np.float64)).astype(np.float32)


def np_softmax_kernel(x: np.ndarray, max_cols=None, sum_cols=None) -> np.ndarray:
    """softmax_rows_kernel in float32, statement by statement: per lane the running max over c = lane, lane + 64, ..; the xor-shuffle tree
    (offsets 32 .. 1); per lane the sequential sum of expf(x - m) from 0.f; the same tree; inv = 1.f / s; y = expf(x - m) * inv.
    Planted: max_cols / sum_cols = 64 (only the first 64 columns enter the maximum / the sum)."""
    x = np.asarray(x, np.float32)
    rows, Cc = x.shape
    lanes = np.arange(64)
    out = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(rows):
            p = x[r]
            m = np.full(64, -np.inf, np.float32)
            for c0 in range(0, Cc if max_cols is None else min(Cc, max_cols), 64):
                seg = p[c0:c0 + 64]
                m[:len(seg)] = np.fmax(m[:len(seg)], seg)
            for o in (32, 16, 8, 4, 2, 1):
                m = np.fmax(m, m[lanes ^ o])
            e = _exp_f32((p - m[0]).astype(np.float32))
            s = np.zeros(64, np.float32)
            for c0 in range(0, Cc if sum_cols is None else min(Cc, sum_cols), 64):
                seg = e[c0:c0 + 64]
                s[:len(seg)] = (s[:len(seg)] + seg).astype(np.float32)
            for o in (32, 16, 8, 4, 2, 1):
                s = (s + s[lanes ^ o]).astype(np.float32)
            inv = np.float32(1.0) / s[0]
            out[r] = (e * inv).astype(np.float32)
    return out


def check_softmax(got, x, ref=None, what: str = ""):
    """Per element  |got - ref| <= 2^-24 * (|x - max| + k + ceil(C/64)) * ref  against the fp64 softmax of the fp32 inputs, in units of
    U = 2^-24 relative to ref (first order):
      |x - max|      d = fl(x - max) is off by <= U |d|, which exp turns into a relative error of U |d|;
      ceil(C/64) + 6 the sum s: a lane adds ceil(C/64) terms to 0.f (the first addition exact), the shuffle tree adds six levels;
      k = 17 =  6    the tree's six levels (above),
              + 2    expf(d) of the numerator: HIP documents expf with a maximum error of 1 ulp (HIP math API, single precision), <= 2 U,
              + 2    expf of the sum's terms: the same 2 U on every term, hence on s,
              + 4    the subtraction round-off of the sum's terms, U |d_j| each: on s this is U * sum_j p_j |d_j| (p = the softmax itself,
                     d_max = 0); that expectation equals H(p) + log p_max, so for C <= 200 entries it is below 4 (the worst row has one entry
                     at 0 and C - 1 equal entries at -a: a t / (1 + t), t = (C - 1) e^-a, maximal 3.15 at a = 4.15 for C = 200),
              + 1    inv = 1.f / s: fp32 division is correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, <= U,
              + 1    the product expf(d) * inv, <= U,
              + 1    the second-order terms of the above (about (35 U)^2) and the fp64 reference's own error.
    An entry whose reference is 0 (a -inf logit) has bound 0: it must be exactly 0.  Every input of this file keeps x - max above -87, so no
    probability is subnormal in fp32 — except those zeros.
    Row sums (in fp64) lie within (C + 8) * 2^-24 of 1: the numerators are the very expf values that were summed, so what is left is s's
    accumulation (ceil(C/64) + 6 <= C + 6), the reciprocal and the product."""
    x64 = np.asarray(x, np.float64)
    got = np.asarray(got, np.float64)
    ref = ref_softmax(x64) if ref is None else ref
    rows, Cc = x64.shape
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(x64), np.abs(x64 - x64.max(1, keepdims=True)), 0.0)
    bound = U * (d + SOFTMAX_K + -(-Cc // 64)) * ref
    bad = ~(np.abs(got - ref) <= bound)                       # (a NaN in got is bad)
    assert got.shape == ref.shape and not bad.any(), \
        f"{what}: {int(bad.sum())} probabilities outside the bound, first at {tuple(np.argwhere(bad)[0])}: worst {np.nanmax(np.abs(got - ref) / np.maximum(bound, 1e-300)):.2f} x bound"
    rs = np.abs(got.sum(1) - 1.0)
    assert (rs <= (Cc + 8) * U).all(), f"{what}: row sum off by {rs.max():.3e}"


# ------------------------------------------------------------------------------------------------------------------------------
# ctc_batch_mean
# ------------------------------------------------------------------------------------------------------------------------------
BATCH_MEAN_B = [1, 3, 63, 64, 65, 257, 1000]


def batch_mean_nll(B: int) -> np.ndarray:
    return (np.abs(det.unitvar((B,), 60 + B)) * np.float32(300.0)).astype(np.float32)


def np_batch_mean_kernel(nll: np.ndarray) -> np.float32:
    """batch_mean_kernel in float32: lane-strided sums from 0.f, the xor-shuffle tree, one division by (float)B"""
    nll = np.asarray(nll, np.float32)
    lanes = np.arange(64)
    s = np.zeros(64, np.float32)
    for b0 in range(0, len(nll), 64):
        seg = nll[b0:b0 + 64]
        s[:len(seg)] = (s[:len(seg)] + seg).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[lanes ^ o]).astype(np.float32)
    return np.float32(s[0] / np.float32(len(nll)))


def check_batch_mean(got: float, nll: np.ndarray, what: str = ""):
    """|got - sum(nll)/B| <= B * 2^-24 * sum|nll| / B.  The kernel rounds at most ceil(B/64) - 1 (lane) + 6 (tree) + 1 (division) times, and never
    more than B times: with B < 64 only B lanes hold a non-zero value, adding a zero is exact, so at most B - 1 additions of the tree
    round, plus the division — B = 1 is exact.  Each rounding is at most 2^-24 of a partial that is at most sum|nll|."""
    n64 = np.asarray(nll, np.float64)
    B = len(n64)
    ref = n64.sum() / B
    bound = B * U * np.abs(n64).sum() / B
    assert abs(float(got) - ref) <= bound, f"{what}: B={B} got {float(got)!r} want {ref!r} (bound {bound:.3e})"


# ------------------------------------------------------------------------------------------------------------------------------
# adamw
# ------------------------------------------------------------------------------------------------------------------------------
ADAMW_N = [1, 2, 3, 4, 5, 1003, 4096 * 256 * 4 + 5]       # n < 4, the n % 4 tail, the second trip of the 4096-block stride loop
ADAMW_STEPS = [1, 2, 1000]
ADAMW_HYPER = {
    "trainer": dict(lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, grad_scale=1.0),
    "stressed": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.1, grad_scale=0.5),
}
ADAMW_C0 = 11


def adamw_state(n: int, seed: int = 0):
    """(p, g, m, v) float32, v >= 0, no inf / NaN.  By element index i (a seeded category each):
         category 0  g = 0 exactly, m = v = 0        : the update is exactly 0, p changes only by the decay factor
         category 1  g != 0, m = v = 0               : a first step
         category 2  m has g's sign, v ~ g^2         : no cancellation in m'
         category 3  m has the opposite sign of g    : m' = b1 m + (1 - b1) g cancels (|m| between 0.05 and 0.2 |g|, so b1 |m| ~ (1 - b1) |g|)
       |g| = 10^e with e uniform in [-20, 15], both signs; element 0 is category 0 and (n > 1) element n - 1 category 3."""
    s = 7000 + 31 * seed + (n % 9973)
    p = det.unitvar((n,), s)
    e = det.uniform((n,), s + 1, -20.0, 15.0).astype(np.float64)
    sign = np.where(det.uniform01((n,), s + 2) < 0.5, -1.0, 1.0)
    g = (sign * 10.0 ** e).astype(np.float32)
    cat = det.randint((n,), s + 3, 0, 4)
    cat[0] = 0
    if n > 1:
        cat[-1] = 3
    fac = det.uniform((n,), s + 4, 0.05, 0.2).astype(np.float64)
    g[cat == 0] = 0.0
    m = np.zeros(n, np.float64)
    m[cat == 2] = (g.astype(np.float64) * fac * 8.0)[cat == 2]
    m[cat == 3] = (-g.astype(np.float64) * fac)[cat == 3]
    v = np.where(cat >= 2, (g.astype(np.float64) ** 2) * det.uniform((n,), s + 5, 0.5, 1.5), 0.0)
    return p, g, m.astype(np.float32), v.astype(np.float32)


def _f32(x) -> float:
    return float(np.float32(x))


def ref_adamw(p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale):
    """fp64 reference of the CONTRACT: torch's single-tensor AdamW (the formula in the header of csrc/optim.hip) with the hyper-parameters
    as the float32 values the entry receives; 1 - beta from the float32 beta (exact for beta >= 0.5); bias corrections in double from
    the float32 betas, as the host code forms them.  Returns (p', m', v', upd, kappa): upd = the update subtracted from the decayed p,
    kappa = (|b1 m| + |(1 - b1) g|) / |m'| >= 1, the condition number of the sum that forms m' (1 where m and g agree in sign)."""
    lr, b1, b2, eps, wd, gs = _f32(lr), _f32(betas[0]), _f32(betas[1]), _f32(eps), _f32(weight_decay), _f32(grad_scale)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    g = g * gs
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    t1, t2 = b1 * m, (1.0 - b1) * g
    m2 = t1 + t2
    v2 = b2 * v + (1.0 - b2) * g * g
    upd = (lr / bc1) * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps)
    p2 = p * (1.0 - lr * wd) - upd
    mag = np.abs(t1) + np.abs(t2)
    kappa = np.where(m2 != 0.0, mag / np.where(m2 != 0.0, np.abs(m2), 1.0), 1.0)
    return p2, m2, v2, upd, kappa


def np_adamw_kernel(p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale, plant: str = ""):
    """adamw_kernel + ds2_adamw_gated_f32's host part in float32, statement by statement.  Returns new (p, m, v) float32.
    plant: '' | 'eps_in_sqrt' | 'bc2_no_sqrt' | 'l2_decay' | 'decay_after' | 'gscale_once' | 'step_minus_1' | 'tail_untouched'."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = f(lr), f(betas[0]), f(betas[1]), f(eps), f(weight_decay), f(grad_scale)
    p0, m0, v0 = (np.asarray(a, np.float32) for a in (p, m, v))
    st = step - 1 if plant == "step_minus_1" else step
    with np.errstate(all="ignore"):
        bc1 = f(1.0 - float(b1) ** st)
        bc2 = 1.0 - float(b2) ** st
        bc2s = f(bc2) if plant == "bc2_no_sqrt" else f(np.sqrt(bc2))
        gg = (np.asarray(g, np.float32) * gs).astype(np.float32)
        pp = p0
        if plant == "l2_decay":
            gg = (gg + wd * pp).astype(np.float32)
        elif plant != "decay_after":
            pp = (pp * f(f(1.0) - f(lr * wd))).astype(np.float32)
        mm = (f(b1) * m0 + (f(1.0) - b1) * gg).astype(np.float32)
        g2 = np.asarray(g, np.float32) if plant == "gscale_once" else gg
        vv = (b2 * v0 + ((f(1.0) - b2) * gg).astype(np.float32) * g2).astype(np.float32)
        if plant == "eps_in_sqrt":
            den = np.sqrt((vv / f(bc2s * bc2s) + eps).astype(np.float32)).astype(np.float32)
        else:
            den = ((np.sqrt(vv).astype(np.float32) / bc2s).astype(np.float32) + eps).astype(np.float32)
        pp = (pp - ((f(lr / bc1) * mm).astype(np.float32) / den).astype(np.float32)).astype(np.float32)
        if plant == "decay_after":
            pp = (pp * f(f(1.0) - f(lr * wd))).astype(np.float32)
    if plant == "tail_untouched":
        k = len(p0) - len(p0) % 4
        pp[k:], mm[k:], vv[k:] = p0[k:], m0[k:], v0[k:]
    return pp, mm, vv


def check_adamw(got, state, step, hyper, what: str = ""):
    """got = (p', m', v') of ONE step from state = (p, g, m, v), per element against ref_adamw, u = 2^-24, first order:
      m' :  3 u (|b1 m| + |(1 - b1) g|)     the two products and the addition (1 - b1 is exact);
      v' :  4 u (|b2 v| + |(1 - b2) g^2|) + 2 TINY    (1 - b2) * g, * g, b2 * v and the addition: at most 3 roundings on a term (4 as the
            issue states it; g * grad_scale is exact for the powers of two used here); TINY = 2^-149: the two products of the g^2 term
            may underflow (|g| down to 1e-20 with v = 0), each then off by at most half of the smallest subnormal;
      p' :  3 u |p| + c u |upd| (+ the v' underflow carried through the denominator),  c = 11 + 3 kappa:
              |p| : the decay factor fl(1 - fl(lr wd)), the product p * factor, and |p|'s share of the final subtraction;
              c   : bc1 rounded to float by the host (1), lr / bc1 (1), m' itself (3 kappa, its bound above relative to |m'|; kappa = 1
                    where m and g agree in sign or m = 0: c = 14), the product with m' (1), the denominator (6: v' carries 4 u, halved by the
                    square root = 2, sqrtf correctly rounded 1, sqrt(bc2) rounded to float by the host 1, the division by it 1, the
                    addition of eps 1 — all of them shrink by sqrt(v^)/den <= 1), the division by it (1), and |upd|'s share of the final
                    subtraction (1): 1 + 1 + 1 + 6 + 1 + 1 = 11, plus 3 kappa.
            Operation counts of the kernel's statements under correctly rounded +, *, /, sqrtf (hipcc's default); none of it measured.
    Where g = 0 and m = v = 0: m' = v' = 0 exactly and p' has the bits of p * fl(1 - fl(lr wd)) in float32."""
    p, g, m, v = state
    gp, gm, gv = (np.asarray(a, np.float64) for a in got)
    p2, m2, v2, upd, kappa = ref_adamw(p, g, m, v, step, **hyper)
    b1, b2, gs = _f32(hyper["betas"][0]), _f32(hyper["betas"][1]), _f32(hyper["grad_scale"])
    p64, g64, m64, v64 = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gg = g64 * gs
    bm = 3 * U * (np.abs(b1 * m64) + np.abs((1.0 - b1) * gg))
    bv = 4 * U * (np.abs(b2 * v64) + np.abs((1.0 - b2) * gg * gg)) + np.where(gg != 0.0, 2 * TINY, 0.0)
    bc2s = np.sqrt(1.0 - b2 ** step)
    den = np.sqrt(v2) / bc2s + _f32(hyper["eps"])
    under = np.where(v2 > 0.0, 2 * TINY / (2.0 * np.sqrt(np.where(v2 > 0.0, v2, 1.0)) * bc2s * den), 0.0)      # d den / den for dv = 2 TINY
    bp = 3 * U * np.abs(p64) + (ADAMW_C0 + 3 * kappa) * U * np.abs(upd) + under * np.abs(upd)
    for name, got_, ref_, bnd in (("m", gm, m2, bm), ("v", gv, v2, bv), ("p", gp, p2, bp)):
        bad = ~(np.abs(got_ - ref_) <= bnd)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{what}: {name}: {int(bad.sum())} of {bad.size} outside the bound, first at {i}: got {got_[i]!r} want {ref_[i]!r} "
                                 f"(err {abs(got_[i] - ref_[i]):.3e}, bound {bnd[i]:.3e})")
    z = (g64 == 0.0) & (m64 == 0.0) & (v64 == 0.0)
    if z.any():
        f = np.float32
        decay = f(f(1.0) - f(f(hyper["lr"]) * f(hyper["weight_decay"])))
        assert (gm[z] == 0.0).all() and (gv[z] == 0.0).all(), f"{what}: m', v' not exactly 0 where g = m = v = 0"
        assert_same_bits(np.asarray(got[0], np.float32)[z], (np.asarray(p, np.float32)[z] * decay).astype(np.float32), what + ": p where the update is 0")
