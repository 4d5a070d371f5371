"""-m gpu: the kernels that move, round and re-lay data between the heavy ones (casts, transposes, split / padded / channels-last bf16
operands), each against a plain restatement of the same operation — bit for bit, at the shapes where such kernels go wrong: one element,
sizes around the tile and vector widths, unaligned and pitched sources (the scalar `vec == 0` path), zero pads, special values, and one
size per grid cap that sends the stride loop round a second time.  Shapes, inputs and references: tests/layout_cases.py (checked on the
CPU by tests/test_cpu_layout_refs.py).

Special values (layout_cases.SPECIAL_BITS) ride in every cast input: +-0, +-inf, NaN, the largest finite float (rounds to +inf), exact
bf16 ties above an even and an odd upper half in both signs, a value on either side of a tie, fp32 subnormals.  The reference is torch's
x.bfloat16() on the CPU; NaN positions only have to be NaN.  Subnormals are held to round-to-nearest-even like every other value: the
gfx950 conversion does not flush them (a subnormal input keeps its rounded subnormal bf16, a subnormal bf16 widens to itself)."""
import functools

import numpy as np
import pytest
import torch

import layout_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def g(a, dev):
    return torch.as_tensor(np.asarray(a)).to(dev)


def poison(dev, nbytes):
    """leave NaNs for the allocator to hand back: an output the kernel does not write then shows (best effort — never the only check)"""
    torch.full((max(int(nbytes), 4) // 4,), float("nan"), device=dev)


def sources(R, Cc, seed, dev, finite=False):
    """(label, the (R, C) values on the host, the device source): contiguous, and the unaligned odd-pitch column view (vec == 0)"""
    x = L.special_f32((R, Cc), seed, finite)
    big, c0 = L.unaligned_view((R, Cc), seed + 1, finite)
    return [("contiguous", x, g(x, dev)), ("view", big[:, c0:c0 + Cc], g(big, dev)[:, c0:c0 + Cc])]


@functools.lru_cache(maxsize=2)
def big_flat(n, seed):
    return L.special_f32((n,), seed)


# ---------------------------------------------------------------------------------------------- cast_bf16
@pytest.mark.parametrize("Cc", L.CAST_C)
@pytest.mark.parametrize("R", L.CAST_R)
def test_cast_bf16(dev, R, Cc):
    """(R, C) -> (R, ld) for ld = default, pad8(C) + 8, pad8(C) + 64: values rounded to nearest even, columns C..ld zero; contiguous and on
    the odd-pitch view big[:, 1:1+C]."""
    from asr_amd import ops
    for label, x, src in sources(R, Cc, 100, dev):
        for ld in L.cast_lds(Cc):
            ref = L.ref_cast(x, ld)
            poison(dev, ref.numel() * 2)
            got = ops.cast_bf16(src, ld)
            assert got.shape == ref.shape and got.is_contiguous()
            L.assert_same_bits(got, ref, f"cast_bf16 {label} ({R},{Cc}) ld={ld}")
            assert not L.bits(got)[:, Cc:].any()


def test_cast_bf16_second_trip(dev):
    """R * ld / 4 > 8192 * 256: every thread of the capped grid converts a second group; C % 8 == 4 keeps a half-filled last group per row"""
    from asr_amd import ops
    R, Cc = L.CAST_BIG
    assert R * L.pad8(Cc) // 4 > 8192 * 256
    x = L.special_f32((R, Cc), 101)
    poison(dev, R * L.pad8(Cc) * 2)
    L.assert_same_bits(ops.cast_bf16(g(x, dev)), L.ref_cast(x), "cast_bf16 second trip")


# ---------------------------------------------------------------------------------------------- transposing casts
@pytest.mark.parametrize("R,Cc", L.T_SHAPES)
def test_cast_transpose_and_both(dev, R, Cc):
    """cast_transpose_bf16 (without / with colsum=) and cast_bf16_both (without / with colsum, ld_r default and pad8(C) + 8 where the entry
    accepts it): the transposed copy (C, pad8(R)) and the row-major copy (R, ld_r), every pad column zero, and the column sums against the
    fp64 sums of the same fp32 source values within  n * 2^-24 * sum_r |x[r, c]|,  n = 64: cast_transpose_bf16_kernel adds the 64 rows of
    its tile one after the other in fp32 and ds2i_col_finalize_sums adds the tiles' partials in fp64 (layout_cases.check_colsum).
    The copies are checked with inf / NaN in the source, the sums on finite sources (subnormals and ties stay in)."""
    from asr_amd import ops
    for label, x, src in sources(R, Cc, 110, dev):
        what = f"{label} ({R},{Cc})"
        ref_t = L.ref_cast_t(x)
        poison(dev, ref_t.numel() * 2)
        got_t = ops.cast_transpose_bf16(src)
        assert got_t.shape == ref_t.shape
        L.assert_same_bits(got_t, ref_t, "cast_transpose_bf16 " + what)
        for ld_r in L.both_ld_r(Cc):
            ref_r = L.ref_cast(x, ld_r)
            poison(dev, ref_r.numel() * 2)
            poison(dev, ref_t.numel() * 2)
            got_r, got_t = ops.cast_bf16_both(src, ld_r=ld_r)
            L.assert_same_bits(got_r, ref_r, f"cast_bf16_both row-major {what} ld_r={ld_r}")
            L.assert_same_bits(got_t, ref_t, f"cast_bf16_both transposed {what} ld_r={ld_r}")
    for label, x, src in sources(R, Cc, 112, dev, finite=True):
        what = f"{label} ({R},{Cc})"
        ref_t = L.ref_cast_t(x)
        cs = torch.full((Cc,), float("nan"), device=dev)
        got_t = ops.cast_transpose_bf16(src, colsum=cs)
        L.assert_same_bits(got_t, ref_t, "cast_transpose_bf16 colsum= " + what)
        L.check_colsum(cs.cpu().numpy(), x, "cast_transpose_bf16 colsum= " + what)
        for ld_r in L.both_ld_r(Cc):
            poison(dev, Cc * 4)
            got_r, got_t, cs2 = ops.cast_bf16_both(src, colsum=True, ld_r=ld_r)
            L.assert_same_bits(got_r, L.ref_cast(x, ld_r), f"cast_bf16_both colsum row-major {what} ld_r={ld_r}")
            L.assert_same_bits(got_t, ref_t, f"cast_bf16_both colsum transposed {what} ld_r={ld_r}")
            assert cs2.shape == (Cc,)
            L.check_colsum(cs2.cpu().numpy(), x, f"cast_bf16_both colsum {what} ld_r={ld_r}")
            assert torch.equal(cs2, cs)                                      # one kernel, one order: the two entries agree bit for bit


@pytest.mark.parametrize("R,Cc", L.T_SHAPES)
def test_transpose_bf16(dev, R, Cc):
    """bf16 (R, C) -> (C, pad8(R)), colsum False / True / a caller's tensor.  The entry wants a pitch % 8 == 0 and a 16-byte base: the sources
    are the first C columns of an (R, pad8(C)) buffer and the column block [8, 8 + C) of an (R, pad8(C) + 16) one.  Column sums: of the
    bf16 values widened to fp32, same bound as above with n = 64 (transpose_bf16_kernel sums its 64-row tile the same way)."""
    from asr_amd import ops
    for finite in (False, True):
        for label, W, c0 in (("natural", L.pad8(Cc), 0), ("column block", L.pad8(Cc) + 16, 8)):
            big = L.ref_bf16(L.special_f32((R, W), 120 + c0, finite))
            xb = big[:, c0:c0 + Cc]
            src = big.to(dev)[:, c0:c0 + Cc]
            what = f"transpose_bf16 {label} ({R},{Cc})"
            ref_t = L.ref_cast_t(xb)
            poison(dev, ref_t.numel() * 2)
            if not finite:
                L.assert_same_bits(ops.transpose_bf16(src), ref_t, what)
                continue
            got_t, cs = ops.transpose_bf16(src, colsum=True)
            L.assert_same_bits(got_t, ref_t, what + " colsum=True")
            L.check_colsum(cs.cpu().numpy(), xb.float().numpy(), what + " colsum=True")
            mine = torch.full((Cc + 4,), float("nan"), device=dev)
            got_t, cs2 = ops.transpose_bf16(src, colsum=mine[:Cc])
            L.assert_same_bits(got_t, ref_t, what + " colsum=tensor")
            assert cs2.data_ptr() == mine.data_ptr() and torch.equal(mine[:Cc], cs) and bool(torch.isnan(mine[Cc:]).all())


# ---------------------------------------------------------------------------------------------- split_bf16
@pytest.mark.parametrize("pad_rows", [0, 64])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_split_bf16(dev, order, pad_rows):
    """hi = bf16(x), lo = bf16(x - float(hi)) (exact subtraction: the reference is unambiguous); order 0 = [hi | hi | lo], 1 = [hi | lo | hi],
    2 = [hi | lo], every block pad8(C) wide; pad columns and pad rows zero.  R x C over the whole grid, contiguous and unaligned."""
    from asr_amd import ops
    for R in L.SPLIT_R:
        for Cc in L.SPLIT_C:
            for label, x, src in sources(R, Cc, 130, dev):
                ref = L.ref_split(x, order, pad_rows)
                poison(dev, ref.numel() * 2)
                got = ops.split_bf16(src, order, pad_rows)
                assert got.shape == ref.shape
                L.assert_same_bits(got, ref, f"split_bf16 order {order} pad_rows {pad_rows} {label} ({R},{Cc})")


def test_split_bf16_second_trip(dev):
    """R * pad8(C) / 4 > 16384 * 256: the capped grid's stride loop goes round again"""
    from asr_amd import ops
    R, Cc = 2050, 8196
    assert R * L.pad8(Cc) // 4 > 16384 * 256
    x = L.special_f32((R, Cc), 131)
    L.assert_same_bits(ops.split_bf16(g(x, dev), 2), L.ref_split(x, 2), "split_bf16 second trip")


# ---------------------------------------------------------------------------------------------- widen, residual, sum3
@pytest.mark.parametrize("n", L.WIDEN_N)
def test_widen_bf16(dev, n):
    from asr_amd import ops
    xb = L.ref_bf16(big_flat(n, 140))
    poison(dev, n * 4)
    L.assert_same_bits(ops.widen_bf16(xb.to(dev)), xb.float(), f"widen_bf16 n={n}")


@pytest.mark.parametrize("n", L.FLAT_N)
def test_bf16_residual(dev, n):
    """x - float(bf16(x)), exact in fp32 (inf - inf and NaN give NaN on both sides)"""
    from asr_amd import ops
    x = big_flat(n, 141)
    poison(dev, n * 4)
    L.assert_same_bits(ops.bf16_residual(g(x, dev)), L.ref_residual(x), f"bf16_residual n={n}")


@pytest.mark.parametrize("n", L.FLAT_N)
def test_sum3(dev, n):
    """three operands: the bits of (a + b) + c in fp32; two operands: the VALUE a + b (the kernel adds a +0.f, which turns -0 into +0);
    b and c untouched, the result is `a` itself"""
    from asr_amd import ops
    a = big_flat(n, 141)
    with np.errstate(over="ignore"):                                        # (the largest finite float times -1.25: an inf more)
        b = np.ascontiguousarray(a[::-1]) * np.float32(0.75)
        c = np.roll(a, 1) * np.float32(-1.25)
    ta, tb, tc = torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)
    ad, bd, cd = g(a, dev).clone(), g(b, dev), g(c, dev)
    out = ops.sum3_(ad, bd, cd)
    assert out is ad
    L.assert_same_bits(ad, (ta + tb) + tc, f"sum3_ n={n}")
    L.assert_same_bits(bd, tb, "b untouched")
    L.assert_same_bits(cd, tc, "c untouched")
    ad = g(a, dev).clone()
    p0 = ad.data_ptr()
    out = ops.sum3_(ad, bd)
    ref = (ta + tb).numpy()
    got = out.cpu().numpy()
    assert out is ad and ad.data_ptr() == p0
    assert np.where(np.isnan(ref), np.isnan(got), got == ref).all(), f"sum3_ two operands n={n}"
    L.assert_same_bits(bd, tb, "b untouched")


# ---------------------------------------------------------------------------------------------- fp32 transposes
@pytest.mark.parametrize("B,F,T", L.BFT_SHAPES)
def test_transpose_bft(dev, B, F, T):
    """(B,F,T) -> (T,B,F) equals permute(2,0,1), the other direction its inverse, and the round trip returns the input — bits, on data with
    NaN payloads and signed zeros in it (a move must not touch them)"""
    from asr_amd import ops
    a = torch.from_numpy(L.special_f32((B, F, T), 150))
    poison(dev, a.numel() * 4)
    tbf = ops.transpose_bft(g(a, dev), B, F, T, True)
    assert tbf.shape == (T, B, F)
    assert np.array_equal(L.bits(tbf), L.bits(a.permute(2, 0, 1).contiguous()))
    c = torch.from_numpy(L.special_f32((T, B, F), 151))
    poison(dev, a.numel() * 4)
    bft = ops.transpose_bft(g(c, dev), B, F, T, False)
    assert bft.shape == (B, F, T)
    assert np.array_equal(L.bits(bft), L.bits(c.permute(1, 2, 0).contiguous()))
    assert np.array_equal(L.bits(ops.transpose_bft(tbf, B, F, T, False)), L.bits(a))


@pytest.mark.parametrize("nb,R,Cc", L.BATCHED_SHAPES)
def test_transpose_batched(dev, nb, R, Cc):
    from asr_amd import ops
    a = torch.from_numpy(L.special_f32((nb, R, Cc), 152))
    poison(dev, a.numel() * 4)
    got = ops.transpose_batched(g(a, dev))
    assert got.shape == (nb, Cc, R)
    assert np.array_equal(L.bits(got), L.bits(a.transpose(1, 2).contiguous()))


# ---------------------------------------------------------------------------------------------- conv operands
@pytest.mark.parametrize("shape", L.NHWC_SHAPES)
def test_nhwc_bf16(dev, shape):
    """(B,32,D,T) fp32 -> (B,D,T,32) bf16 = x.permute(0,2,3,1).bfloat16()"""
    from asr_amd import ops
    x = L.special_f32(shape, 160)
    ref = L.ref_nhwc(x)
    poison(dev, ref.numel() * 2)
    got = ops.nhwc_bf16(g(x, dev))
    assert got.shape == ref.shape and got.is_contiguous()
    L.assert_same_bits(got, ref, f"nhwc_bf16 {shape}")


@pytest.mark.parametrize("T", L.PADCAST_T)
@pytest.mark.parametrize("B,Cc,D", L.PADCAST_BCD)
def test_padcast_bf16(dev, B, Cc, D, T):
    """(B,C,D,T) fp32 -> (B,C,D,Tp) bf16, Tp = ds2_conv_padded_pitch(T): eight leading zeros, the T values rounded once, a zero tail"""
    from asr_amd import _lib, ops
    x = L.special_f32((B, Cc, D, T), 161)
    ref = L.ref_padcast(x)
    Tp = _lib.load().ds2_conv_padded_pitch(T)
    assert Tp == L.padded_pitch(T)
    poison(dev, ref.numel() * 2)
    got = ops.padcast_bf16(g(x, dev))
    assert got.shape == (B, Cc, D, Tp) and got.is_contiguous()
    L.assert_same_bits(got, ref, f"padcast_bf16 ({B},{Cc},{D},{T})")
    gb = L.bits(got)
    assert not gb[..., :8].any() and not gb[..., 8 + T:].any()
