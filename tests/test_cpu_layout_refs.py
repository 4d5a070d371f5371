"""The references and checkers of tests/layout_cases.py, without a GPU: every checker must ACCEPT a float32 numpy restatement of its
kernel's statement order on every case of the GPU files (the reference alone stays inside every bound), and must REJECT each planted
mistake — a checker that cannot tell a subtly wrong kernel from a right one anchors nothing."""
import numpy as np
import pytest
import torch

import det
import layout_cases as L


def rejects(fn, *a, **kw) -> bool:
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------- bits, special values, rounding
def test_special_values_and_rounding_reference():
    """torch's x.bfloat16() (THE reference of every cast test) is round-to-nearest-even on every special value, the numpy restatement
    agrees with it bit for bit, and the builder really places the values it promises — first and last element included."""
    sp = np.array(L.SPECIAL_BITS, np.uint32).view(np.float32)
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82, 0x3F807FFF: 0x3F80, 0x3F808001: 0x3F81,
            0x7F7FFFFF: 0x7F80, 0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80,
            0x00000001: 0x0000, 0x007FFFFF: 0x0080, 0x80012345: 0x8001, 0x00408000: 0x0040, 0x00018000: 0x0002, 0x00008000: 0x0000}
    tb = L.bits(L.ref_bf16(sp))
    for b, t in zip(L.SPECIAL_BITS, tb):
        if b in want:
            assert int(t) == want[b], (hex(b), hex(int(t)))
    assert torch.isnan(L.ref_bf16(sp)[L.SPECIAL_BITS.index(0x7FC00000)])
    L.assert_same_bits(L.np_bf16_bits(sp), L.ref_bf16(sp), "specials")
    for shape in [(65, 63), (1, 130), (3, 7), (2040,)]:
        x = L.special_f32(shape, 3)
        L.assert_same_bits(L.np_bf16_bits(x), L.ref_bf16(x), str(shape))
        xb = set(int(b) for b in L.bits(x).reshape(-1))
        assert set(L.SPECIAL_BITS) <= xb
        assert int(L.bits(x).reshape(-1)[0]) == L.SPECIAL_BITS[0] and int(L.bits(x).reshape(-1)[-1]) == L.SPECIAL_BITS[-1]
        assert int(L.subnormal_mask(x).sum()) == 6
    fin = L.special_f32((129, 70), 5, finite=True)
    assert np.isfinite(fin).all() and float(np.abs(fin).max()) < 4.0 and L.subnormal_mask(fin).any()
    tiny = L.special_f32((1, 1), 2)
    assert int(L.bits(tiny)[0, 0]) in L.SPECIAL_BITS
    # the NaN rule: payloads are free, NaN against a number is not
    L.assert_same_bits(np.array([0x7FC1, 0xFFFF], np.uint16), np.array([0x7FC0, 0x7FC0], np.uint16))
    assert rejects(L.assert_same_bits, np.array([0x7F80], np.uint16), np.array([0x7FC0], np.uint16))
    assert rejects(L.assert_same_bits, np.array([0x7FC0], np.uint16), np.array([0x7F80], np.uint16))
    assert rejects(L.assert_same_bits, np.array([0x8000], np.uint16), np.array([0x0000], np.uint16))        # -0 is not +0
    # a conversion that flushed subnormal inputs to a signed zero would not pass
    flushed = np.where(L.subnormal_mask(sp), np.where(np.signbit(sp), 0x8000, 0), L.np_bf16_bits(sp)).astype(np.uint16)
    assert rejects(L.assert_same_bits, flushed, L.ref_bf16(sp))


# ---------------------------------------------------------------------------------------------- casts
@pytest.mark.parametrize("R", L.CAST_R)
@pytest.mark.parametrize("Cc", L.CAST_C)
def test_cast_restatement_accepted(R, Cc):
    for ld in L.cast_lds(Cc):
        x = L.special_f32((R, Cc), 11)
        L.assert_same_bits(L.np_cast(x, 0, Cc, ld), L.ref_cast(x, ld))
        big, c0 = L.unaligned_view((R, Cc), 12)
        L.assert_same_bits(L.np_cast(big, c0, Cc, ld), L.ref_cast(big[:, c0:c0 + Cc], ld))


@pytest.mark.parametrize("R,Cc", L.T_SHAPES)
def test_cast_transpose_restatement_accepted(R, Cc):
    big, c0 = L.unaligned_view((R, Cc), 13, finite=True)
    x = big[:, c0:c0 + Cc]
    L.assert_same_bits(L.np_cast_t(big, c0, Cc), L.ref_cast_t(x))
    L.check_colsum(L.np_colsum_tiles(x), x)
    xb = L.ref_bf16(x)                                                       # transpose_bf16: a bf16 source, sums of its widened values
    L.assert_same_bits(L.np_cast_t(xb.float().numpy(), 0, Cc), L.ref_cast_t(xb))
    L.check_colsum(L.np_colsum_tiles(xb.float().numpy()), xb.float().numpy())


def test_cast_checker_rejects_planted_mistakes():
    R, Cc = 65, 63
    big, c0 = L.unaligned_view((R, Cc), 12)
    x = big[:, c0:c0 + Cc]
    ref = L.ref_cast(x)
    L.assert_same_bits(L.np_cast(big, c0, Cc), ref)
    assert rejects(L.assert_same_bits, L.np_cast(big, c0, Cc, mode="trunc"), ref)
    assert rejects(L.assert_same_bits, L.np_cast(big, c0, Cc, mode="away"), ref)
    assert rejects(L.assert_same_bits, L.np_cast(big, c0, Cc, pad="input"), ref)
    assert rejects(L.assert_same_bits, L.np_cast_t(big, c0, Cc, mode="trunc"), L.ref_cast_t(x))
    assert rejects(L.assert_same_bits, L.np_cast_t(big, c0, Cc, mode="away"), L.ref_cast_t(x))
    # ties away from zero differs from RNE ONLY at a tie above an even upper half: on data without the special values it would pass
    plain = det.unitvar((R, Cc), 12)
    L.assert_same_bits(L.np_cast(plain, 0, Cc, mode="away"), L.ref_cast(plain))
    # column sums: one row left out, one column shifted, a float16-grade sum
    xf = L.special_f32((129, 70), 13, finite=True)
    cs = L.np_colsum_tiles(xf)
    L.check_colsum(cs, xf)
    assert rejects(L.check_colsum, L.np_colsum_tiles(xf[:-1]), xf)
    assert rejects(L.check_colsum, np.roll(cs, 1), xf)
    assert rejects(L.check_colsum, cs.astype(np.float16).astype(np.float32), xf)


# ---------------------------------------------------------------------------------------------- split
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("pad_rows", [0, 64])
def test_split_restatement_accepted_and_mistakes_rejected(order, pad_rows):
    for R in L.SPLIT_R:
        for Cc in L.SPLIT_C:
            big, c0 = L.unaligned_view((R, Cc), 21)
            for x in (L.special_f32((R, Cc), 20), big[:, c0:c0 + Cc]):
                ref = L.ref_split(x, order, pad_rows)
                assert ref.shape == (-(-R // pad_rows) * pad_rows if pad_rows else R, (2 if order == 2 else 3) * L.pad8(Cc))
                L.assert_same_bits(L.np_split(x, order, pad_rows), ref)
                assert rejects(L.assert_same_bits, L.np_split(x, order, pad_rows, lo_from_x=True), ref)
                if order != 2:
                    assert rejects(L.assert_same_bits, L.np_split(x, order, pad_rows, swap01=True), ref)
    # hi + lo recovers x to 2^-17 relative (two bf16 roundings), exactly where x has 16 significant bits
    x = det.unitvar((5, 9), 22)
    s = L.ref_split(x, 2).float()
    assert np.abs((s[:, :9] + s[:, 16:25]).numpy().astype(np.float64) - x).max() <= 2.0 ** -17 * np.abs(x).max()


# ---------------------------------------------------------------------------------------------- residual, padcast, nhwc, transposes
def test_residual_and_padcast_and_layout_references():
    x = L.special_f32((1023,), 30)
    r = L.ref_residual(x)
    hi = L.np_bf16_to_f32(L.np_bf16_bits(x))
    with np.errstate(invalid="ignore"):
        L.assert_same_bits((x - hi).astype(np.float32), r)
    fin = np.isfinite(x) & np.isfinite(hi)
    assert (hi[fin].astype(np.float64) + r.numpy()[fin].astype(np.float64) == x[fin].astype(np.float64)).all()       # the subtraction is exact
    for (B, C_, D) in L.PADCAST_BCD:
        for T in L.PADCAST_T:
            x = L.special_f32((B, C_, D, T), 31)
            ref = L.ref_padcast(x)
            Tp = L.padded_pitch(T)
            assert ref.shape[-1] == Tp and Tp % 8 == 0 and Tp >= T + 16
            rb = L.bits(ref)
            assert not rb[..., :8].any() and not rb[..., 8 + T:].any()
            L.assert_same_bits(L.np_padcast(x), ref)
            assert rejects(L.assert_same_bits, L.np_padcast(x, lead=7), ref), (B, C_, D, T)
            assert rejects(L.assert_same_bits, L.np_padcast(x, clear_tail=False), ref)
    x = L.special_f32((3, 32, 2, 130), 32)
    n = L.ref_nhwc(x)
    assert n.shape == (3, 2, 130, 32)
    assert int(L.bits(n)[2, 1, 129, 31]) == int(L.np_bf16_bits(x)[2, 31, 1, 129]) and int(L.bits(n)[0, 0, 0, 0]) == int(L.np_bf16_bits(x)[0, 0, 0, 0])


# ---------------------------------------------------------------------------------------------- softmax
def _softmax_inputs():
    for rows in L.SOFTMAX_ROWS:
        for Cc in L.SOFTMAX_C:
            yield f"plain {rows}x{Cc}", L.softmax_logits(rows, Cc), None
            grid = L.softmax_logits(rows, Cc, "grid")
            ref = L.ref_softmax(grid)
            for sh in L.SOFTMAX_SHIFTS:
                yield f"grid{sh:+.0f} {rows}x{Cc}", (grid + np.float32(sh)).astype(np.float32), ref
            yield f"neginf {rows}x{Cc}", L.softmax_logits(rows, Cc, "neginf"), None
            yield f"single {rows}x{Cc}", L.softmax_logits(rows, Cc, "single"), None


def test_softmax_restatement_accepted_on_every_case():
    n = 0
    for what, x, ref in _softmax_inputs():
        y = L.np_softmax_kernel(x)
        L.check_softmax(y, x, ref, what)
        assert (y[np.isneginf(x)] == 0.0).all()
        if what.startswith("single"):
            assert (y[np.isfinite(x)] == 1.0).all() and (y.sum(1) == 1.0).all()
        if what.startswith("grid"):
            assert (ref == L.ref_softmax(x)).all(), what                      # the shift is exact: the very same reference
        n += 1
    assert n == len(L.SOFTMAX_ROWS) * len(L.SOFTMAX_C) * 6


def test_softmax_checker_rejects_planted_mistakes():
    for Cc in (65, 80, 200):
        x = L.softmax_logits(5, Cc)
        assert rejects(L.check_softmax, L.np_softmax_kernel(x, sum_cols=64), x)
        # a maximum over the first 64 columns is the same softmax until it overflows: the row whose first 64 logits are all -inf shows it
        xi = L.softmax_logits(5, Cc, "neginf")
        L.check_softmax(L.np_softmax_kernel(xi), xi)
        assert rejects(L.check_softmax, L.np_softmax_kernel(xi, max_cols=64), xi)
    x = L.softmax_logits(77, 29)
    y = L.np_softmax_kernel(x)
    assert rejects(L.check_softmax, y * np.float32(1 + 2.0 ** -18), x)        # a relative error of 4e-6 on every entry
    assert rejects(L.check_softmax, np.roll(y, 1, axis=1), x)


# ---------------------------------------------------------------------------------------------- batch mean
def test_batch_mean_restatement_accepted_and_bound_bites():
    for B in L.BATCH_MEAN_B:
        nll = L.batch_mean_nll(B)
        got = L.np_batch_mean_kernel(nll)
        L.check_batch_mean(got, nll)
        if B > 1:
            assert rejects(L.check_batch_mean, L.np_batch_mean_kernel(nll[:-1]) * np.float32((B - 1) / B), nll)      # the last utterance dropped
            assert rejects(L.check_batch_mean, got * np.float32(B) / np.float32(B + 1), nll)                          # divided by B + 1
    bad = L.batch_mean_nll(65)
    bad[64] = np.nan
    assert np.isnan(L.np_batch_mean_kernel(bad))


# ---------------------------------------------------------------------------------------------- AdamW
ADAMW_CPU_N = [n for n in L.ADAMW_N if n < 10 ** 6] + [4096 * 4 + 5]      # (the 4 M element case runs once, below)


@pytest.mark.parametrize("hyper", list(L.ADAMW_HYPER))
@pytest.mark.parametrize("step", L.ADAMW_STEPS)
def test_adamw_restatement_accepted(step, hyper):
    for n in ADAMW_CPU_N:
        st = L.adamw_state(n, step)
        L.check_adamw(L.np_adamw_kernel(*st, step, **L.ADAMW_HYPER[hyper]), st, step, L.ADAMW_HYPER[hyper], f"n={n} step={step} {hyper}")


def test_adamw_restatement_accepted_at_full_size():
    """... and why the p' bound carries kappa: with a constant c = 14 (m and g taken to agree in sign everywhere) the float32 restatement
    itself leaves the bound on an element whose m' cancels, so that form cannot be asked of the kernel either."""
    n, step, hyper = L.ADAMW_N[-1], 1, L.ADAMW_HYPER["stressed"]
    st = L.adamw_state(n, step)
    got = L.np_adamw_kernel(*st, step, **hyper)
    L.check_adamw(got, st, step, hyper, "full size")
    p2, _, _, upd, kappa = L.ref_adamw(*st, step, **hyper)
    flat = 3 * L.U * np.abs(st[0].astype(np.float64)) + (L.ADAMW_C0 + 3) * L.U * np.abs(upd)
    out = np.abs(got[0].astype(np.float64) - p2) > flat
    assert out.any() and (kappa[out] > 10.0).all()


def test_adamw_state_covers_what_the_issue_lists():
    p, g, m, v = L.adamw_state(1003, 1)
    a = np.abs(g[g != 0])
    assert (g == 0).any() and a.min() < 1e-19 and a.max() > 1e14 and (g > 0).any() and (g < 0).any()
    assert (v >= 0).all() and np.isfinite(p).all() and np.isfinite(g).all() and np.isfinite(m).all() and np.isfinite(v).all()
    assert ((g == 0) & (m == 0) & (v == 0)).any() and ((g != 0) & (m == 0)).any() and (m * g > 0).any() and (m * g < 0).any()
    _, _, _, _, kappa = L.ref_adamw(p, g, m, v, 2, **L.ADAMW_HYPER["trainer"])
    assert kappa.min() >= 1.0 and kappa.max() > 3.0                           # the cancelling elements are there


@pytest.mark.parametrize("plant", ["eps_in_sqrt", "bc2_no_sqrt", "l2_decay", "decay_after", "gscale_once", "step_minus_1", "tail_untouched"])
def test_adamw_checker_rejects(plant):
    """Each planted mistake, planted in the float32 restatement, moves at least one element past its bound — on the stressed set for every
    step, and (all but the two that need a large lr * wd or grad_scale != 1) on the trainer's defaults too."""
    n = 1003
    for step in L.ADAMW_STEPS:
        st = L.adamw_state(n, step)
        for name, hyper in L.ADAMW_HYPER.items():
            L.check_adamw(L.np_adamw_kernel(*st, step, **hyper), st, step, hyper)
            r = rejects(L.check_adamw, L.np_adamw_kernel(*st, step, **hyper, plant=plant), st, step, hyper)
            if name == "stressed":
                assert r, (plant, step, name)
            elif plant not in ("decay_after", "gscale_once"):
                assert r, (plant, step, name)
    for n in (1, 2, 3, 5):                                                    # the n % 4 tail of a buffer shorter than, or just past, one float4
        if plant == "tail_untouched":
            st = L.adamw_state(n, 1)
            assert rejects(L.check_adamw, L.np_adamw_kernel(*st, 1, **L.ADAMW_HYPER["stressed"], plant=plant), st, 1, L.ADAMW_HYPER["stressed"])
