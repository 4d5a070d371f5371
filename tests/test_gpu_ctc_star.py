"""-m gpu: the wildcard CTC loss (ds2_ctc_star_loss_f32, ops.ctc_star_loss, CTCLoss(star=...)) against the plain entry (the same bits
without wildcards and flags), against itself (the one-wavefront lattice and the one-workgroup lattice write the same bits) and against
its fp64 restatement (tests/ctc_star_loss_oracle.py), with the bars tests/test_gpu_kernels.py holds the plain kernel to."""
import numpy as np
import pytest
import torch

import ctc_star_loss_oracle as O
import det
from helpers import rel_l2

pytestmark = pytest.mark.gpu

PEN = float(np.float32(np.log(0.5)))


def _labels(n, C, seed):
    return [int(v) for v in det.randint((max(n, 1),), seed, 1, C)[:n]]


def _edges(C):
    """One batch of the wave-kernel shapes (2U + 1 <= 127): (targets, input lengths, flags), T = 150.  W = C is the wildcard."""
    W, T = C, 150
    long50 = _labels(50, C, 5)
    long50[10:13] = [7, 7, W]                    # next to a repeated label
    long50[20:23] = [9, W, 9]                    # between two equal labels
    long50[30] = W                               # in the middle
    long63 = [W] + _labels(61, C, 6) + [W]       # first and last, S = 127: the last shape the wave kernel takes
    every4 = [W if k % 4 == 1 else v for k, v in enumerate(_labels(20, C, 7))]
    rows = [
        ([], 1, 0), ([W], 1, 0), ([W], 2, 3), ([3], 7, 1), ([W, 5], 8, 1), ([5, W], 9, 2), (long50, 145, 0), (long63, T, 3),
        (_labels(50, C, 8), 149, 3), ([4, W, 4, W, W], 10, 0), ([2, 2, 6], 17, 2), (_labels(63, C, 9), T, 1), ([1, 2], 2, 3),
        ([], 9, 3), (every4, T, 3),              # the last utterance of the batch holds wildcards and T_b = T
    ]
    return T, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def _workgroup(C):
    """A batch that takes the workgroup kernel (U = 64 and 200), T = 420."""
    W, T = C, 420
    t200 = [W if k % 8 == 3 else v for k, v in enumerate(_labels(200, C, 15))]
    t200[100:103] = [6, W, 6]
    t64 = [W] + _labels(62, C, 16) + [W]
    return T, [t64, [3, W, 3, 3, W], t200], [300, 9, T], [1, 2, 3]     # the last utterance: wildcards, T_b = T


def _infeasible(C):
    """More labels than frames, T_b = 0, a label C + 1 and a label 0 among utterances that are fine."""
    W, T = C, 40
    rows = [([1, W, 2], 40, 1), (_labels(12, C, 21), 11, 0), ([4, W], 0, 0), ([5, C + 1, 6], 30, 2), ([W, 2, 2], 40, 0), ([7, 0, 1], 25, 3),
            ([], 0, 0), ([W], 13, 2)]
    return T, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


CASES = {"edges_c29": (29, _edges), "edges_c80": (80, _edges), "workgroup_c29": (29, _workgroup), "workgroup_c80": (80, _workgroup),
         "infeasible_c29": (29, _infeasible)}
_CACHE = {}


def _case(name):
    """(C, T, targets, input lengths, flags, logits (T,B,C) fp32 numpy, oracle nll, oracle grad at scale 0.125): computed once."""
    if name not in _CACHE:
        C, make = CASES[name]
        T, targets, il, flags = make(C)
        logits = det.unitvar((T, len(targets), C), 7 + C + T) * np.float32(2.0)
        nll, grad = O.loss_and_grad(logits, targets, il, PEN, flags, grad_scale=0.125)      # (PEN is exact in fp32: log 0.5 rounded)
        for a in (logits, nll, grad):
            a.setflags(write=False)
        _CACHE[name] = (C, T, targets, il, flags, logits, nll, grad)
    return _CACHE[name]


def _device_targets(targets, dev):
    from asr_amd.ctc import _prep_targets
    flat = torch.tensor([i for t in targets for i in t], dtype=torch.int32)
    return _prep_targets(flat, torch.tensor([len(t) for t in targets], dtype=torch.int32), dev)


def _run(name, lattice, pen=PEN, with_flags=True, strip=False, plain=False):
    from asr_amd import ops
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    dev = torch.device("cuda:0")
    C, T, targets, il, flags, logits, _, _ = _case(name)
    if strip:
        targets = [[i for i in t if i != C] for t in targets]
    tg, off, tl, max_u = _device_targets(targets, dev)
    x = torch.from_numpy(logits.copy()).to(dev)
    ild = torch.tensor(il, dtype=torch.int32, device=dev)
    if plain:
        out = ops.ctc_loss(x, tg, off, ild, tl, max_u, 0.125, lattice=lattice, return_ab=True)
    else:
        fl = torch.tensor(flags, dtype=torch.int32, device=dev) if with_flags else None
        out = ops.ctc_star_loss(x, tg, off, ild, tl, max_u, 0.125, star_penalty=pen, flags=fl, lattice=lattice, return_ab=True)
    torch.cuda.synchronize()
    return out


def _same_bits(what, got, ref):
    for name, a, b in zip(("nll", "grad", "ab"), got, ref):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        print(f"{what}: {name} differing words: {diff} of {a.numel()}")
        assert diff == 0, (what, name)


@pytest.mark.parametrize("lattice", [0, 1])
@pytest.mark.parametrize("case", ["edges_c29", "edges_c80", "workgroup_c29", "workgroup_c80"])
def test_without_wildcards_and_flags_it_is_the_plain_loss_bit_for_bit(case, lattice):
    """No C in the targets, flags NULL: nll, gradient and both lattices are the bits of ops.ctc_loss, in both lattice kernels."""
    got = _run(case, lattice, with_flags=False, strip=True)
    ref = _run(case, lattice, strip=True, plain=True)
    assert np.isfinite(ref[0].cpu().numpy()).all()
    _same_bits(f"{case} lattice={lattice} star vs plain", got, ref)


@pytest.mark.parametrize("case", ["edges_c29", "edges_c80", "infeasible_c29"])
def test_wave_lattice_is_bit_identical_to_workgroup_lattice(case):
    """The STAR instances of the two lattice kernels, with wildcards and flags: the same bits, as the plain pair."""
    _same_bits(f"{case} wave vs workgroup", _run(case, 0), _run(case, 1))


# The gradient bar is the plain kernel's of tests/test_gpu_kernels.py, rel_l2 < 1e-4.  The two workgroup-kernel batches (U = 200 against
# T = 420, nll of about 1e3) miss it, and so does the PLAIN kernel on the same logits with the wildcards removed: at that size the
# roundings of alpha and beta, values of several hundred, random-walk to a few 1e-4.  Those two cases are therefore held to TWICE THE
# PLAIN KERNEL'S ERROR against the same oracle, measured in the same test.  MI355X figures, star against plain:
#   workgroup_c29  1.76e-4 against 2.36e-4      workgroup_c80  2.39e-4 against 4.08e-4
# (Before the wildcard cell added its constant to log(sum) first — star_cell in csrc/ctc.hip — they were 1.21e-3 and 2.65e-3: the same
# constant added to a value of alpha's magnitude in every frame is rounded the same way every time, and the error drifted.)
_LONG = ("workgroup_c29", "workgroup_c80")
_PLAIN_CACHE = {}


def _plain_error(case, lattice):
    """rel_l2 of the PLAIN kernel's gradient on the case's logits with the wildcards removed, against the same fp64 oracle."""
    C, T, targets, il, flags, logits, _, _ = _case(case)
    if case not in _PLAIN_CACHE:
        _PLAIN_CACHE[case] = O.loss_and_grad(logits, [[i for i in t if i != C] for t in targets], il, PEN, None, grad_scale=0.125)
    nll_ref, grad_ref = _PLAIN_CACHE[case]
    nll, grad, _ = _run(case, lattice, strip=True, plain=True)
    assert np.allclose(nll.cpu().numpy(), nll_ref, rtol=1e-5, atol=1e-4)
    return rel_l2(grad.cpu().numpy(), grad_ref)


def _check_against_oracle(case, lattice):
    C, T, targets, il, flags, _, nll_ref, grad_ref = _case(case)
    nll, grad, _ = _run(case, lattice)
    nll, grad = nll.cpu().numpy(), grad.cpu().numpy()
    fin = np.isfinite(nll_ref)
    assert np.array_equal(np.isinf(nll) & (nll > 0), ~fin), (case, nll, nll_ref)          # +inf exactly where the oracle is
    err, bar = rel_l2(grad, grad_ref), 1e-4
    print(f"{case} lattice={lattice}: nll max abs err {np.abs(nll[fin] - nll_ref[fin]).max():.3e}, grad rel_l2 {err:.3e}")
    if case in _LONG:
        plain = _plain_error(case, lattice)
        bar = 2 * plain
        print(f"{case} lattice={lattice}: the plain kernel without the wildcards: grad rel_l2 {plain:.3e}; the bar is twice that")
    assert np.allclose(nll[fin], nll_ref[fin], rtol=1e-5, atol=1e-4), (case, nll, nll_ref)
    assert err < bar, (case, err, bar)
    for b in range(len(targets)):
        assert not grad[max(min(il[b], T), 0):, b].any(), (case, b)                        # exactly 0 beyond T_b
        if not fin[b]:
            assert not grad[:, b].any(), (case, b)                                         # and for an infeasible utterance
    return nll, grad


@pytest.mark.parametrize("case,lattice", [("edges_c29", 0), ("edges_c80", 0), ("workgroup_c29", 0), ("workgroup_c80", 0), ("edges_c29", 1)])
def test_against_fp64_oracle(case, lattice):
    nll, grad = _check_against_oracle(case, lattice)
    assert np.isfinite(nll).all()
    C, T, targets, il, flags, _, _, _ = _case(case)
    assert C in targets[-1] and il[-1] == T                                                # the wildcard's address at the allocation's end


@pytest.mark.parametrize("lattice", [0, 1])
def test_infeasible_utterances(lattice):
    """+inf and zero rows for: more labels than frames, T_b = 0, a label C + 1, a label 0; their neighbours equal the oracle."""
    nll, grad = _check_against_oracle("infeasible_c29", lattice)
    assert np.isinf(nll[[1, 2, 3, 5]]).all() and np.isfinite(nll[[0, 4, 7]]).all() and nll[6] == 0.0
    for b in (0, 4, 7):
        assert grad[:, b].any()


def test_optional_tokens_only_add_paths_and_the_penalty_orders_the_loss():
    from asr_amd import ops
    dev = torch.device("cuda:0")
    C, T = 29, 60
    base = [_labels(9, C, 31), _labels(1, C, 32), [3, 3, 4], _labels(20, C, 33)]
    il = [60, 5, 17, 59]
    x = torch.from_numpy(det.unitvar((T, len(base), C), 77) * np.float32(2.0)).to(dev)
    ild = torch.tensor(il, dtype=torch.int32, device=dev)

    def nll_of(targets, flags, pen):
        tg, off, tl, max_u = _device_targets(targets, dev)
        fl = torch.tensor(flags, dtype=torch.int32, device=dev)
        return ops.ctc_star_loss(x, tg, off, ild, tl, max_u, 1.0, star_penalty=pen, flags=fl, want_grad=False)[0].cpu().numpy().astype(np.float64)

    plain = nll_of(base, [0] * 4, PEN)
    free = nll_of([[C] + t for t in base], [1] * 4, PEN)
    tol = 2 * (1e-4 + 1e-5 * np.abs(plain))          # each side is within the kernel's bar (rtol 1e-5, atol 1e-4) of its exact value
    print("plain", plain, "free start", free)
    assert np.isfinite(plain).all() and (free <= plain + tol).all()
    # a wildcard that every path must pass through: each path pays the penalty at least once, so 0 against -3 moves the nll by >= 3
    mid = [t[: len(t) // 2] + [C] + t[len(t) // 2:] for t in base]
    n0, n3 = nll_of(mid, [0] * 4, 0.0), nll_of(mid, [0] * 4, -3.0)
    print("penalty 0", n0, "penalty -3", n3)
    assert np.isfinite(n3).all() and (n0 <= n3 - 3.0 + tol).all()


def test_bad_penalty_is_refused_before_any_launch():
    from asr_amd import _lib, ops
    dev = torch.device("cuda:0")
    x = torch.zeros(4, 1, 5, device=dev)
    tg, off, tl, max_u = _device_targets([[1]], dev)
    ild = torch.tensor([4], dtype=torch.int32, device=dev)
    for bad in (0.25, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(_lib.DS2LibraryError):
            ops.ctc_star_loss(x, tg, off, ild, tl, max_u, 1.0, star_penalty=bad)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_ctcloss_star_through_autograd(reduction):
    """CTCLoss(star=True, free_start=True, free_end=True): backward fills logits.grad with the kernel gradient times the upstream factor."""
    from asr_amd import CTCLoss, ops
    dev = torch.device("cuda:0")
    C, T = 29, 50
    targets = [[4, C, C, 5, 6], [C, 2], [8], [1, 2, 3, C]]
    tl = torch.tensor([len(t) for t in targets])
    il = torch.tensor([50, 20, 9, 33], dtype=torch.int32)
    flat = torch.tensor([i for t in targets for i in t], dtype=torch.int32)
    x = torch.from_numpy(det.unitvar((T, 4, C), 90) * np.float32(2.0)).to(dev).requires_grad_(True)
    crit = CTCLoss(reduction=reduction, star=True, free_start=True, free_end=True, star_penalty=-1.25)
    loss = crit(x, flat, il, tl)
    w = torch.tensor([0.5, -2.0, 3.0, 1.5], device=dev)
    ((loss * w).sum() if reduction == "none" else loss * 2.5).backward()
    # the kernel's own results on the prepared targets
    t_h, off_h, tl_h, max_u, flags_h = crit.prepare_targets(flat, tl, C)
    assert t_h.tolist() == [C, 4, C, 5, 6, C, C, 2, C, C, 8, C, C, 1, 2, 3, C] and flags_h.tolist() == [3, 3, 3, 3]
    nll, grad = ops.ctc_star_loss(x.detach(), t_h.to(dev), off_h.to(dev), il.to(dev), tl_h.to(dev), max_u, 1.0, star_penalty=-1.25,
                                  flags=flags_h.to(dev))
    ref_nll, ref_grad = O.loss_and_grad(x.detach().cpu().numpy(), [t_h[o:o + n].tolist() for o, n in zip(off_h.tolist(), tl_h.tolist())],
                                        il.tolist(), -1.25, flags_h.tolist())
    assert np.allclose(nll.cpu().numpy(), ref_nll, rtol=1e-5, atol=1e-4) and rel_l2(grad.cpu().numpy(), ref_grad) < 1e-4
    if reduction == "none":
        want, up = nll, w
    elif reduction == "sum":
        want, up = nll.sum(), torch.full((4,), 2.5, device=dev)
    else:                                              # the caller's target lengths, not the lengths after the insertion
        want, up = (nll / tl.to(dev)).mean(), 2.5 / tl.to(dev) / 4
    assert torch.allclose(loss.detach(), want, rtol=1e-6, atol=0)
    assert torch.allclose(x.grad, grad * up.view(1, -1, 1), rtol=1e-6, atol=1e-12)
    assert not x.grad[20:, 1].any() and x.grad[:20, 1].any()
