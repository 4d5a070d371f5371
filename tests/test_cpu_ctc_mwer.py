"""No GPU: the fp64 restatement of the minimum-error-rate loss (tests/ctc_mwer_oracle.py) against a brute-force enumeration of the
hypotheses' state paths and against central differences of its own loss; its identities (rows of the gradient sum to 0, one
hypothesis or equal risks give no gradient); what ds2_ctc_mwer_f32 refuses before any HIP call; the workspace size; MWERLoss's
constructor."""
import itertools

import numpy as np
import pytest

import ctc_mwer_oracle as O
import ctc_star_loss_oracle as S

P = 4096                                    # any non-null address: no call below gets as far as reading through it
NAN, INF = float("nan"), float("inf")


def test_oracle_nll_equals_brute_force_and_the_recorded_loss():
    f = O.fixture_a()
    loss, nll, post, grad = O.loss_and_grad(f["logits"], f["hyps"], f["valid"], f["in_lens"], f["risk"])
    worst = 0.0
    for b, k in itertools.product(range(f["B"]), range(f["K"])):
        hyp, Tb = f["hyps"][b][k], f["in_lens"][b]
        if not f["valid"][b][k] or any(v < 1 or v >= f["C"] for v in hyp):
            assert np.isinf(nll[b, k]) and post[b, k] == 0.0
            continue
        want = S.brute_force_nll(S.extended_emissions(f["logits"][:Tb, b], 0.0), hyp, 0)
        if np.isinf(want):
            assert np.isinf(nll[b, k]) and nll[b, k] > 0 and post[b, k] == 0.0, (b, k)
        else:
            worst = max(worst, abs(nll[b, k] - want))
    print(f"oracle nll vs brute force: worst {worst:.2e}")
    assert worst <= 1e-12
    assert np.isinf(nll[1, 3]) and np.isinf(nll[2, 1]) and np.isfinite(np.delete(nll.reshape(-1), [7, 9])).all()
    assert np.abs(loss - f["loss"]).max() <= 5e-9                      # the figures of the issue, 8 decimals
    assert np.abs(post.sum(1) - 1.0).max() <= 1e-12


def test_oracle_gradient_equals_central_differences():
    f = O.fixture_a()
    x = f["logits"]
    _, _, _, grad = O.loss_and_grad(x, f["hyps"], f["valid"], f["in_lens"], f["risk"])
    total = lambda y: O.loss_and_grad(y, f["hyps"], f["valid"], f["in_lens"], f["risk"], want_grad=False)[0].sum()   # noqa: E731
    h, num = 1e-5, np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        num[idx] = (total(xp) - total(xm)) / (2 * h)
    err = np.abs(num - grad).max()
    print(f"oracle gradient vs central differences: {err:.2e} (largest entry {np.abs(grad).max():.3f})")
    assert err <= 1e-7
    assert np.abs(grad).max() > 0.1
    assert not grad[9:, 1].any() and not grad[2:, 2].any()             # rows beyond T_b


def test_gradient_rows_sum_to_zero():
    f = O.fixture_a()
    prior = np.random.default_rng(3).normal(size=f["logits"].shape)
    _, _, _, grad = O.loss_and_grad(f["logits"], f["hyps"], f["valid"], f["in_lens"], f["risk"], grad_scale=0.7)
    assert np.abs(grad.sum(2)).max() <= 1e-14
    _, _, _, acc = O.loss_and_grad(f["logits"], f["hyps"], f["valid"], f["in_lens"], f["risk"], grad_scale=0.7, prior=prior)
    assert np.abs(acc - prior - grad).max() <= 1e-15


def test_single_hypothesis_and_equal_risks_give_no_gradient():
    f = O.fixture_a()
    one = [[h[0], [0], [0], [0]] for h in f["hyps"]]                   # one valid hypothesis per utterance
    valid = [[1, 0, 0, 0]] * 3
    risk = np.array([[2.5, 9, 9, 9], [0.0, 9, 9, 9], [7.0, 9, 9, 9]])
    loss, nll, post, grad = O.loss_and_grad(f["logits"], one, valid, f["in_lens"], risk)
    assert np.allclose(loss, [2.5, 0.0, 7.0], rtol=0, atol=0) and not grad.any()
    assert (post[:, 0] == 1.0).all() and not post[:, 1:].any()
    loss, _, _, grad = O.loss_and_grad(f["logits"], f["hyps"], f["valid"], f["in_lens"], np.full((3, 4), 3.0))
    assert np.abs(loss - 3.0).max() <= 1e-15 and np.abs(grad).max() <= 1e-15
    # no finite slot, and no frames: loss 0, no gradient
    loss, nll, post, grad = O.loss_and_grad(f["logits"][:, :2], [[[0], [5]], [[], [1]]], None, [12, 0], np.ones((2, 2)))
    assert np.isinf(nll[0]).all() and nll[1, 0] == 0.0 and np.isinf(nll[1, 1])
    assert not loss.any() and not grad.any() and not post[0].any()
    # a hypothesis longer than max_hyp_len is infeasible
    _, nll, _, _ = O.loss_and_grad(f["logits"][:, :1], [[[1, 2, 3], [1, 2]]], None, [12], np.ones((1, 2)), max_hyp_len=2)
    assert np.isinf(nll[0, 0]) and np.isfinite(nll[0, 1])


def _lib():
    from asr_amd import _lib
    return _lib.load()


def _ok(lib):
    T, B, C, K, U = 10, 2, 29, 4, 10
    need = lib.ds2_ctc_mwer_workspace_bytes(T, B, K, U)
    assert need > 0
    return dict(logits=P, ld=C, T=T, B=B, C=C, K=K, hyps=P, off=P, lens=P, valid=None, in_lens=P, max_hyp_len=U, risk=P, loss=P, nll=P,
                post=P, grad=P, ldg=C, grad_scale=0.5, accumulate=0, lattice=0, ws=P, wsb=need, stream=None)


def test_entry_refuses_every_single_fault_before_any_launch():
    """Dummy pointers: a call that got as far as a launch would fault.  Fails on a library without the symbol."""
    lib = _lib()
    ok = _ok(lib)
    bad = [dict(logits=None), dict(hyps=None), dict(off=None), dict(lens=None), dict(in_lens=None), dict(risk=None), dict(loss=None),
           dict(nll=None), dict(post=None), dict(ws=None), dict(T=0), dict(T=-1), dict(B=0), dict(B=-1), dict(C=0), dict(C=1), dict(C=-1),
           dict(K=0), dict(K=-1), dict(max_hyp_len=-1), dict(ld=28), dict(ldg=28), dict(accumulate=2), dict(accumulate=-1), dict(lattice=2),
           dict(lattice=-1), dict(grad_scale=NAN), dict(grad_scale=INF), dict(grad_scale=-INF), dict(wsb=ok["wsb"] - 1), dict(wsb=0),
           dict(lattice=1, max_hyp_len=4096, wsb=1 << 40),                  # LDS lattice rows: 2 * 8193 floats
           dict(max_hyp_len=5000, wsb=1 << 40),                             # the same through the launcher's own choice
           dict(C=20000, ld=20000, ldg=20000, wsb=1 << 40)]                 # the gradient's class rows
    for v in bad:
        assert set(v) <= set(ok)
        rc = lib.ds2_ctc_mwer_f32(*dict(ok, **v).values())
        msg = lib.ds2_last_error().decode()
        assert rc != 0 and msg.startswith("ds2_ctc_mwer_f32: "), (v, rc, msg)
    # without a gradient buffer neither its pitch nor the gradient kernel's LDS is asked for ... but the call would launch: not made


def test_workspace_bytes_is_monotone_and_covers_the_lattices():
    lib = _lib()
    base = dict(T=20, B=3, K=4, U=7)
    f = lambda **kw: lib.ds2_ctc_mwer_workspace_bytes(*dict(base, **kw).values())   # noqa: E731
    for name in base:
        sizes = [f(**{name: base[name] + d}) for d in range(0, 40, 3)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (name, sizes)
    assert f() >= 4 * 20 * 3 + 8 * 3 * 4 * 20 * 15
    assert f(T=0) == 0 and f(K=0) == 0 and f(U=-1) == 0 and f(U=0) > 0
    big = lib.ds2_ctc_mwer_workspace_bytes(501, 64, 4, 501)
    assert 1.0e9 < big < 1.1e9                                           # "about 1 GB", as the header says


def test_mwerloss_constructor():
    from asr_amd import BeamCTCDecoder, GreedyDecoder, MWERLoss
    labels = "_abcd "
    dec = BeamCTCDecoder(labels, beam_width=8)
    crit = MWERLoss(dec)
    assert (crit.nbest, crit.ctc_weight, crit.risk, crit.max_hyp_len, crit.reduction, crit.last_nbest) == (4, 0.01, "label", None, "sum", None)
    assert MWERLoss(dec, nbest=8, risk="word", ctc_weight=0).nbest == 8
    for kw in (dict(nbest=9), dict(nbest=0), dict(risk="char"), dict(risk=None), dict(ctc_weight=-0.1), dict(ctc_weight=NAN),
               dict(max_hyp_len=-1), dict(reduction="batchmean")):
        with pytest.raises(ValueError):
            MWERLoss(dec, **kw)
    with pytest.raises(TypeError):
        MWERLoss(GreedyDecoder(labels))
    with pytest.raises(ValueError):
        MWERLoss(BeamCTCDecoder(labels, beam_width=8, blank_index=1))


def test_step_refuses_the_word_risk():
    from types import SimpleNamespace
    from asr_amd import BeamCTCDecoder, MWERLoss
    from asr_amd.trainers import DeepSpeechTrainer
    tr = SimpleNamespace(criterion=MWERLoss(BeamCTCDecoder("_abcd ", beam_width=8), risk="word"))
    with pytest.raises(NotImplementedError, match="synchronisation"):
        DeepSpeechTrainer._prep_targets_step(tr, [1, 2], [2])
