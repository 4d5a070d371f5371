"""No GPU: the fp64 restatement of the word / character confidences (tests/ctc_conf_oracle.py) against a brute-force enumeration of all
frame labelings; the planted case; logconf <= 0; the unit builder; what ds2_ctc_conf_f32 refuses before any HIP call, its ctypes
signature and workspace; the new method signatures."""
import inspect
import os
import re

import numpy as np
import pytest

import ctc_conf_oracle as O
import ctc_star_loss_oracle as S

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
P = 4096                                    # any non-null address: no call below gets as far as reading through it


def _log_probs(rng, T, C):
    return S.log_softmax(rng.normal(size=(T, C)) * 1.5)


def test_oracle_equals_brute_force_enumeration():
    """Every window placement of every label range of random hypotheses with repeated labels, T <= 6, C = 3."""
    rng = np.random.default_rng(7)
    worst, feasible, impossible, zero = 0.0, 0, 0, 0
    for T, y in ((3, [1]), (4, [1, 2]), (4, [1, 1]), (5, [2, 2, 1]), (5, [1, 2]), (6, [1, 2, 2]), (6, [2, 1, 2]), (6, [1, 1, 1]), (6, [2])):
        lp = _log_probs(rng, T, 3)
        em = np.concatenate([lp, np.zeros((T, 1))], axis=1)
        lat = S.lattice(em, y)
        U = len(y)
        for lo, hi in ((a, b) for a in range(U) for b in range(a + 1, U + 1)):
            for ts, te in ((a, b) for a in range(T) for b in range(a + 1, T + 1)):
                num, A, Bq = O.unit_terms(em, y, lo, hi, ts, te, lat)
                got = O.unit_logconf(num, A, Bq)
                joint, ctx = O.brute_force(lp, y, lo, hi, ts, te)
                if ctx == -np.inf:
                    assert np.isnan(got), (T, y, lo, hi, ts, te, got)
                    impossible += 1
                elif joint == -np.inf:
                    assert got == -np.inf, (T, y, lo, hi, ts, te, got)
                    zero += 1
                else:
                    assert np.isfinite(got) and got <= 0.0
                    worst = max(worst, abs(got - (joint - ctx)), abs(num - joint), abs((A + Bq) - ctx))
                    feasible += 1
    print(f"oracle vs enumeration: worst {worst:.2e} over {feasible} feasible cases; {impossible} impossible contexts, {zero} zeros")
    assert worst <= 1e-12
    assert feasible > 200 and impossible > 100 and zero > 10


def test_planted_case_gives_1_and_a_quarter():
    p, y, units, want = O.planted()
    with np.errstate(divide="ignore"):
        logits = np.log(p)[:, None, :]
    nll, lc, _ = O.confidence(logits, [y], [7], [units])
    assert abs(nll[0] - -np.log(0.25)) <= 1e-12
    assert np.abs(np.exp(lc[0]) - want).max() <= 1e-12
    # the window-free wildcard ratio is not this number: the word's own window matters.  A window that leaves the word out is a zero
    _, lc, _ = O.confidence(logits, [y], [7], [[(2, 3, 2, 4)]])
    assert lc[0, 0] == -np.inf or np.isnan(lc[0, 0])


def test_logconf_is_never_positive_and_fixtures_hold_their_patterns():
    for f in (O.fixture_a(), O.fixture_b()):
        nll, lc, mag = O.confidence(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], max_hyp_len=f["max_hyp_len"])
        fin = np.isfinite(lc)
        assert (lc[fin] <= 0.0).all() and fin.sum() >= 6 and (mag[fin] > 0).all()
    f = O.fixture_a()
    nll, lc, _ = O.confidence(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], max_hyp_len=f["max_hyp_len"])
    assert np.isfinite(nll[0]) and nll[1] == np.inf and nll[2] > 0 and np.isfinite(nll[2])
    assert np.isfinite(lc[0, :12]).all() and lc[0, 12] == -np.inf
    assert np.isnan(lc[0, 13:]).all()                                     # impossible contexts, invalid units, slots beyond n_units
    assert np.isnan(lc[1, 0]) and lc[1, 1] == -np.inf and np.isnan(lc[1, 2:]).all() and np.isnan(lc[2]).all()
    # the whole hypothesis in the whole utterance: nothing is given, the confidence is the hypothesis's own probability
    assert abs(lc[0, 7] + nll[0]) <= 1e-12
    # a count outside [0, W_max] voids the utterance; a bad label and an overlong hypothesis do too
    _, lc, _ = O.confidence(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], n_units=[26, -1, 1])
    assert np.isnan(lc[:2]).all()
    nll, lc, _ = O.confidence(f["logits"], [[1, 5, 2], [1], []], f["in_lens"], [[(0, 1, 0, 3)], [(0, 1, 0, 7)], []], 2, max_hyp_len=2)
    assert nll[0] == np.inf and np.isnan(lc[0]).all() and abs(lc[1, 0] + nll[1]) <= 1e-12
    f = O.fixture_b()
    _, lc, _ = O.confidence(f["logits"], f["hyps"], f["in_lens"], f["units"], f["w_max"], max_hyp_len=64)
    assert np.isfinite(lc[0, :2]).all() and np.isnan(lc[0, 2]) and np.isfinite(lc[0, 3:]).all() and np.isfinite(lc[1, :2]).all()


def test_unit_builder():
    from asr_amd.decoders import confidence_units
    text = " ab  c "
    spans = [(0, 1), (2, 4), (4, 5), (6, 7), (7, 8), (9, 11), (11, 12)]
    assert confidence_units(text, spans, 12) == [("ab", 1, 3, 2, 5), ("c", 5, 6, 9, 11)]
    assert confidence_units(text, spans, 12, margin=2) == [("ab", 1, 3, 0, 7), ("c", 5, 6, 7, 12)]
    assert confidence_units(text, spans, 12, margin=100) == [("ab", 1, 3, 0, 12), ("c", 5, 6, 0, 12)]
    chars = confidence_units(text, spans, 12, unit="char", margin=1)
    assert len(chars) == 7 and chars[0] == (" ", 0, 1, 0, 2) and chars[2] == ("b", 2, 3, 3, 6) and chars[6] == (" ", 6, 7, 10, 12)
    assert confidence_units("", [], 5) == [] and confidence_units("  ", [(0, 1), (1, 2)], 5) == []
    for kw in (dict(unit="token"), dict(margin=-1), dict(margin=0.5), dict(margin=True)):
        with pytest.raises(ValueError):
            confidence_units(text, spans, 12, **kw)
    with pytest.raises(ValueError):
        confidence_units("abc", spans, 12)


def _lib():
    from asr_amd import _lib
    return _lib.load()


def _ok(lib):
    T, B, C, U, W = 10, 2, 29, 10, 4
    need = lib.ds2_ctc_conf_workspace_bytes(T, B, U)
    assert need > 0
    return dict(logits=P, ld=C, T=T, B=B, C=C, hyps=P, off=P, lens=P, in_lens=P, max_hyp_len=U, n_units=P, lo=P, hi=P, ws_=P, we=P, W=W,
                nll=P, logconf=P, lattice=0, ws=P, wsb=need, stream=None)


def test_entry_refuses_every_single_fault_before_any_launch():
    """Dummy pointers: a call that got as far as a launch would fault.  Fails on a library without the symbol."""
    lib = _lib()
    ok = _ok(lib)
    bad = [dict(logits=None), dict(hyps=None), dict(off=None), dict(lens=None), dict(in_lens=None), dict(n_units=None), dict(lo=None),
           dict(hi=None), dict(ws_=None), dict(we=None), dict(nll=None), dict(logconf=None), dict(ws=None), dict(T=0), dict(T=-1), dict(B=0),
           dict(B=-1), dict(C=0), dict(C=1), dict(C=-1), dict(W=0), dict(W=-1), dict(max_hyp_len=-1), dict(ld=28), dict(lattice=2),
           dict(lattice=-1), dict(wsb=ok["wsb"] - 1), dict(wsb=0), dict(B=65536, wsb=1 << 40),
           dict(lattice=1, max_hyp_len=4096, wsb=1 << 40),                  # LDS lattice rows: 2 * 8193 floats
           dict(max_hyp_len=5000, wsb=1 << 40)]                             # the same through the launcher's own choice
    for v in bad:
        assert set(v) <= set(ok)
        rc = lib.ds2_ctc_conf_f32(*dict(ok, **v).values())
        msg = lib.ds2_last_error().decode()
        assert rc != 0 and msg.startswith("ds2_ctc_conf_f32: "), (v, rc, msg)


def test_signature_workspace_and_limit():
    from asr_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    for name in ("ds2_ctc_conf_f32", "ds2_ctc_conf_workspace_bytes", "ds2_ctc_conf_max_unit_labels"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["ds2_ctc_conf_f32"][1]) == 22
    assert lib.ds2_ctc_conf_max_unit_labels() == 63 == O.MAX_UNIT_LABELS
    base = dict(T=20, B=3, U=7)
    f = lambda **kw: lib.ds2_ctc_conf_workspace_bytes(*dict(base, **kw).values())   # noqa: E731
    for name in base:
        sizes = [f(**{name: base[name] + d}) for d in range(0, 40, 3)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (name, sizes)
    assert f() >= 4 * 20 * 3 + 8 * 3 * 20 * 15
    assert f(T=0) == 0 and f(B=0) == 0 and f(U=-1) == 0 and f(U=0) > 0


def test_method_signatures_and_constructor():
    from asr_amd import CTCConfidence, DeepSpeech, ops
    assert list(inspect.signature(ops.ctc_confidence).parameters) == [
        "logits", "hyps_dev", "hyp_off_dev", "hyp_lens_dev", "in_lens_dev", "max_hyp_len", "n_units", "unit_lo", "unit_hi", "win_start",
        "win_end", "lattice"]
    assert inspect.signature(ops.ctc_confidence).parameters["lattice"].default == 0
    sig = inspect.signature(CTCConfidence.score)
    assert list(sig.parameters) == ["self", "probs", "sizes", "texts", "is_log", "unit", "margin"]
    assert (sig.parameters["is_log"].default, sig.parameters["unit"].default, sig.parameters["margin"].default) == (False, "word", 0)
    sig = inspect.signature(DeepSpeech.confidence)
    assert list(sig.parameters) == ["self", "inputs", "input_sizes", "decoder", "unit", "margin"]
    assert (sig.parameters["decoder"].default, sig.parameters["unit"].default, sig.parameters["margin"].default) == (None, "word", 0)
    long_, base = inspect.signature(DeepSpeech.confidence_long), inspect.signature(DeepSpeech.transcribe_long)
    assert list(long_.parameters) == list(base.parameters) + ["unit", "margin"]
    assert all(long_.parameters[k].default == v.default for k, v in base.parameters.items())
    with pytest.raises(ValueError):
        CTCConfidence("_ab ", blank_index=1)
    c = CTCConfidence("_ab ")
    for kw in (dict(unit="token"), dict(margin=-1)):
        with pytest.raises(ValueError):
            c.score(np.zeros((1, 2, 4), np.float32), None, ["a"], **kw)
