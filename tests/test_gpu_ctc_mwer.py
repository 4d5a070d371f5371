"""-m gpu: the minimum-error-rate loss (ds2_ctc_mwer_f32, ops.ctc_mwer, MWERLoss) against its fp64 restatement
(tests/ctc_mwer_oracle.py), with the bars of tests/test_gpu_ctc_star.py: nll rtol 1e-5 / atol 1e-4, the same bar pushed through the
softmax for the loss, rel_l2 < 1e-4 for the gradient.  MI355X figures are in profiles/ctc_mwer_timing.txt."""
import numpy as np
import pytest
import torch

import ctc_beam_oracle as BO
import ctc_mwer_oracle as O
from helpers import rel_l2

pytestmark = pytest.mark.gpu

_CACHE = {}


def _fixture_b():
    """T = 70, hypotheses of 64 labels (2 * 64 + 1 = 129 states: the workgroup lattice whatever `lattice` says), K = 3; flat logits and
    hypotheses one label apart, so that the posteriors are comparable and the gradient is not all rounding."""
    T, B, C, K = 70, 2, 7, 3
    logits = np.random.default_rng(11).normal(size=(T, B, C)) * 0.5
    seq = [1 + (i % (C - 1)) for i in range(64)]
    a, b = list(seq), list(seq)
    a[10], b[40] = seq[10] % (C - 1) + 1, seq[40] % (C - 1) + 1
    a[11] = a[10]                                                    # a repeated label: 65 frames at least
    hyps = [[seq, a, b], [[2, 2, 5], [], seq[:33]]]
    return dict(T=T, B=B, C=C, K=K, logits=logits, in_lens=[70, 33], hyps=hyps, valid=[[1, 1, 1], [1, 1, 1]],
                risk=np.array([[0.0, 2.0, 1.0], [1.0, 3.0, 30.0]]), max_hyp_len=64)


def _fixture(name):
    if name not in _CACHE:
        f = O.fixture_a() if name == "a" else _fixture_b()
        f.setdefault("max_hyp_len", max(len(h) for u in f["hyps"] for h in u))
        f["logits"] = f["logits"].astype(np.float32)                # what the kernels see
        f["oracle"] = O.loss_and_grad(f["logits"], f["hyps"], f["valid"], f["in_lens"], f["risk"], grad_scale=0.25,
                                      max_hyp_len=f["max_hyp_len"])
        for a in (f["logits"],) + f["oracle"]:
            a.setflags(write=False)
        _CACHE[name] = f
    return _CACHE[name]


def _run(f, lattice=0, prior=None, want_grad=True, slots=None, scale=0.25):
    """ops.ctc_mwer on a fixture (slots: keep these slot indices of every utterance) -> (loss, nll_hyp, post, grad) on the GPU"""
    from asr_amd import ops
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    dev = torch.device("cuda:0")
    slots = list(range(f["K"])) if slots is None else slots
    hyps = [[u[k] for k in slots] for u in f["hyps"]]
    flat = [7, 7, 7] + [i for u in hyps for h in u for i in h]      # (offsets do not start at 0)
    lens = [len(h) for u in hyps for h in u]
    off = np.concatenate([[3], 3 + np.cumsum(lens)[:-1]]).astype(np.int64)
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt, device=dev)          # noqa: E731
    B, K = f["B"], len(slots)
    out = ops.ctc_mwer(torch.from_numpy(f["logits"].copy()).to(dev), t(flat, torch.int32), t(off, torch.int64).view(B, K),
                       t(lens, torch.int32).view(B, K), t(np.asarray(f["valid"])[:, slots], torch.int32).contiguous(),
                       t(f["in_lens"], torch.int32), f["max_hyp_len"], t(f["risk"][:, slots], torch.float32).contiguous(), scale,
                       want_grad=want_grad, grad=prior, lattice=lattice)
    torch.cuda.synchronize()
    return out


def _check_values(what, got, want, risk):
    """nll, +inf pattern, posteriors' support and the loss of (loss, nll_hyp, post, ...) against the oracle's"""
    loss, nll, post = (a.cpu().numpy().astype(np.float64) for a in got[:3])
    wl, wn, wp = want[:3]
    assert (np.isinf(nll) == np.isinf(wn)).all() and (nll[np.isinf(nll)] > 0).all(), (what, nll, wn)
    fin = np.isfinite(wn)
    err_n = np.abs(nll[fin] - wn[fin])
    bar_l = 2.0 * risk.max() * (1e-4 + 1e-5 * np.abs(wn[fin]).max())
    print(f"{what}: nll err {err_n.max():.2e} (largest nll {np.abs(wn[fin]).max():.1f}), loss err {np.abs(loss - wl).max():.2e} "
          f"(bar {bar_l:.2e}), post err {np.abs(post - wp).max():.2e}")
    assert (err_n <= 1e-4 + 1e-5 * np.abs(wn[fin])).all(), what
    assert (np.abs(loss - wl) <= bar_l).all(), what
    assert ((post == 0) == (wp == 0)).all(), what


@pytest.mark.parametrize("name", ["a", "b"])
def test_against_the_oracle(name):
    f = _fixture(name)
    got = _run(f)
    _check_values(f"fixture {name}", got, f["oracle"], f["risk"])
    grad, want = got[3].cpu().numpy(), f["oracle"][3]
    err = rel_l2(grad, want)
    print(f"fixture {name}: gradient rel_l2 {err:.2e}, largest entry {np.abs(want).max():.3e}, row sums {np.abs(grad.sum(2)).max():.2e}")
    assert np.abs(want).max() > 1e-3                                  # (not a comparison of rounding with rounding)
    assert err < 1e-4
    for b, Tb in enumerate(f["in_lens"]):
        assert not grad[Tb:, b].any()                                 # rows beyond T_b are 0, exactly
    if name == "a":
        assert np.abs(f["oracle"][0] - f["loss"]).max() < 1e-6        # (the fp32-rounded logits move the recorded figures this little)


def test_accumulate_adds_to_the_buffer_and_leaves_rows_beyond_the_frames_alone():
    f = _fixture("a")
    prior = torch.from_numpy(np.random.default_rng(5).normal(size=f["logits"].shape).astype(np.float32)).cuda()
    before = prior.clone()
    got = _run(f, prior=prior)
    assert got[3].data_ptr() == prior.data_ptr()
    want = before.cpu().numpy().astype(np.float64) + f["oracle"][3]
    total = rel_l2(got[3].cpu().numpy(), want)
    # ... and what was added alone, against the oracle's gradient (the buffer's own fp32 rounding included)
    added = rel_l2(got[3].cpu().numpy() - before.cpu().numpy().astype(np.float64), f["oracle"][3])
    print(f"accumulate: rel_l2 of the sum {total:.2e}, of the added part {added:.2e}")
    assert total < 1e-4 and added < 1e-4
    for b, Tb in enumerate(f["in_lens"]):
        assert torch.equal(got[3][Tb:, b].view(torch.int32), before[Tb:, b].view(torch.int32))
    same = _run(f)                                                    # accumulate = 0 and the values are the same bits either way
    for a, b in zip(got[:3], same[:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_wave_and_workgroup_lattices_write_the_same_bits():
    f = _fixture("a")
    got0, got1 = _run(f, lattice=0), _run(f, lattice=1)
    for name, a, b in zip(("loss", "nll_hyp", "post", "grad"), got0, got1):
        diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
        print(f"lattice 0 vs 1: {name} differing words: {diff} of {a.numel()}")
        assert diff == 0, name


def test_one_slot_and_three_slots():
    f = _fixture("a")
    loss, nll, post, grad = _run(f, slots=[0])                        # K = 1: the loss is the slot's risk, no gradient
    assert np.isfinite(nll.cpu().numpy()).all()
    assert torch.equal(loss.cpu(), torch.tensor(f["risk"][:, 0], dtype=torch.float32)) and bool((post == 1).all()) and not bool(grad.any())
    slots = [3, 0, 2]                                                 # K = 3, another slot order
    want = O.loss_and_grad(f["logits"], [[u[k] for k in slots] for u in f["hyps"]], np.asarray(f["valid"])[:, slots], f["in_lens"],
                           f["risk"][:, slots], grad_scale=0.25)
    got = _run(f, slots=slots)
    _check_values("K = 3", got, want, f["risk"])
    assert rel_l2(got[3].cpu().numpy(), want[3]) < 1e-4
    # equal risks: every weight is rounding, the gradient nothing next to the one above
    f2 = dict(f, risk=np.full_like(f["risk"], 3.0))
    g2 = _run(f2)[3].cpu().numpy()
    assert np.abs(g2).max() <= 1e-6 * 3.0


def test_without_a_gradient_buffer_only_the_values_are_written():
    f = _fixture("a")
    got = _run(f, want_grad=False)
    assert got[3] is None
    _check_values("no gradient", got, f["oracle"], f["risk"])


# ---- MWERLoss end to end: peaked random posteriors, T = 20, B = 2, C = 6, beam_width 8, nbest 4.  The seed was chosen on the CPU with
# the two oracles: every decision of both beam searches clears 1e-3, and both utterances hold finite hypotheses of different risk.
E2E = dict(seed=3, T=20, B=2, C=6, in_lens=[20, 16])


def _e2e():
    if "e2e" not in _CACHE:
        rng = np.random.default_rng(E2E["seed"])
        x = (rng.normal(size=(E2E["T"], E2E["B"], E2E["C"])) * 3.0).astype(np.float32)
        refs = [[int(v) for v in rng.integers(1, E2E["C"], 6)], [int(v) for v in rng.integers(1, E2E["C"], 4)]]
        e = np.exp(x.astype(np.float64) - x.max(2, keepdims=True))
        p = e / e.sum(2, keepdims=True)
        beams = []
        for b in range(E2E["B"]):
            res = BO.beam_search(p[:, b], E2E["in_lens"][b], 0, 8, 40, 1.0)
            assert BO.decisive(res, 1e-3)
            beams.append([list(bm[0]) for bm in res["beams"][:4]])
        _CACHE["e2e"] = (x, refs, beams)
    return _CACHE["e2e"]


def _criterion(**kw):
    from asr_amd import BeamCTCDecoder, MWERLoss
    return MWERLoss(BeamCTCDecoder("_abcde", beam_width=8), nbest=4, **kw)


def _call(crit, x, refs):
    xt = torch.from_numpy(x.copy()).cuda().requires_grad_(True)
    value = crit(xt, torch.tensor([i for r in refs for i in r], dtype=torch.int32), torch.tensor(E2E["in_lens"], dtype=torch.int32),
                 torch.tensor([len(r) for r in refs], dtype=torch.int32))
    value.sum().backward()
    torch.cuda.synchronize()
    return value.detach(), xt.grad


def test_mwerloss_end_to_end():
    from asr_amd import ops
    from asr_amd.decoders import _edit_distance
    x, refs, beams = _e2e()
    crit = _criterion(ctc_weight=0.0, reduction="none")
    value, grad = _call(crit, x, refs)
    labels, lens, valid, risk, post = (a.cpu().numpy() for a in crit.last_nbest)
    assert labels.shape == (2, 4, 20) and valid.all()
    hyps = [[labels[b, k, :lens[b, k]].tolist() for k in range(4)] for b in range(2)]
    assert hyps == beams                                              # the beam oracle's top 4, in its order
    want_risk = np.array([[_edit_distance(h, refs[b]) for h in hyps[b]] for b in range(2)], np.float64)
    assert (risk == want_risk).all()
    loss, nll, wpost, wgrad = O.loss_and_grad(x, hyps, valid, E2E["in_lens"], want_risk)
    assert np.isfinite(nll).all() and all(len(set(r)) > 1 for r in want_risk.tolist())      # (the gradient test is not vacuous)
    err = rel_l2(grad.cpu().numpy(), wgrad)
    print(f"MWERLoss: value {value.cpu().numpy()} oracle {loss}, post err {np.abs(post - wpost).max():.2e}, gradient rel_l2 {err:.2e}, "
          f"largest entry {np.abs(wgrad).max():.3f}")
    assert (np.abs(value.cpu().numpy() - loss) <= 2.0 * want_risk.max() * (1e-4 + 1e-5 * np.abs(nll).max())).all()
    assert np.abs(wgrad).max() > 0.05 and err < 1e-4
    assert _criterion(ctc_weight=0.0)(torch.from_numpy(x).cuda(), torch.tensor([i for r in refs for i in r]), torch.tensor(E2E["in_lens"]),
                                      torch.tensor([len(r) for r in refs])).item() == pytest.approx(float(value.sum()), rel=1e-6)
    # ctc_weight adds the plain loss's value and gradient at that scale: the same kernels' bits, summed once
    crit5 = _criterion(ctc_weight=0.5, reduction="none")
    value5, grad5 = _call(crit5, x, refs)
    dev = grad.device
    tg = torch.tensor([i for r in refs for i in r], dtype=torch.int32, device=dev)
    tl = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
    off = torch.tensor([0, len(refs[0])], dtype=torch.int32, device=dev)
    il = torch.tensor(E2E["in_lens"], dtype=torch.int32, device=dev)
    nll_ref, g_ref = ops.ctc_loss(torch.from_numpy(x.copy()).to(dev), tg, off, il, tl, 6, 0.5)
    assert torch.equal(value5, torch.add(value, nll_ref, alpha=0.5))
    assert torch.equal(grad5, g_ref + grad)
    assert float((grad5 - grad).abs().max()) > 0.01


def test_mwerloss_word_risk_is_the_decoders_wer():
    x, refs, beams = _e2e()
    crit = _criterion(ctc_weight=0.0, risk="word", reduction="none")
    crit.decoder = type(crit.decoder)("_abcd ", beam_width=8)         # the last class is the space
    value, grad = _call(crit, x, refs)
    dec = crit.decoder
    labels, lens, valid, risk, post = (a.cpu().numpy() for a in crit.last_nbest)
    text = lambda ids: "".join(dec._char(int(i)) for i in ids)       # noqa: E731
    want = [[dec.wer(text(labels[b, k, :lens[b, k]]), text(refs[b])) for k in range(4)] for b in range(2)]
    assert risk.tolist() == want and np.isfinite(value.cpu().numpy()).all()
