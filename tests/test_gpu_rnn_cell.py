"""-m gpu: the Elman (tanh) cell, rnn_type="nn.RNN", on the gfx950 recurrence kernels (gates = 1).
Kernel level against the fp64 restatement (tests/tanh_rnn_oracle.py), persistent and step kernel families bit for bit; model level against
the reference's golden vectors (tests/golden/make_golden_rnn.py) and the fp64 restatement; full-size properties at c3's and C2's shapes."""
import os
import tempfile

import numpy as np
import pytest
import torch

from helpers import rel_l2, subsample
import det
import tanh_rnn_oracle as R
from oracle import ds2_oracle as O
from test_gpu_model import grad_check, make_model

pytestmark = pytest.mark.gpu
TOL = 1e-3
DEV = "cuda:0"


def _t(seed, *shape):
    return torch.from_numpy(det.unitvar(shape, seed))


def _ragged(B, T, seed):
    lens = sorted([int(v) for v in det.randint((B,), seed, 1, T + 1)], reverse=True)
    lens[0] = T
    if B > 2:
        lens[-1] = 1                                            # a one-frame sample
    return lens


def _layer(H, B, T, lens, mode):
    """one bidirectional tanh layer through ops.rnn_fwd / rnn_bwd (gates = 1): (h (T,B,2,H), dGx (T,B,2,H), rnn_last_path bits) on cuda:0"""
    from asr_amd import ops
    k = 1.0 / H ** 0.5
    gx = (_t(31, T, B, 2, H) * 0.8).float()
    whh = torch.from_numpy(det.uniform((2, H, H), 32, -k, k))
    bhh = torch.from_numpy(det.uniform((2, H), 33, -k, k))
    dy = _t(34, T, B, H).float()
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    gxd = gx.reshape(T * B, 2 * H).to(DEV).contiguous()
    wpf, wpb = ops.rnn_pack(1, whh.to(DEV).contiguous(), bf16=mode)
    hbuf, aux = ops.rnn_fwd(1, gxd, wpf, bhh.to(DEV).contiguous(), ld, T, B, H, bf16=mode)
    assert aux is None
    assert torch.equal(gxd.cpu(), gx.reshape(T * B, 2 * H))      # the forward leaves the x-projections alone
    path = ops.rnn_last_path() & 1
    ops.rnn_bwd(1, dy.reshape(T * B, H).to(DEV), gxd, None, hbuf, wpb, ld, T, B, H, bf16=mode)
    path |= ops.rnn_last_path() & 2
    torch.cuda.synchronize()
    ops.rnn_persistent_check()
    return hbuf.view(T, B, 2, H).cpu(), gxd.view(T, B, 2, H).cpu(), path, (gx, whh, bhh, dy)


def _reference(H, B, T, lens, ops_in):
    gx, whh, bhh, dy = (t.double() for t in ops_in)
    gx.requires_grad_(True)
    lt = torch.tensor(lens, dtype=torch.int32)
    yf = R.tanh_direction(gx[:, :, 0], whh[0], bhh[0], lt, False)
    yb = R.tanh_direction(gx[:, :, 1], whh[1], bhh[1], lt, True)
    ((yf + yb) * dy).sum().backward()
    return yf.detach(), yb.detach(), gx.grad


CASES = [(16, 1, 9), (16, 5, 40), (256, 16, 60), (256, 64, 33), (768, 5, 50), (768, 64, 40), (1024, 16, 48), (1024, 64, 40)]


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16", "split"])
@pytest.mark.parametrize("H,B,T", CASES)
def test_tanh_layer_vs_fp64_and_persistent_vs_step(H, B, T, mode):
    """h and dGx of one bidirectional layer against the fp64 restatement (fp32 modes 2e-5 / 5e-5, bf16 operands 2e-2 / 5e-2 — the bars of
    test_gpu_kernels.py::test_rnn_fwd_bwd); rows beyond each length are exact zeros; both recurrences run as persistent launches, and the
    one-launch-per-step kernels give the same bits (the split mode's step fallback is the fp32 kernels: ~1e-6, not bitwise)."""
    from asr_amd import ops
    lens = _ragged(B, T, 30 + H + B)
    hb, dgx, path, ins = _layer(H, B, T, lens, mode)
    yf, yb, dgx_ref = _reference(H, B, T, lens, ins)
    e1, e2 = (2e-2, 5e-2) if mode == 1 else (2e-5, 5e-5)
    assert rel_l2(hb[:, :, 0], yf) < e1 and rel_l2(hb[:, :, 1], yb) < e1
    assert rel_l2(dgx, dgx_ref) < e2
    pad = torch.arange(T).view(T, 1) >= torch.tensor(lens).view(1, B)
    assert int(torch.count_nonzero(hb[pad])) == 0 and int(torch.count_nonzero(dgx[pad])) == 0
    assert path == 3, f"both recurrences should have run as persistent launches (last_path bits {path})"
    ops.rnn_persistent_enable(False, False)
    try:
        hb_s, dgx_s, path_s, _ = _layer(H, B, T, lens, mode)
    finally:
        ops.rnn_persistent_enable(True, True)
    assert path_s == 0
    if mode == 2:
        assert rel_l2(hb_s, hb) < 1e-5 and rel_l2(dgx_s, dgx) < 1e-5
    else:
        assert torch.equal(hb_s, hb) and torch.equal(dgx_s, dgx)


def test_tanh_layer_bf16_training_buffers():
    """The bf16 training mode's buffers for gates = 1: bf16 x-projections in, no gate record, dGx into the bf16 side buffer with gx = None,
    the bias partial sums of the persistent backward -> db_ih = db_hh = column sums of dGx."""
    from asr_amd import ops
    H, B, T = 256, 16, 50
    lens = _ragged(B, T, 77)
    k = 1.0 / H ** 0.5
    gx = (_t(31, T * B, 2 * H) * 0.8).float().to(DEV)
    whh = torch.from_numpy(det.uniform((2, H, H), 32, -k, k)).to(DEV)
    bhh = torch.from_numpy(det.uniform((2, H), 33, -k, k)).to(DEV)
    dy = _t(34, T * B, H).float().to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    wpf, wpb = ops.rnn_pack(1, whh, bf16=True)
    h_bf = torch.empty(T * B, 2 * H, dtype=torch.bfloat16, device=DEV)
    hbuf, aux, rec = ops.rnn_fwd(1, gx.bfloat16(), wpf, bhh, ld, T, B, H, bf16=True, packed_gates=True, h_bf16=h_bf)
    assert aux is None and rec is None and ops.rnn_last_path() & 1
    hb_ref, _ = ops.rnn_fwd(1, gx.bfloat16().float(), wpf, bhh, ld, T, B, H, bf16=True)
    assert torch.equal(hbuf, hb_ref) and torch.equal(h_bf, hbuf.bfloat16())
    side = torch.empty(T * B, 2 * H, dtype=torch.bfloat16, device=DEV)
    part = torch.empty(B, 2, 4, H, dtype=torch.float32, device=DEV)
    ops.rnn_bwd(1, dy, None, None, hbuf, wpb, ld, T, B, H, bf16=True, dgx_bf16=side, bias_part=part)
    assert ops.rnn_last_path() & 2 and not ops.rnn_last_path() & 4       # persistent, all-gather (no K-split kernel for the tanh cell)
    dgx32 = gx.clone()
    ops.rnn_bwd(1, dy, dgx32, None, hbuf, wpb, ld, T, B, H, bf16=True)
    assert torch.equal(side, dgx32.bfloat16())
    dbih, dbhh = torch.empty(2 * H, device=DEV), torch.empty(2, H, device=DEV)
    ops.rnn_bias_grads(1, part, dbih, dbhh)
    ref = dgx32.double().sum(0)
    assert rel_l2(dbih.cpu(), ref.cpu()) < 1e-5 and torch.equal(dbih.view(2, H), dbhh)
    torch.cuda.synchronize()
    ops.rnn_persistent_check()


# ---- model level --------------------------------------------------------------------------------------------------------------------

RNN_FIXTURES = ["rnn_h32_l2", "rnn_h48_l3"]


def _fixture(name):
    from helpers import load_model_fixture
    z, cfg = load_model_fixture(name)
    return z, cfg, R.model_inputs(cfg)


@pytest.mark.parametrize("name", RNN_FIXTURES)
def test_fit_matches_reference_golden(name):
    """fit() + loss.backward() over 3 AdamW steps, fp32 mode, against the reference's goldens at 1e-3; then eval-mode probabilities."""
    from asr_amd import CTCLoss
    from asr_amd.trainers import DeepSpeechTrainer
    z, cfg, (sd, x, targets, pct, tsz) = _fixture(name)
    model = make_model(cfg, sd)
    assert model._cfg.gates == 1
    opt = torch.optim.AdamW(model.parameters(), lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, "cuda", "cuda", False, None)
    losses = []
    for step in range(3):
        valid, loss, lv = tr.fit((x, targets, pct.clone(), tsz))
        assert valid
        opt.zero_grad()
        loss.backward()
        if step == 0:
            for k, p in model.named_parameters():
                grad_check(k, p.grad.cpu().numpy(), z["grad_" + k], z["gradnorm_" + k])
            for k, v in model.state_dict().items():
                if "running_" in k:
                    assert np.allclose(v.cpu().numpy(), z["buf_" + k], rtol=1e-3, atol=1e-5), k
        opt.step()
        losses.append(lv)
    assert np.allclose(losses, z["losses"], rtol=TOL), (losses, z["losses"])
    for k, p in model.named_parameters():
        assert rel_l2(subsample(p.detach().cpu().numpy()), z["final_" + k]) < TOL, k
    model.eval()
    with torch.no_grad():
        probs, _ = model.forward(x.cuda(), O.lengths_from_percentages(pct, x.size(3)))
    assert rel_l2(probs.cpu().numpy(), z["eval_probs"]) < TOL


@pytest.mark.parametrize("name", RNN_FIXTURES)
def test_fused_step_matches_reference_golden(name):
    """trainer.step() (no autograd, FusedAdamW): step-0 logits, the 3-step loss curve and the final weights of the reference at 1e-3."""
    from asr_amd import CTCLoss, FusedAdamW
    from asr_amd.trainers import DeepSpeechTrainer
    z, cfg, (sd, x, targets, pct, tsz) = _fixture(name)
    model = make_model(cfg, sd)
    with torch.no_grad():
        logits, out_lens = model.forward(x.cuda(), O.lengths_from_percentages(pct, x.size(3)))
    assert np.array_equal(out_lens.numpy(), z["output_sizes"])
    assert rel_l2(logits.cpu().numpy(), z["logits"]) < TOL
    model = make_model(cfg, sd)
    opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, "cuda", "cuda", False, None)
    losses = []
    for _ in range(3):
        valid, lv = tr.step((x, targets, pct.clone(), tsz))
        assert valid
        losses.append(lv)
    assert np.allclose(losses, z["losses"], rtol=TOL), (losses, z["losses"])
    for k, p in model.named_parameters():
        assert rel_l2(subsample(p.detach().cpu().numpy()), z["final_" + k]) < TOL, k
    sd_saved = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    again = make_model(cfg, sd_saved)                          # state_dict round trip: same keys, same eval output
    model.eval()
    again.eval()
    with torch.no_grad():
        lens = O.lengths_from_percentages(pct, x.size(3))
        assert torch.equal(model.forward(x.cuda(), lens)[0], again.forward(x.cuda(), lens)[0])


def test_evaluate_decodes_with_the_tanh_cell():
    """evaluate(): eval forward -> softmax -> greedy decode; the probabilities equal the fp64 restatement's eval forward at 1e-3 and the
    transcripts are the greedy decode of the restatement where its top-2 margin is decisive."""
    cfg = dict(rnn="rnn", hidden=40, layers=2, classes=29, t_ins=[140, 120, 90, 33], seed=1)
    sd, x, targets, pct, tsz = R.model_inputs(cfg)
    model = make_model(cfg, sd)
    model.eval()
    lens = O.lengths_from_percentages(pct, x.size(3))
    probs_ref, out_lens = R.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.double(), lens, training=False)
    with torch.no_grad():
        probs, _ = model.forward(x.cuda(), lens)
    assert rel_l2(probs.cpu().numpy(), probs_ref.numpy()) < TOL
    report = os.path.join(tempfile.mkdtemp(), "eval.txt")
    wer, cer, output_data = model.evaluate(loader=[(x, targets, pct.clone(), tsz)], device="cuda", output_file=report)
    assert np.isfinite(wer) and np.isfinite(cer)
    pe, out_sizes, target_strings = output_data[0]
    assert np.array_equal(np.asarray(out_sizes), np.asarray(out_lens)) and rel_l2(pe, probs_ref.numpy()) < TOL
    dec = model.decoder
    strings, _ = dec.decode(torch.from_numpy(pe).cuda(), torch.as_tensor(out_sizes))
    pr = probs_ref.numpy()
    for b in range(x.size(0)):
        n = int(out_sizes[b])
        path = np.argmax(pe[b, :n], axis=1)
        top2 = np.sort(pr[b, :n], axis=1)[:, -2:]
        if (top2[:, 1] - top2[:, 0]).min() > 1e-4:                              # decisive frames: restatement path == HIP path
            assert np.array_equal(path, np.argmax(pr[b, :n], axis=1))
        want = "".join(dec.int_to_char[int(k)] for t, k in enumerate(path) if k != 0 and (t == 0 or k != path[t - 1]))
        assert strings[b][0] == want


BF16_CASES = [(256, 3, 8, 500), (1024, 5, 16, 400)]


@pytest.mark.parametrize("hidden,layers,B,tmax", BF16_CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_vs_fp64_restatement(hidden, layers, B, tmax, precision):
    """Shapes the goldens do not cover (3x256 B = 8, 5x1024 B = 16, T_in 250-500): logits, loss and every gradient against the fp64
    restatement — fp32 mode at 1e-3; bf16 mode at the bars test_gpu_model.py::test_bf16_precision_vs_oracle states for the GRU (logits /
    loss 2e-2, recurrent and fc gradients 4e-2, conv-stack gradients 3 sqrt(f) from the counted Hardtanh branch flips, floor 4e-2)."""
    from asr_amd import CTCLoss
    cfg = dict(rnn="rnn", hidden=hidden, layers=layers, classes=29)
    t_ins = sorted([int(v) for v in det.randint((B,), 63, tmax // 2, tmax + 1)], reverse=True)
    t_ins[0] = tmax
    cfg["t_ins"], cfg["seed"] = t_ins, 1
    sd, x, targets, pct, tsz = R.model_inputs(cfg)
    ref = R.fit_and_grads(sd, x, targets, pct, tsz, dtype=torch.float64)
    model = make_model(cfg, sd)
    model.precision = precision
    lens = O.lengths_from_percentages(pct, x.size(3))
    out, out_lens = model.forward(x.cuda(), lens)
    loss = CTCLoss(reduction="sum")(out.transpose(0, 1), targets, out_lens, tsz) / B
    loss.backward()
    e_logits = rel_l2(out.detach().cpu().numpy(), ref["logits"].numpy())
    e_loss = abs(float(loss.detach()) - ref["loss"]) / ref["loss"]
    errs = {k: np.linalg.norm(p.grad.cpu().numpy().astype(np.float64) - ref["grads"][k].numpy()) / max(np.linalg.norm(ref["grads"][k].numpy()), 1e-12)
            for k, p in model.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{layers}x{hidden} tanh B={B} {precision}: logits {e_logits:.2e} loss {e_loss:.2e} worst grad {worst[1]:.2e} ({worst[0]})")
    if precision == "fp32":
        assert e_logits < TOL and e_loss < TOL
        for k, e in errs.items():
            assert e <= TOL, (k, e)
        return
    assert 1e-5 < e_logits < 2e-2, e_logits
    assert e_loss < 2e-2, e_loss
    from helpers import hardtanh_flip_fraction
    f = hardtanh_flip_fraction(model, x, pct)
    tol_conv = max(3.0 * f ** 0.5, 4e-2)
    assert tol_conv <= 1.5e-1, f
    for k, e in errs.items():
        assert e <= (tol_conv if k.startswith("conv.") else 4e-2), (k, e)


FULL = [("c3", 1024, 64, 300, True), ("C2", 768, 32, 400, False)]


@pytest.mark.parametrize("name,hidden,B,tlo,bf16", FULL, ids=[f[0] for f in FULL])
def test_full_size_tanh(name, hidden, B, tlo, bf16):
    """c3's shape with the cell swapped (5x1024 BiRNN, B = 64, T_in = 1001, bf16 training mode) and C2's (5x768, B = 32, fp32 mode): both
    recurrences ran as persistent launches, exact zeros beyond each length in every layer's h, a finite loss that decreases over 3 fused
    steps, and two runs from the same state bit-identical."""
    from asr_amd import CTCLoss, FusedAdamW, engine, ops
    from asr_amd.trainers import DeepSpeechTrainer
    cfg = dict(rnn="rnn", hidden=hidden, layers=5, classes=29)
    tmax = 1001
    t_ins = sorted([int(v) for v in det.randint((B,), 64, tlo, tmax + 1)], reverse=True)
    t_ins[0] = tmax
    torch.manual_seed(0)
    model = make_model(cfg)
    x, targets, pct, tsz = map(torch.from_numpy, det.batch(B, t_ins, 29, seed=3))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    runs, paths = [], []
    for _ in range(2):
        model.load_state_dict(sd0)
        opt = FusedAdamW(model, lr=3e-4)
        tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, "cuda", "cuda", bf16, None)
        assert model.precision == ("bf16" if bf16 else "fp32")
        ls = []
        for _ in range(3):
            valid, lv = tr.step((x, targets, pct.clone(), tsz))
            tr.synchronize()
            assert valid
            ls.append(lv)
            paths.append(ops.rnn_last_path())
        flat, flat_grad = model.flat_parameters()
        assert bool(torch.isfinite(flat_grad).all()) and bool(torch.isfinite(flat).all())
        runs.append((ls, flat.clone()))
    print(name, "losses", runs[0][0], "last_path", paths)
    assert all(p & 3 == 3 for p in paths), paths
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][0][0]) and runs[0][0][-1] < runs[0][0][0], runs[0][0]
    model.load_state_dict(sd0)
    lens = O.lengths_from_percentages(pct, tmax)
    out_lens = O.seq_lens_after_conv(lens)
    W = model._flat.tensors(model)
    with torch.no_grad():
        logits, ctx = engine.forward(W, model._cfg, x.cuda(), out_lens.cuda(), training=True, save=True)
    T = logits.shape[0]
    tmask = (torch.arange(T).view(T, 1) >= out_lens.view(1, B)).cuda()
    for lc in ctx.layers:
        assert lc.aux is None and lc.rec is None
        assert float(lc.hbuf.view(T, B, -1)[tmask].abs().max()) == 0.0
    model.precision = "fp32"
