"""CPU: the Elman (tanh) cell, rnn_type="nn.RNN" — the fp64 restatement (tests/tanh_rnn_oracle.py) against golden vectors of the unmodified
reference (tests/golden/make_golden_rnn.py), the model's cell configuration, and the library's size queries for gates = 1."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import load_model_fixture, noise_only_grads, rel_l2, subsample
import tanh_rnn_oracle as R

RNN_FIXTURES = ["rnn_h32_l2", "rnn_h48_l3"]


@pytest.mark.parametrize("name", RNN_FIXTURES)
def test_restatement_matches_reference_golden(name):
    """logits, loss and every gradient of step 0 to the fp32 floor (the reference runs in fp32, the restatement in fp64)."""
    z, cfg = load_model_fixture(name)
    sd, x, targets, pct, tsz = R.model_inputs(cfg)
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith("rnns.0.rnn.")}["rnns.0.rnn.weight_hh_l0"] == (cfg["hidden"], cfg["hidden"])
    res = R.fit_and_grads(sd, x, targets, pct, tsz, dtype=torch.float64)
    assert np.array_equal(res["input_sizes"].numpy(), z["input_sizes"])
    assert np.array_equal(res["out_lens"].numpy(), z["output_sizes"])
    assert rel_l2(res["logits"].numpy(), z["logits"]) < 2e-5
    assert abs(res["loss"] - z["losses"][0]) / z["losses"][0] < 1e-5
    assert set(res["grads"]) == {k[len("grad_"):] for k in z.files if k.startswith("grad_")}
    for k, g in res["grads"].items():
        if k in noise_only_grads(cfg):
            continue
        ref, nrm = z["grad_" + k].astype(np.float64), float(z["gradnorm_" + k])
        err = np.linalg.norm(subsample(g.numpy()) - ref)
        assert err <= 2e-4 * max(np.linalg.norm(ref), 1e-6 * max(nrm, 1e-30)) + 1e-9, (k, err, np.linalg.norm(ref))
        gn = float((g ** 2).sum().sqrt())
        assert abs(gn - nrm) <= 2e-4 * nrm + 1e-9, (k, gn, nrm)


def test_deepspeech_maps_nn_rnn_to_the_tanh_cell():
    """DeepSpeech(rnn_type="nn.RNN", bidirectional=True) configures the one-gate cell of the HIP recurrence (not "unsupported"), with the
    reference's state_dict keys and shapes."""
    from test_gpu_model import make_model
    cfg = dict(rnn="nn.RNN", hidden=32, layers=2, classes=7)
    model = make_model(cfg, device="cpu")
    assert model._cfg.rnn == "rnn" and model._cfg.gates == 1
    assert isinstance(model.rnns[0].rnn, torch.nn.RNN) and model.rnns[0].rnn.nonlinearity == "tanh"
    shapes = R.state_shapes(32, 2, 7)
    assert list(model.state_dict().keys()) == list(shapes.keys())
    assert all(tuple(v.shape) == tuple(shapes[k]) for k, v in model.state_dict().items())
    for rnn_type, gates in (("nn.GRU", 3), ("nn.LSTM", 4), ("rnn", 1), ("RNN", 1)):
        assert make_model(dict(cfg, rnn=rnn_type), device="cpu")._cfg.gates == gates


def _lib():
    from asr_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("H", [16, 256, 768, 1024, 1280])
def test_library_sizes_for_one_gate(H):
    """ds2_rnn_packed_bytes / ds2_rnn_*_workspace_bytes for gates = 1: the packed W_hh operands are the one-gate fragment sets (a third of the
    GRU's), the split forms carry no ten-unit-slice operand, and the backward workspace holds the carry, the step kernels' ping-pong
    buffers and the persistent kernels' four exchange buffers over the H-wide dGh."""
    lib = _lib()
    nsl = (H + 15) // 16
    for bf16, kc in ((0, 16), (1, 32)):
        assert lib.ds2_rnn_packed_bytes(1, H, 0, bf16) == 2 * nsl * ((H + kc - 1) // kc) * 1024
        assert lib.ds2_rnn_packed_bytes(1, H, 1, bf16) == 2 * nsl * ((H + kc - 1) // kc) * 1024
        assert 3 * lib.ds2_rnn_packed_bytes(1, H, 0, bf16) == lib.ds2_rnn_packed_bytes(3, H, 0, bf16)
    for which in (0, 1):
        assert lib.ds2_rnn_packed_bytes(1, H, which, 2) == lib.ds2_rnn_packed_bytes(1, H, which, 0) + 2 * lib.ds2_rnn_packed_bytes(1, H, which, 1)
    for B in (1, 5, 16, 64):
        nbt16 = (B + 31) // 32 * 2
        for bf16 in (0, 1, 2):
            kc = 32 if bf16 == 1 else 16
            step = 2 * 2 * nbt16 * ((H + kc - 1) // kc) * 256 * 4
            pers = 4 * 2 * nbt16 * ((H + kc - 1) // kc) * 1024 + 64
            if bf16 == 2:
                pers = max(pers, 8 * 2 * nbt16 * ((H + 31) // 32) * 1024 + 64)
            got = lib.ds2_rnn_bwd_workspace_bytes(1, B, H, bf16)
            assert got == 4 * B * H * 4 + max(step, pers), (B, bf16, got)
            # the forward recurrence of the tanh cell has the GRU's workspace (it depends on H only through the h exchange)
            assert lib.ds2_rnn_fwd_workspace_bytes(B, H, bf16) > 0
            assert got <= lib.ds2_rnn_bwd_workspace_bytes(3, B, H, bf16)


def test_library_sizes_match_the_recorded_table(golden_dir):
    """ds2_rnn_fwd_workspace_bytes, ds2_rnn_bwd_workspace_bytes and ds2_rnn_packed_bytes over gates x mode x H x B against
    tests/golden/rnn_sizes.json, recorded from the library before the sizes moved into csrc/rnn_sizes.h: callers size their buffers with
    these, and the launchers fill what the same functions state."""
    import json
    lib = _lib()
    with open(os.path.join(golden_dir, "rnn_sizes.json")) as f:
        tab = json.load(f)
    G, M, Hs, Bs = tab["gates"], tab["modes"], tab["H"], tab["B"]
    assert (G, M) == ([1, 3, 4], [0, 1, 2]) and len(Hs) == 11 and len(Bs) == 6
    for mi, m in enumerate(M):
        for hi, H in enumerate(Hs):
            for bi, B in enumerate(Bs):
                assert lib.ds2_rnn_fwd_workspace_bytes(B, H, m) == tab["fwd_workspace_bytes"][mi][hi][bi], (m, H, B)
                for gi, g in enumerate(G):
                    assert lib.ds2_rnn_bwd_workspace_bytes(g, B, H, m) == tab["bwd_workspace_bytes"][gi][mi][hi][bi], (g, m, H, B)
            for gi, g in enumerate(G):
                for which in (0, 1):
                    assert lib.ds2_rnn_packed_bytes(g, H, which, m) == tab["packed_bytes"][gi][mi][hi][which], (g, m, H, which)


@pytest.mark.parametrize("H", [256, 512, 1024, 1280])
def test_ksplit_footprint_reports_not_available_for_one_gate(H):
    """No K-split backward for the tanh cell: the footprint query answers 0 ("no such kernel") without an error, and the co-residence
    decision of the host layer follows."""
    from asr_amd import ops
    out = (C.c_int * 3)(7, 7, 7)
    assert _lib().ds2_rnn_bwd_ksplit_footprint(1, H, out) == 0
    assert list(out) == [0, 0, 0]
    assert ops.wgrad_fits_beside_bwd_recurrence(1, H) is False


def test_gates_other_than_1_3_4_are_still_refused():
    lib = _lib()
    out = (C.c_int * 3)()
    assert lib.ds2_rnn_bwd_ksplit_footprint(2, 256, out) < 0
    assert "ds2_rnn_bwd_ksplit_footprint" in lib.ds2_last_error().decode()
