"""-m gpu: the one-launch weight-operand preparation of the bf16 training step (ds2_weight_prep_bf16) against the per-layer entry points
it replaces there (ds2_rnn_pack_whh with bf16 = 1, ds2_cast_transpose_bf16, ds2_cast_bf16_both): every output buffer byte for byte; and
the operands a training step uses always come from the weights as they are at that step."""
import os
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import model_inputs

pytestmark = pytest.mark.gpu


def _bytes_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# name -> (gates, H, [(W_ih columns, row-major pitch or None)] per layer)
STACKS = {
    "gru1024x5": (3, 1024, [(1312, 1344), (1024, None), (1024, None), (1024, 1024), (1024, None)]),    # first layer 1312 -> 1344
    "gru768": (3, 768, [(1312, 1344), (768, None), (768, 768)]),
    "lstm1280": (4, 1280, [(1312, 1344), (1280, None)]),
    "tanh1024": (1, 1024, [(1312, 1344), (1024, None)]),
    "gru100_any_h": (3, 100, [(1312, 1312), (100, 104), (100, None)]),                                   # H % 16 != 0: the per-fragment path
    "first_layer_only": (3, 256, [(1312, 1344)]),
}


@pytest.mark.parametrize("name", list(STACKS))
def test_batched_prep_matches_per_layer_entry_points(name):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import ops
    dev = torch.device("cuda:0")
    G, H, layers = STACKS[name]
    gen = torch.Generator(device="cpu").manual_seed(len(name) + H)
    whh = [(torch.randn(2, G * H, H, generator=gen) * 0.05).to(dev) for _ in layers]
    wih = [(torch.randn(2 * G * H, c, generator=gen) * 0.05).to(dev) for c, _ in layers]
    got = ops.weight_prep_bf16([(G, whh[i], wih[i], layers[i][1]) for i in range(len(layers))])
    assert len(got) == len(layers)
    for i, (c, ld_r) in enumerate(layers):
        wpf, wpb = ops.rnn_pack(G, whh[i], bf16=True)
        assert _bytes_equal(got[i][0], wpf), (name, i, "wp_fwd")
        assert _bytes_equal(got[i][1], wpb), (name, i, "wp_bwd")
        if ld_r is None:
            assert got[i][3] is None
            assert _bytes_equal(got[i][2], ops.cast_transpose_bf16(wih[i])), (name, i, "wihT")
        else:
            wr, wt = ops.cast_bf16_both(wih[i], ld_r=ld_r)
            assert _bytes_equal(got[i][2], wt), (name, i, "wihT")
            assert _bytes_equal(got[i][3], wr), (name, i, "wih row-major")
    # a layer may ask for one half only
    half = ops.weight_prep_bf16([(G, whh[0], None, None), (G, None, wih[0], None)])
    assert half[0][2] is None and half[1][0] is None
    assert _bytes_equal(half[0][0], got[0][0]) and _bytes_equal(half[0][1], got[0][1]) and _bytes_equal(half[1][2], got[0][2])


def _make_model(cfg, sd):
    import pandas as pd
    from asr_amd import DeepSpeech
    audio = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                            spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + ["|"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": chars[: cfg["classes"]]}).to_csv(path, index=False)
        model = DeepSpeech(audio_conf=audio, decoder=None, label_path=path, rnn_type=cfg["rnn"], rnn_hidden_size=cfg["hidden"],
                           rnn_hidden_layers=cfg["layers"], bidirectional=True)
    model.load_state_dict({k: v.cpu() for k, v in sd.items()})
    model.to("cuda:0")
    model.train()
    return model


def test_step_operands_follow_the_current_weights():
    """After load_state_dict, after a step check_loss skipped, and after an applied step, the operands the next step keeps for its backward
    pass (packed W_hh^T fragments, bf16 W_ih^T) are the per-layer kernels' output for the weights as they are THEN."""
    from asr_amd import CTCLoss, FusedAdamW, engine, ops
    from asr_amd.trainers import DeepSpeechTrainer
    from oracle import ds2_oracle as O
    cfg = dict(rnn="gru", hidden=64, layers=3, classes=29, t_ins=[61, 55, 48, 40, 33, 27, 21, 14])
    sd, x, targets, pct, tsz = model_inputs(cfg)
    model = _make_model(cfg, sd)
    model.precision = "bf16"
    B = x.size(0)
    out_lens = model.get_seq_lens(O.lengths_from_percentages(pct, x.size(3)))

    def check(what):
        W = model._flat.tensors(model)
        with torch.no_grad():
            logits, ctx = engine.forward(W, model._cfg, x.cuda(), out_lens.cuda(), training=True, save=True)
        assert len(ctx.layers) == cfg["layers"]
        for l, lc in enumerate(ctx.layers):
            assert _bytes_equal(lc.wpb, ops.rnn_pack(3, W[f"rnns.{l}.whh_cat"], bf16=True)[1]), (what, l, "wp_bwd")
            assert _bytes_equal(lc.wihT, ops.cast_transpose_bf16(W[f"rnns.{l}.wih_cat"])), (what, l, "wihT")
        return logits.clone(), {k: v.clone() for k, v in W.items() if "whh_cat" in k or "wih_cat" in k}

    model._ensure_flat(torch.device("cuda:0"))
    lg0, w0 = check("initial")
    # load_state_dict with other recurrent weights
    sd2 = {k: (v * 1.25 if "rnn" in k and "weight" in k else v) for k, v in model.state_dict().items()}
    model.load_state_dict(sd2)
    lg1, w1 = check("after load_state_dict")
    assert any(not torch.equal(w0[k], w1[k]) for k in w0) and not torch.equal(lg0, lg1)
    # a step that check_loss skips: 40 equal labels need 79 frames
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, FusedAdamW(model, lr=3e-4), None, None, "cuda", "cuda", False, None)
    bad_t, bad_sz = torch.ones(40 * B, dtype=torch.int32), torch.full((B,), 40, dtype=torch.int32)
    valid, lv = tr.step((x, bad_t, pct.clone(), bad_sz))
    assert not valid and lv == float("inf")
    lg2, w2 = check("after a skipped step")
    assert all(torch.equal(w1[k], w2[k]) for k in w1) and torch.equal(lg1, lg2)
    # an applied step
    valid, lv = tr.step((x, targets, pct.clone(), tsz))
    assert valid and np.isfinite(lv)
    lg3, w3 = check("after an applied step")
    assert any(not torch.equal(w2[k], w3[k]) for k in w2) and not torch.equal(lg2, lg3)
