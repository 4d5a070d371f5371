"""Golden vectors of the bidirectional DeepSpeech model with the Elman (tanh) cell, rnn_type="nn.RNN", from the unmodified reference.

    python tests/golden/make_golden_rnn.py          # writes model_rnn_h32_l2.npz and model_rnn_h48_l3.npz next to this file

Same record layout as make_golden.gen_model (logits, loss, sub-sampled gradients and their norms, BatchNorm running statistics, a 3-step
AdamW loss curve, final weights, the eval-mode softmax and the cfg).  The state_dict shape manifest is taken from the reference model
itself (det.state_shapes knows the GRU / LSTM layouts only); weights and data come from det, as for the other fixtures.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import det  # noqa: E402
from _ref_shim import import_reference  # noqa: E402
from make_golden import audio_conf, label_csv, subsample  # noqa: E402

MODELS = {
    # name: (rnn, hidden, layers, classes, t_ins)
    "rnn_h32_l2": ("rnn", 32, 2, 7, [40, 33, 21]),
    "rnn_h48_l3": ("rnn", 48, 3, 29, [90, 77, 64, 50, 31]),
}


def gen_model_rnn(out, name, DeepSpeech, tmp):
    rnn, hidden, layers, classes, t_ins = MODELS[name]
    model = DeepSpeech(audio_conf=audio_conf(), decoder=None, label_path=label_csv(tmp, classes), rnn_type="nn.RNN",
                       rnn_hidden_size=hidden, rnn_hidden_layers=layers, bidirectional=True)
    assert isinstance(model.rnns[0].rnn, torch.nn.RNN) and model.rnns[0].rnn.nonlinearity == "tanh"
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    weights = det.model_state(shapes, base_seed=0)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    model.train()

    # data seed: the first whose BatchNorm2d outputs keep >= 4e-6 from the Hardtanh kinks (as make_golden.gen_model)
    seed = 1
    while True:
        x, targets, pct, tsz = det.batch(len(t_ins), t_ins, classes, seed=seed)
        inputs = torch.from_numpy(x)
        zs = []
        hk = [model.conv.seq_module[i].register_forward_hook(lambda m, i, o: zs.append(o.detach().clone())) for i in (1, 4)]
        with torch.no_grad():
            sizes = torch.from_numpy(pct.copy()).mul_(int(inputs.size(3))).int()
            ol = model.get_seq_lens(sizes)
            model.conv(inputs, ol)
        for h in hk:
            h.remove()
        margin = 1e30
        for zt in zs:
            msk = (torch.arange(zt.size(3)).view(1, 1, 1, -1) < ol.view(-1, 1, 1, 1)).expand_as(zt)
            v = zt[msk].double()
            margin = min(margin, float(torch.minimum(v.abs(), (v - 20).abs()).min()))
        if margin >= 4e-6 or seed > 400:
            break
        seed += 2
    print(name, "data seed", seed, "kink margin", margin)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})  # undo BN running-stat updates
    targets = torch.from_numpy(targets)
    tsz = torch.from_numpy(tsz)
    criterion = torch.nn.CTCLoss(reduction="sum")
    opt = torch.optim.AdamW(model.parameters(), lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)

    rec = {}
    losses = []
    for step in range(3):
        input_percentages = torch.from_numpy(pct.copy())
        input_sizes = input_percentages.mul_(int(inputs.size(3))).int()
        o, output_sizes = model.forward(inputs, input_sizes)
        o = o.transpose(0, 1)
        loss = criterion(o.float().log_softmax(2), targets, output_sizes, tsz) / inputs.size(0)
        loss_value = loss.item()
        opt.zero_grad()
        loss.backward()
        if step == 0:
            rec["input_sizes"] = input_sizes.numpy()
            rec["output_sizes"] = output_sizes.numpy()
            rec["logits"] = o.detach().transpose(0, 1).contiguous().numpy()   # (B,T,C)
            for k, p in model.named_parameters():
                g = p.grad.detach().numpy()
                rec["grad_" + k] = subsample(g)
                rec["gradnorm_" + k] = np.array(float(np.sqrt((g.astype(np.float64) ** 2).sum())))
                rec["gradsum_" + k] = np.array(float(g.astype(np.float64).sum()))
            for k, v in model.state_dict().items():
                if "running_" in k:
                    rec["buf_" + k] = v.numpy().copy()
        opt.step()
        losses.append(loss_value)
    rec["losses"] = np.array(losses, dtype=np.float64)
    for k, p in model.named_parameters():
        rec["final_" + k] = subsample(p.detach().numpy())
    model.eval()
    with torch.no_grad():
        input_sizes = torch.from_numpy(pct.copy()).mul_(int(inputs.size(3))).int()
        o, _ = model.forward(inputs, input_sizes)
    rec["eval_probs"] = o.numpy()
    rec["cfg"] = np.array(json.dumps(dict(rnn=rnn, hidden=hidden, layers=layers, classes=classes, t_ins=t_ins, seed=seed)))
    np.savez_compressed(os.path.join(out, f"model_{name}.npz"), **rec)
    print(name, "losses", losses)


def main():
    DeepSpeech, _blocks, _functional = import_reference()
    torch.set_num_threads(4)
    with tempfile.TemporaryDirectory() as tmp:
        for name in MODELS:
            gen_model_rnn(HERE, name, DeepSpeech, tmp)


if __name__ == "__main__":
    main()
