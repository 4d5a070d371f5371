"""fp64 restatement of the bidirectional DeepSpeech model with the Elman (tanh) cell (rnn_type="nn.RNN"), composed from the oracle's
pieces (oracle/ds2_oracle.py knows the GRU / LSTM recurrences only, and stays as it is): conv stack, collapse, BatchNorm1d, fc block and
CTC loss are the oracle's own; the recurrence is `tanh_direction`, written in the style of ds2_oracle.gru_direction."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

import det  # tests/golden/det.py (on sys.path via conftest)
from oracle import ds2_oracle as O


def state_shapes(hidden: int, layers: int, classes: int) -> dict:
    """state_dict shape manifest of the reference model with nn.RNN: the GRU manifest with one gate row block instead of three."""
    sh = det.state_shapes("gru", hidden, layers, classes)
    return {k: ((v[0] // 3,) + tuple(v[1:]) if ".rnn." in k else v) for k, v in sh.items()}


def tanh_direction(gx: Tensor, w_hh: Tensor, b_hh: Tensor, lens: Tensor, reverse: bool) -> Tensor:
    """One direction of a 1-layer tanh RNN in padded+masked form.  gx: (T,B,H) = x W_ih^T + b_ih.  h0 = 0.  Rows t >= len[b] output 0 and
    do not advance the state; the reverse direction therefore starts at each sample's own last frame."""
    T, B, H = gx.shape
    h = gx.new_zeros(B, H)
    outs: List[Optional[Tensor]] = [None] * T
    order = range(T - 1, -1, -1) if reverse else range(T)
    lens_d = lens.to(gx.device)
    for t in order:
        h_new = torch.tanh(gx[t] + h @ w_hh.t() + b_hh)
        m = (t < lens_d).to(gx.dtype).unsqueeze(1)
        h = m * h_new + (1.0 - m) * h
        outs[t] = m * h_new
    return torch.stack(outs, 0)


def bidirectional(x: Tensor, out_lens: Tensor, sd: Dict[str, Tensor], rp: str) -> Tensor:
    """y = h_fwd + h_bwd of one layer without BatchNorm; x (T,B,I), parameters under prefix rp ("rnns.<l>.rnn.")."""
    y = None
    for sfx, rev in (("", False), ("_reverse", True)):
        gx = x @ sd[rp + "weight_ih_l0" + sfx].t() + sd[rp + "bias_ih_l0" + sfx]
        yd = tanh_direction(gx, sd[rp + "weight_hh_l0" + sfx], sd[rp + "bias_hh_l0" + sfx], out_lens, rev)
        y = yd if y is None else y + yd
    return y


def batch_rnn(x: Tensor, out_lens: Tensor, sd: Dict[str, Tensor], prefix: str, batch_norm: bool, training: bool = True,
              stats: Optional[dict] = None) -> Tensor:
    """BatchRNN.forward with the tanh cell: [BatchNorm1d over all T*B rows] -> bi-RNN -> sum of the directions (ds2_oracle.batch_rnn)."""
    T, B, I = x.shape
    if batch_norm:
        bp = prefix + "batch_norm.module."
        flat = x.reshape(T * B, I)
        if training:
            flat, mu, var = O.batch_norm_train(flat, sd[bp + "weight"], sd[bp + "bias"], (0,), (1, -1))
            O._update_running(stats, bp[:-1], mu, var, T * B)
        else:
            flat = O.batch_norm_eval(flat, sd[bp + "weight"], sd[bp + "bias"], sd[bp + "running_mean"], sd[bp + "running_var"], (1, -1))
        x = flat.reshape(T, B, I)
    return bidirectional(x, out_lens, sd, prefix + "rnn.")


def forward(sd: Dict[str, Tensor], x: Tensor, lengths: Tensor, training: bool = True, stats: Optional[dict] = None):
    """DeepSpeech.forward with nn.RNN -> (logits (B,T,C) [softmax in eval], out_lens int32 CPU)."""
    out_lens = O.seq_lens_after_conv(lengths.cpu().int())
    h = O.collapse_to_tbf(O.conv_stack(x, out_lens, sd, training, stats))
    for l in range(O.num_layers(sd)):
        h = batch_rnn(h, out_lens, sd, f"rnns.{l}.", batch_norm=(l > 0), training=training, stats=stats)
    logits = O.fc_block(h, sd, training, stats).transpose(0, 1)
    if not training:
        logits = torch.softmax(logits, dim=-1)
    return logits, out_lens


def fit_and_grads(sd: Dict[str, Tensor], inputs: Tensor, targets: Tensor, input_percentages: Tensor, target_sizes: Tensor, dtype=torch.float64):
    """ds2_oracle.fit_and_grads for the tanh-cell model: {logits, out_lens, loss, grads, stats, input_sizes}."""
    params = {}
    for k, v in sd.items():
        v = v.detach().to(dtype) if v.is_floating_point() else v.detach()
        if v.is_floating_point() and "running_" not in k:
            v = v.clone().requires_grad_(True)
        params[k] = v
    stats: dict = {}
    input_sizes = O.lengths_from_percentages(input_percentages, inputs.size(3))
    out, out_lens = forward(params, inputs.to(dtype), input_sizes, training=True, stats=stats)
    loss = O.ctc_loss_sum(out.transpose(0, 1).log_softmax(2), targets, out_lens, target_sizes) / inputs.size(0)
    keys = [k for k, v in params.items() if v.requires_grad]
    gs = torch.autograd.grad(loss, [params[k] for k in keys], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(params[k])) for k, g in zip(keys, gs)}
    return {"logits": out.detach(), "out_lens": out_lens, "loss": float(loss.detach()), "grads": grads, "stats": stats,
            "input_sizes": input_sizes}


def model_inputs(cfg):
    """(state_dict, inputs, targets, pct, target_sizes) of a fixture cfg, regenerated from det (cfg["seed"] pins the data seed)."""
    w = det.model_state(state_shapes(cfg["hidden"], cfg["layers"], cfg["classes"]), base_seed=0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    x, targets, pct, tsz = det.batch(len(cfg["t_ins"]), cfg["t_ins"], cfg["classes"], seed=int(cfg.get("seed", 1)))
    return sd, torch.from_numpy(x), torch.from_numpy(targets), torch.from_numpy(pct), torch.from_numpy(tsz)
