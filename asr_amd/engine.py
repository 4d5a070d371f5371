"""Forward / backward orchestration of the DeepSpeech2 hot path over the libds2hip kernels.

Mirrors, block for block, what autograd replays for the reference's
`DeepSpeech.forward` (modules/deepspeech.py:130-149) — MaskConv conv stack (modules/blocks.py:42-56),
L x BatchRNN (modules/blocks.py:84-93), fc block (modules/deepspeech.py:103-109) — but as an explicit
schedule of HIP kernels with hand-derived backward passes, no torch compute ops on the path.

`W` is a mapping {reference state_dict key -> fp32 GPU tensor} plus the zero-copy concatenated views
`rnns.{l}.wih_cat (2GH, I)`, `rnns.{l}.whh_cat (2, GH, H)`, `rnns.{l}.bih_cat (2GH,)`,
`rnns.{l}.bhh_cat (2, GH)` provided by `asr_amd.params.FlatParams` (forward and reverse direction
weights are stored adjacently, so both directions run as ONE GEMM / ONE recurrence launch series).

`forward` and `backward` are sequences of stage functions (_conv_forward, _rnn_layer_forward, _fc_forward; _fc_backward,
_backward_rnn_deferred or _backward_rnn_layerwise, _conv_backward).  Which path a shape takes is decided in ONE place, `_decide`, which both
evaluate when they start; what a layer's weight-gradient products are is stated in ONE place, `_wgrad_products`.  The schedule experiments
that lost (and their measurements) are in docs/HISTORY.md.
"""
from __future__ import annotations

import os as _os
import threading
from dataclasses import dataclass, field
from functools import partial
from typing import Dict, List, Optional

import torch

from . import _lib, ops

Tensor = torch.Tensor


def _tune(name: str, default: str) -> str:
    """A-B switches of the schedule that tests use as each other's reference: honoured only together with DS2_EXPERIMENTAL=1, so that a stray
    variable cannot change what the product runs.  The precision selectors DS2_F32_GEMM / _RNN / _CONV ("f32" = exact fp32 arithmetic instead of
    split-bf16 products) and the data-parallel schedule DS2_DP_MODE are user choices, not gated."""
    return _os.environ.get(name, default) if _os.environ.get("DS2_EXPERIMENTAL") == "1" else default


# Off-critical-path work of backward.  bf16 training (_backward_rnn_deferred): the operand-preparation passes of the weight-gradient GEMMs
# (transposing casts of dGx / h / d(hn) / Xn, with the bias column sums they carry) run on a side stream: they are HBM-bound and light (17 KB of
# LDS, ~40 registers), so they co-reside with whatever runs on the compute stream — the compute-bound GEMMs, or the latency-bound persistent
# recurrence of the next layer, which leaves most of the memory system idle.  The weight-gradient GEMMs themselves stay on the compute stream,
# one layer late (behind the next layer's recurrence launch), so that nothing heavy ever waits beside a persistent launch that needs every CU.
# c3: 31.7 -> 30.x ms per step.  (The name of this schedule in the measurements: "2"; the two that lost are in docs/HISTORY.md.)
OVERLAP_MODE = "2"
# Weight gradients of the recurrent layers in bf16 mode (DS2_WGRAD_TN, default 1): dW_ih / dW_hh as TN-form GEMMs straight from the row-major
# bf16 buffers the recurrence kernels write (dGx, d(hn), h) and the forward pass kept (Xn), bias gradients from the per-row sums of the
# backward recurrence — no cast / transpose pass at all.  Needs both recurrences of the layer to have run as persistent launches (they are
# the ones that write the bf16 copies); a layer whose recurrences did not keeps the transposing-cast passes below.  0: always those passes.
WGRAD_TN = _tune("DS2_WGRAD_TN", "1") != "0"
# bf16 training, weight gradients of a recurrent layer whose recurrences ran as persistent launches (DS2_WGRAD_SIDE):
#   "sk" (default) ONE launch of the 256 x 256 TN kernel over all products of the layer with a common split-K factor + ONE reduce launch
#                  (ops.gemm_bf16_tn_splitk_group: 192 tiles x 4 K slices = 768 equal work items = three full rounds of the chip), compute stream
#   "0"            round 3's schedule: three TN launches, each with its own split-K factor, slabs and reduce pass, compute stream
#   "1"            ONE launch of the co-resident grouped TN kernel (ops.gemm_bf16_tn_group: 4 waves x 128 registers, one workgroup per CU, no
#                  split-K) on the side stream, released when the compute stream reaches the backward recurrence of the layer BELOW.  The
#                  kernel is sized for exactly the registers / LDS the K-split recurrence leaves on a CU, so the recurrence's residency
#                  holds by construction (csrc/gemm_tn_group.h; 0 starved steps, gradients bit-identical to "main").  Layer 0's products run
#                  beside the conv-stack backward.  MEASURED AND NOT KEPT AS THE DEFAULT (profiles/r04_wgrad_side_ab.txt): the recurrence's
#                  per-step gather queues behind the co-resident kernel's operand DMA in the CU's own memory path and the recurrence loses
#                  1.65-2.0 us per time step (0.83-1.0 ms per layer) — more than the 0.86 ms of work it hides: 27.3 vs 25.9 ms per step.
#   "main"         the same grouped kernel on the compute stream right behind the layer's critical-path work (the one-stream schedule the
#                  side-stream results are compared with bit for bit: tests/test_gpu_round4.py); +0.5 ms per step against "0"
WGRAD_SIDE = _tune("DS2_WGRAD_SIDE", "sk")
# "sk" only: run a layer's grouped launch on the side stream beside the NEXT layer's persistent backward recurrence when that recurrence leaves
# at least WGRAD_IDLE_MIN_CUS compute units without a workgroup (B = 32 shapes: c2, c4); see _backward_rnn_deferred
WGRAD_IDLE = _tune("DS2_WGRAD_IDLE", "1") != "0"
WGRAD_IDLE_MIN_CUS = 64
# fp32 mode, the dense input-to-hidden products (forward projection, dXn, dW_ih, dW_hh) of layers large enough for the 256 x 256 kernels
# (DS2_F32_GEMM): "split" (default) = every fp32 operand split into two bf16 terms (hi = bf16(x), lo = bf16(x - hi)) and the product taken
# as hi.hi + hi.lo + lo.hi on the bf16 matrix cores with fp32 accumulation — ~1e-5 of the fp32 product (the 2^-18 lo.lo term is dropped),
# two orders inside north_star's 1e-3, at 3 bf16 MFMA products instead of one at a sixteenth of the rate (ops.split_bf16);
# "f32" = the fp32-input MFMA kernels (csrc/gemm.hip) for every shape, as rounds 1-3.  Recurrences, BatchNorm, CTC, conv stack: fp32 as before.
F32_GEMM = _os.environ.get("DS2_F32_GEMM", "split")
# fp32 mode, recurrences (DS2_F32_RNN): "split" (default) = the persistent kernels with the moving operand (h_t / dGh_t) and W_hh as two bf16
# planes each (hi + lo) and three bf16 MFMAs per product where the shape fits (forward: GRU up to H = 1024, LSTM up to H = 768; backward:
# GRU / LSTM up to H = 768: csrc/rnn.hip, SP) — fp32-grade results (~1e-6 of the
# fp32 kernels) at a fifth of the fp32-MFMA time; "f32" = the fp32-MFMA kernels.  The library falls back to them by itself where the split
# kernel does not fit, and during a cooldown.
F32_RNN = _os.environ.get("DS2_F32_RNN", "split")
# fp32 mode, conv2's BACKWARD (DS2_F32_CONV): "split" (default) = the bf16 mode's conv2 input-gradient and weight-gradient kernels run three
# times each on split operands — a = hi + lo with hi = bf16(a), lo = bf16(a - hi) (ops.bf16_residual + the bf16 mode's own cast / pack
# kernels), product = hi.hi + lo.hi + hi.lo, the three fp32 results summed by ops.sum3_ (<= 2e-5 of fp64) — instead of the fp32-input MFMA
# kernels (csrc/conv.hip), which run at a sixteenth of the bf16 rate; "f32" = those kernels, as rounds 1-3.  The conv FORWARD stays on the
# fp32 kernels on purpose: measured, a 1e-6 perturbation of y2 flips a ~1e-6 fraction of the Hardtanh(0, 20) branches behind it, and a
# flipped element switches its whole gradient on or off, so the conv-stack gradients move by ~sqrt(1e-6) = 2e-3 — outside north_star's 1e-3
# (4.bias, which depends on the forward alone, showed exactly that; profiles/r04_f32_conv_ab.txt).  conv1 stays fp32 as well.
F32_CONV = _os.environ.get("DS2_F32_CONV", "split")
# bf16 training, BatchNorm1d of the recurrent layers 1 .. L-1 folded into their input projections (DS2_BN_FOLD): the direction sum + statistics
# pass of the layer in front writes ONLY the centred bf16 operand yc = y - m0 (ops.center_colstats: column means from the per-tile sums of h the
# forward recurrence emits, statistics of the centred values) and the normalisation goes into the weights, gx = yc (W_ih diag(s))^T + (b + W_ih c)
# (ops.wih_fold); backward: dW_ih = (dGx^T yc) diag(s) + db (x) c, BatchNorm backward on (yc, delta, var).  Neither y (fp32) nor BN(y) exists
# any more: 327 MB moved per layer in forward instead of 589, 196 instead of 262 for the backward sums.  0: the separate passes of rounds 1-5.
BN_FOLD = _tune("DS2_BN_FOLD", "1") != "0"


def _f32_split_ok(M: int, N: int, K: int, H: int = 8) -> bool:
    """fp32 mode: do this layer's input-to-hidden products run as three-term split-bf16 GEMMs?  H: the layer's hidden size — backward's dW_hh
    problems have N = H and column offsets d * H, d * G * H, which the grouped TN launch wants 16-byte aligned (H % 8 == 0); hidden sizes
    with H % 8 == 4 (accepted by the recurrence entry points) keep the fp32-MFMA GEMM path."""
    return F32_GEMM == "split" and M >= 512 and N >= 256 and K >= 256 and K % 8 == 0 and N % 8 == 0 and H % 8 == 0


_BWD_PERSISTENT = {}      # (id of the recurrence context in use, gates, H, B) -> did the last backward recurrence of this shape run as a persistent launch?
_SIDE = {}


def _bwd_recurrence_workgroups(B: int, H: int) -> int:
    """a persistent backward recurrence is one workgroup per (direction, 16-row batch tile, 32-unit slice) (csrc/rnn_bwd_ksplit.h,
    rnn_bwd_persistent_kernel)"""
    return 2 * ((B + 15) // 16) * ((H + 31) // 32)


def _idle_cus_beside_bwd_recurrence(device, B: int, H: int) -> int:
    """compute units without a workgroup while a persistent backward recurrence runs"""
    return torch.cuda.get_device_properties(device).multi_processor_count - _bwd_recurrence_workgroups(B, H)


def _side_stream(device):
    key = (device.type, device.index, threading.get_ident())      # one side stream per driving thread: two threads never share one
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


@dataclass
class ModelCfg:
    rnn: str            # "gru" | "lstm" | "rnn" (Elman cell, tanh: nn.RNN)
    hidden: int
    layers: int
    classes: int
    freq: int = 161
    precision: str = "fp32"   # "fp32": everything fp32 (parity path) | "bf16": bf16 MFMA operands, fp32 accumulate/state

    @property
    def gates(self) -> int:
        return {"gru": 3, "rnn": 1}.get(self.rnn, 4)


@dataclass(frozen=True)
class _Plan:
    """Which paths a step of this shape takes under the switches as they are now: every shape-and-switch decision of forward and backward,
    each condition once.  Not in here, because they can change between the forward and the backward of one step: what the library did for the
    last recurrence call (ops.rnn_last_path) and for the last backward recurrence of the shape (_BWD_PERSISTENT); they are read where used."""
    rmode: int          # operand mode of the recurrences (what W_hh is packed for): 1 bf16, 2 split-bf16 planes (fp32 mode), 0 fp32
    pack: bool          # bf16 training, B % 8 == 0 (16-byte aligned time-shifted operand views): the saved gates are packed bf16 records and the
                        # backward recurrence writes dGx in bf16; other batch sizes keep fp32 gates / dGx + a cast pass
    deferred: bool      # backward of the recurrent stack is _backward_rnn_deferred (else: _backward_rnn_layerwise)
    may_fold: bool      # layers 1 .. L-1 fold their BatchNorm into the input projection (BN_FOLD)
    wants_h_bf: bool    # the forward recurrence writes a bf16 copy of h: the operand of the TN-form dW_hh
    group_ok: bool      # a layer's TN-form products go out as one grouped launch
    side_ok: bool       # ... the co-resident one, on the side stream beside the backward recurrence of the layer below (WGRAD_SIDE = "1")
    idle: bool          # ... the split-K one, on the side stream on the CUs the backward recurrence of the layer below leaves idle
    idle_f32: bool      # fp32 mode: a layer's off-critical-path block runs on the side stream beside the next layer's backward recurrence


def _decide(cfg: ModelCfg, B: int, T: int, cus: int, in0: int, training: bool = True, save: bool = True) -> _Plan:
    """cus: compute units of the device; in0: input width of recurrent layer 0; backward runs on what a training=True, save=True forward left."""
    G, H = cfg.gates, cfg.hidden
    bf = cfg.precision == "bf16"
    pack = bf and save and B % 8 == 0
    deferred = pack and T > 1
    group_ok = WGRAD_SIDE != "0" and in0 % 8 == 0
    # The idle-CU schedules.  At B = 32 a persistent backward recurrence holds 96 (H = 768) or 160 (H = 1280) of the 256 CUs.  bf16: the grouped
    # split-K launch of the layer above runs on the side stream BEHIND the recurrence launch: its 256 x 256 workgroups (2 x 256 registers per SIMD
    # lane) cannot share a CU with a recurrence workgroup, so they take exactly the CUs the recurrence leaves idle — no CU's memory path is
    # shared (what sank the co-resident kernel, WGRAD_SIDE = "1").  Measured (profiles/r04_wgrad_idle_ab.txt): c4 (LSTM 1280, 160 of 256 CUs in
    # the recurrence) 55.6 -> 51.7 ms — the recurrence pays 3.93 -> 4.52 us per time step for 1.07 ms of hidden GEMM per layer; c2 (GRU 768, 96
    # CUs in the recurrence) 15.08 -> 15.07: with 160 CUs the GEMM is over in 0.4 ms and doubles the step time meanwhile; at an even 128 / 128
    # split (GRU 1024 at B = 32: what a 32-row backward kernel would create at c3's B = 64) the recurrence pays MORE than is hidden — 5.61 ->
    # 7.63 ms of recurrences for 4 x 0.45 ms of GEMM, the step 18.2 -> 19.2 ms (profiles/r05_idle_split_proxy.txt) — so only where the
    # recurrence is the clear majority tenant (idle < half the chip).  fp32 mode: the split-bf16 weight-gradient launch of a layer beside the
    # next layer's recurrence, c2 f32 33.9 -> 32.6 ms (the recurrence pays 3.40 -> 3.75 us per time step, same profile).
    n_idle = cus - _bwd_recurrence_workgroups(B, H)
    idle_room = WGRAD_IDLE and n_idle >= WGRAD_IDLE_MIN_CUS
    return _Plan(rmode=1 if bf else (2 if (F32_RNN == "split" and H % 32 == 0) else 0),
                 pack=pack, deferred=deferred,
                 may_fold=deferred and BN_FOLD and training and H % 8 == 0,
                 wants_h_bf=deferred and WGRAD_TN,
                 group_ok=group_ok,
                 side_ok=deferred and group_ok and WGRAD_SIDE == "1" and ops.wgrad_fits_beside_bwd_recurrence(G, H),
                 idle=deferred and group_ok and WGRAD_SIDE == "sk" and idle_room and n_idle < cus // 2,
                 idle_f32=idle_room and not bf)


def _plan_for(W, cfg: ModelCfg, B: int, T: int, device, training: bool = True, save: bool = True) -> _Plan:
    return _decide(cfg, B, T, torch.cuda.get_device_properties(device).multi_processor_count, W["rnns.0.wih_cat"].shape[1], training, save)


def _hh_gate_rows(G: int, H: int) -> int:
    """rows of dW_hh (per direction) that come from dGx; a GRU's n-gate rows come from d(hn) instead"""
    return 2 * H if G == 3 else G * H


def _wgrad_products(G: int, H: int, B: int, M: int, dgx, dhn, h, xn, dwih, dwhh, transposed: bool = False):
    """The weight-gradient products of one recurrent layer, as (A, B, out) with out = A^T B over the reduction index t * B + b:
        ih:  (dGx, Xn, dW_ih)
        hh:  per term (the dGx rows; for a GRU also the n-gate rows from d(hn)) one entry (direction 0, direction 1, out of both), where
             direction 0 pairs dGh[t] with h[t-1] and direction 1 dGh[t] with h[t+1]: a shift of B along the reduction index.
    Operands are row-major (reduction index on the rows: the shift is a row offset) or, transposed=True, their transposes (a column offset).
    h = None (T = 1): no hh term at all.  dhn is only looked at for a GRU."""
    rows = _hh_gate_rows(G, H)
    cut = (lambda t, time, c0, c1: t[c0:c1, time]) if transposed else (lambda t, time, c0, c1: t[time, c0:c1])
    shift = ((slice(B, M), slice(0, M - B)), (slice(0, M - B), slice(B, M)))          # (rows of dGh, rows of h) per direction
    hh = []
    if h is not None:
        for src, width, r0, r1 in ((dgx, G * H, 0, rows),) + (((dhn, H, 2 * H, 3 * H),) if G == 3 else ()):
            hh.append(tuple((cut(src, shift[d][0], d * width, d * width + r1 - r0), cut(h, shift[d][1], d * H, (d + 1) * H), dwhh[d, r0:r1])
                            for d in (0, 1)) + (dwhh[:, r0:r1],))
    return (dgx, xn, dwih), hh


@dataclass
class BnGrad:
    """Gradient wrt a BatchNorm1d OUTPUT together with what its elementwise backward needs: consumed by ops.rnn_bwd_bn of the layer below."""
    dyn: Tensor          # (M, H) gradient wrt the BatchNorm output
    x: Tensor            # (M, H) the BatchNorm input (= the layer below's y)
    mean: Tensor
    var: Tensor
    gamma: Tensor
    sums: tuple          # two (H,) vectors: column sums of dyn and of dyn * xhat


def _bn_backward(dxn: Tensor, x: Tensor, mean, var, gamma, dgamma, dbeta, fuse: bool, private_sums: bool):
    """BatchNorm1d backward in front of a recurrent layer's backward: the materialised gradient, or (fuse: bf16 training, the elementwise half
    is applied inside the K-split backward recurrence of the layer below, ops.rnn_bwd_bn — one more 4-byte load per pair and step instead of a
    pass over (T*B, H)) the column sums only + a BnGrad.
    private_sums: the gradient buffers may be all-reduced (asynchronously, in place) before the recurrence below has read the sums."""
    xbf = x.dtype == torch.bfloat16                      # BN_FOLD: x = the centred bf16 operand, mean = its delta
    if not fuse:
        return (ops.bn1d_bwd_xbf if xbf else ops.bn1d_bwd)(dxn, x, mean, var, gamma, dgamma, dbeta)
    sums_fn = ops.bn1d_bwd_sums_xbf if xbf else ops.bn1d_bwd_sums
    if private_sums:
        sums = sums_fn(dxn, x, mean, var, gamma)
        dbeta.copy_(sums[0])
        dgamma.copy_(sums[1])
    else:
        sums = sums_fn(dxn, x, mean, var, gamma, out=(dbeta, dgamma))
    return BnGrad(dxn, x, mean, var, gamma, sums)


@dataclass
class LayerCtx:
    xin: Optional[Tensor] = None     # (M, I) raw layer input (previous y) — BN backward needs it
    xn: Optional[Tensor] = None      # (M, I) GEMM A operand (BN output, or the raw input for layer 0)
    gx: Optional[Tensor] = None      # (M, 2GH) gates -> overwritten by dGx in backward (tanh cell: the x-projections, not written by the forward)
    hbuf: Optional[Tensor] = None    # (M, 2H)
    aux: Optional[Tensor] = None     # (M, 2H) (None for the tanh cell: h is its whole saved state)
    mean: Optional[Tensor] = None    # BN batch stats of this layer's INPUT (layers >= 1)
    var: Optional[Tensor] = None
    wpb: Optional[Tensor] = None     # W_hh^T in fragment order for the backward recurrence
    rec: Optional[Tensor] = None     # bf16 training: packed saved-gate records (M, 2H, 4) instead of gates in gx
    h_bf: Optional[Tensor] = None    # bf16 training, persistent forward recurrence: (M, 2H) bf16 copy of hbuf (operand of the TN-form dW_hh)
    wihT: Optional[Tensor] = None    # bf16 training: bf16 W_ih^T (I, pad8(2GH)), the B operand of dX (cast with the forward projection's operand)
    xs: Optional[Tensor] = None      # fp32 mode, split-bf16 GEMMs: (M, 3 I) [hi | hi | lo] split copy of xn (xn itself is then not kept)
    gshape: tuple = ()               # (M, 2GH) when gx itself was released
    fold: tuple = ()                 # BN_FOLD: (colscale s, colshift c) of this layer's folded BatchNorm; xin / xn are then the centred bf16 operand


@dataclass
class Ctx:
    B: int = 0
    T: int = 0
    D1: int = 0
    D2: int = 0
    x: Optional[Tensor] = None
    lens_dev: Optional[Tensor] = None
    y1: Optional[Tensor] = None
    a1: Optional[Tensor] = None      # fp32 Hardtanh(BN(conv1)) (fp32 mode; bf16 mode keeps only a1p)
    a1p: Optional[Tensor] = None     # bf16 mode: the bf16 operand of conv2's weight gradient (the channels-last copy conv2's forward took)
    y2: Optional[Tensor] = None
    st1: tuple = ()
    st2: tuple = ()
    packs: tuple = ()
    x16t: Optional[Tensor] = None      # bf16 mode: conv1's time-contiguous operand image (kept for its weight gradient)
    layers: List[LayerCtx] = field(default_factory=list)
    y_last: Optional[Tensor] = None
    fc_xn: Optional[Tensor] = None
    fc_stats: tuple = ()
    side_used: bool = False          # backward put weight-gradient work on the side stream: the compute stream joins it at the end


# ================================================================ forward ================================================================

def _running(W, name: str, training: bool):
    return (W[name + ".running_mean"], W[name + ".running_var"]) if training else (None, None)


def _bn2d_statistics(W, name: str, y: Tensor, partials, count: int, training: bool):
    """BatchNorm2d statistics of a conv output: the running ones (eval), from the per-block channel sums of the conv epilogue (bf16 training),
    or from a pass over y"""
    if not training:
        return W[name + ".running_mean"], W[name + ".running_var"]
    if partials is not None:
        return ops.chanstats_from_partials(partials, count, *_running(W, name, True))
    return ops.bn2d_stats(y, *_running(W, name, True))


def _conv_forward(W, cfg: ModelCfg, ctx: Ctx, training: bool, save: bool, debug_acts: bool):
    """MaskConv stack on ctx.x.  Returns (xin, xn0): the (T*B, 32*D2) input of recurrent layer 0 in fp32 (bf16 mode: only with debug_acts) and
    its zero-padded bf16 GEMM operand (bf16 mode).  save: what backward needs goes into ctx."""
    x, lens_dev, B, T, D1, D2 = ctx.x, ctx.lens_dev, ctx.B, ctx.T, ctx.D1, ctx.D2
    Tin = x.shape[3]
    bf = cfg.precision == "bf16"
    cp = "conv.seq_module."
    st_part1 = st_part2 = None
    if bf:
        # conv1 on the bf16 matrix cores: operand images gathered once from the spectrogram (the time-contiguous one is kept
        # for the weight gradient)
        X16, ctx.x16t = ops.conv1_gather_bf16(x, want_fwd=True, want_wgrad=save)
        # training: the BatchNorm2d statistics come out of the conv epilogues (per-block channel sums), not from another pass over y
        y1 = ops.conv1_fwd_bf16(X16, ops.conv1_pack_bf16(W[cp + "0.weight"]), W[cp + "0.bias"], lens_dev, Tin, stats=training)
        if training:
            y1, st_part1 = y1
        del X16
    else:                                                        # (the bf16 mode has its own operand packs: conv1_pack_bf16 / conv2_pack_bf16)
        wpk1, wpk2, wpk2d = ops.conv_pack(W[cp + "0.weight"], W[cp + "3.weight"])
        ctx.packs = (wpk2d,)
        y1 = ops.conv1_fwd(x, wpk1, W[cp + "0.bias"], lens_dev)
    m1, v1 = _bn2d_statistics(W, cp + "1", y1, st_part1, B * D1 * T, training)
    if bf:
        # one pass over y1 emits conv2's channels-last operand, which is also the operand of conv2's weight gradient (kept when backward
        # follows); the fp32 activation itself has no consumer in this mode (debug_acts keeps it for the tests that inspect it)
        a1, _, a1n = ops.bn2d_act_fwd_fused(y1, lens_dev, m1, v1, W[cp + "1.weight"], W[cp + "1.bias"], want_f32=debug_acts, want_pad=False,
                                            want_nhwc=True)
        cwf, cwd0, cwd1 = ops.conv2_pack_bf16(W[cp + "3.weight"])
        ctx.packs = (None, cwd0, cwd1)
        y2 = ops.conv2_fwd_bf16(a1n, cwf, W[cp + "3.bias"], lens_dev, stats=training)
        if training:
            y2, st_part2 = y2
        a1p = a1n if save else None
        del a1n
    else:
        a1, a1p = ops.bn2d_act_fwd(y1, lens_dev, m1, v1, W[cp + "1.weight"], W[cp + "1.bias"]), None
        y2 = ops.conv2_fwd(a1, wpk2, W[cp + "3.bias"], lens_dev)
    m2, v2 = _bn2d_statistics(W, cp + "4", y2, st_part2, B * D2 * T, training)
    xn0 = None
    if bf:
        # BN + Hardtanh + mask + collapse + cast in one pass: layer 0 takes the bf16 operand; nobody needs the fp32 form
        # (row pitch rounded up to the GEMMs' 64-deep k-tile: 1312 -> 1344 zero-padded features put layer 0's projection on the four-wave kernel)
        xin, xn0 = ops.bn2d_act_collapse(y2, lens_dev, m2, v2, W[cp + "4.weight"], W[cp + "4.bias"], want_f32=debug_acts, pad_to=64)
    else:
        a2 = ops.bn2d_act_fwd(y2, lens_dev, m2, v2, W[cp + "4.weight"], W[cp + "4.bias"])
        xin = ops.transpose_bft(a2, B, 32 * D2, T, to_tbf=True).view(T * B, 32 * D2)   # (T*B, 1312), feature = c*D2 + d
        del a2
    if save:
        ctx.y1, ctx.a1, ctx.a1p, ctx.y2, ctx.st1, ctx.st2 = y1, a1, a1p, y2, (m1, v1), (m2, v2)
    return xin, xn0


def _rnn_layer_forward(W, cfg: ModelCfg, plan: _Plan, l: int, xin, xn0, stats, prep, lens_dev, B: int, T: int, training: bool, save: bool):
    """BatchRNN block l on xin (layer 0: xn0 is its bf16 operand).  stats: (mean, var, delta) of xin as the layer in front computed them
    (delta: only with the centred bf16 xin of a folded BatchNorm); prep: the weight operands of ops.weight_prep_bf16 (bf16 training) or None.
    Returns (y, the statistics of y, the layer's saved context)."""
    G, H, L = cfg.gates, cfg.hidden, cfg.layers
    M, dev = T * B, lens_dev.device
    bf = cfg.precision == "bf16"
    mean, var, delta = stats
    wih, bih = W[f"rnns.{l}.wih_cat"], W[f"rnns.{l}.bih_cat"]
    bp = f"rnns.{l}.batch_norm.module."
    lc = LayerCtx()
    # the workspace of a recurrence call (exchange buffers of a persistent launch: every byte 0xff) is armed AHEAD of the GEMM in front of the
    # recurrence instead of by a fill launched between that GEMM and the recurrence
    ws_f = ops.rnn_ws("fwd", G, B, H, plan.rmode, dev)
    # ---- the input projection gx = BN(xin) W_ih^T + b_ih
    if l > 0 and xin.dtype == torch.bfloat16:                    # BN_FOLD: the layer in front left the centred bf16 operand (+ mean, var, delta)
        xn = xin
        w_bf, bias_eff, colscale, colshift = ops.wih_fold(wih, bih, var, W[bp + "weight"], W[bp + "bias"], delta, ld=xn.shape[1])
        lc.wihT = prep[l][2]                                     # (un-scaled: dX is the gradient wrt BN's OUTPUT, as before)
        lc.mean, lc.var, lc.fold = delta, var, (colscale, colshift)        # (the mean OF xin)
        gx = ops.gemm_bf16_nt(xn, w_bf, bias=bias_eff)
    else:
        if l > 0:
            if not training:
                mean, var = W[bp + "running_mean"], W[bp + "running_var"]
            # bf16 mode: the normalised input exists only as the bf16 GEMM operand (kept for dW_ih in backward)
            xn = (ops.bn1d_apply_bf16 if bf else ops.bn1d_apply)(xin, mean, var, W[bp + "weight"], W[bp + "bias"])
            lc.mean, lc.var = mean, var
        else:
            xn = xn0 if bf else xin
        if bf:
            if not save:
                w_bf = ops.cast_bf16(wih, ld=xn.shape[1])
            elif prep[l][3] is not None and prep[l][3].shape[1] == xn.shape[1]:
                lc.wihT, w_bf = prep[l][2], prep[l][3]
            else:
                # ONE read of W_ih gives the row-major bf16 operand of this projection and the transposed one of dX (kept for backward)
                w_bf, lc.wihT = ops.cast_bf16_both(wih, ld_r=xn.shape[1])
            gx = ops.gemm_bf16_nt(xn, w_bf, bias=bih)
        elif _f32_split_ok(M, 2 * G * H, xn.shape[1], H):
            # three-term split-bf16 product as ONE NT GEMM over a reduction index 3 I long: [hi | hi | lo] x [hi | lo | hi]^T
            # (rows padded with zeros to a multiple of the TN kernels' 64-deep k-tile: as the K-row-major operand of dW_ih in backward the split
            #  copy then has a reduction length the four-wave kernel takes — T * B = 16032 at c2, 24032 at c4)
            lc.xs = ops.split_bf16(xn, 0, pad_rows=64 if save else 0)
            gx = ops.gemm_bf16_nt(lc.xs[:M], ops.split_bf16(wih, 1), bias=bih)
            if save:
                xn = None                                        # backward takes dW_ih from the split copy (6 bytes per element instead of 4 + 6)
        else:
            gx = ops.gemm(xn, wih, transB=True, bias=bih)        # (M, 2GH)
    # ---- the recurrence
    wpf, wpb = prep[l][:2] if prep is not None else ops.rnn_pack(G, W[f"rnns.{l}.whh_cat"], bf16=plan.rmode)
    if prep is not None:
        prep[l] = None                                           # (the forward operands die with their layer)
    hsum = None
    if plan.pack:
        # the saved gates are ONE packed bf16 record per hidden unit; the fp32 x-projection buffer is then dead after the recurrence
        # (no bf16 h for shapes whose backward recurrence is known to run one launch per step - LSTM H = 1280: nobody would read the copy)
        h_bf = (torch.empty(M, 2 * H, dtype=torch.bfloat16, device=dev)
                if (plan.wants_h_bf and _BWD_PERSISTENT.get((ops.rnn_ctx_key(dev), G, H, B), True)) else None)
        # BN_FOLD: the layer behind this one folds its BatchNorm — this recurrence emits the per-tile column sums of h it needs
        if plan.may_fold and l + 1 < L:
            hsum = torch.empty(2, (B + 15) // 16, H, dtype=torch.float32, device=dev)
        hbuf, aux, lc.rec = ops.rnn_fwd(G, gx, wpf, W[f"rnns.{l}.bhh_cat"], lens_dev, T, B, H, bf16=True, packed_gates=True, h_bf16=h_bf, ws=ws_f,
                                        hsum=hsum)
        if hsum is not None and not (ops.rnn_last_path(dev) & 1):
            hsum = None                                          # (only a persistent launch writes it)
        gx, lc.gshape = None, (M, 2 * G * H)
        if h_bf is not None and (ops.rnn_last_path(dev) & 1):
            lc.h_bf = h_bf                                       # (only a persistent launch writes it)
    else:
        hbuf, aux = ops.rnn_fwd(G, gx, wpf, W[f"rnns.{l}.bhh_cat"], lens_dev, T, B, H, bf16=plan.rmode, ws=ws_f)
    lc.wpb = wpb
    # ---- direction sum + the statistics of the BatchNorm behind
    run = _running(W, f"rnns.{l + 1}.batch_norm.module" if l + 1 < L else "fc.0.module.0", training)
    if hsum is not None:
        y, mean, var, delta = ops.center_colstats(hbuf[:, :H], hbuf[:, H:], hsum, *run)     # y: the CENTRED bf16 operand
    else:
        (y, mean, var), delta = ops.add_colstats(hbuf[:, :H], hbuf[:, H:], *run), None
    if save:
        lc.xin, lc.xn, lc.gx, lc.hbuf, lc.aux = xin, xn, gx, hbuf, aux
    return y, (mean, var, delta), lc


def _fc_forward(W, xin: Tensor, stats, training: bool):
    """fc block: BatchNorm1d + Linear.  Returns (logits (M, C), the normalised input, the statistics used)."""
    fp = "fc.0.module."
    mean, var = stats[:2] if training else (W[fp + "0.running_mean"], W[fp + "0.running_var"])
    xn = ops.bn1d_apply(xin, mean, var, W[fp + "0.weight"], W[fp + "0.bias"])
    return ops.gemm(xn, W[fp + "1.weight"], transB=True), xn, (mean, var)


def forward(W: Dict[str, Tensor], cfg: ModelCfg, x: Tensor, lens_dev: Tensor, training: bool, save: bool = True, debug_acts: bool = False):
    """x (B,1,F,Tin) fp32 GPU; lens_dev int32 (B,) GPU = output frame counts.  Returns (logits (T,B,C), ctx)."""
    if not x.is_cuda:
        raise _lib.DS2LibraryError("asr_amd.engine.forward needs a GPU tensor: the MI355X kernels are the only implementation "
                                   "(the CPU restatement lives in oracle/ and is test-only)")
    x = x.contiguous().float()
    B, _, F, Tin = x.shape
    D1, D2, T = _lib.conv_dims(F, Tin)
    G, H, L = cfg.gates, cfg.hidden, cfg.layers
    plan = _plan_for(W, cfg, B, T, x.device, training, save)
    ctx = Ctx(B=B, T=T, D1=D1, D2=D2, x=x, lens_dev=lens_dev)
    xin, xn0 = _conv_forward(W, cfg, ctx, training, save, debug_acts)
    prep = None
    if cfg.precision == "bf16" and save:
        # bf16 training: every layer's weight operands (packed W_hh fragments of both recurrences, W_ih^T for dX, and the row-major bf16 W_ih
        # of the layers that do not fold their BatchNorm into it) in ONE launch, from the weights as they are NOW (after the optimizer step,
        # load_state_dict or a skipped step alike: nothing is carried from step to step)
        prep = ops.weight_prep_bf16([(G, W[f"rnns.{l}.whh_cat"], W[f"rnns.{l}.wih_cat"],
                                      xn0.shape[1] if l == 0 else (None if plan.may_fold else ops._pad8(H))) for l in range(L)])
    stats = (None, None, None)
    for l in range(L):
        xin, stats, lc = _rnn_layer_forward(W, cfg, plan, l, xin, xn0, stats, prep, lens_dev, B, T, training, save)
        if save:
            ctx.layers.append(lc)
    logits, fc_xn, fc_stats = _fc_forward(W, xin, stats, training)
    if save:
        ctx.y_last, ctx.fc_xn, ctx.fc_stats = xin, fc_xn, fc_stats
    if training:
        if "_bn_counters" in W:
            ops.add_i64(W["_bn_counters"], 1)          # all num_batches_tracked (views of one buffer: asr_amd/params.py) in one launch
        else:
            for name in (["conv.seq_module.1", "conv.seq_module.4", "fc.0.module.0"] + [f"rnns.{l}.batch_norm.module" for l in range(1, L)]):
                W[name + ".num_batches_tracked"] += 1
    return logits.view(T, B, cfg.classes), ctx


# ================================================================ backward ===============================================================

def _fc_backward(W, Gr, ctx: Ctx, dl: Tensor, fuse: bool, private: bool):
    """dl (M, C).  Linear + BatchNorm1d of the fc block; returns the gradient wrt the top recurrent layer's y (fuse: a BnGrad)."""
    fp = "fc.0.module."
    ops.gemm(dl, ctx.fc_xn, transA=True, out=Gr[fp + "1.weight"])                                 # (C, H)
    dxn = ops.gemm(dl, W[fp + "1.weight"])                                                        # (M, H)
    mean, var = ctx.fc_stats
    return _bn_backward(dxn, ctx.y_last, mean, var, W[fp + "0.weight"], Gr[fp + "0.weight"], Gr[fp + "0.bias"], fuse, private)


def _backward_rnn_deferred(W, Gr, cfg: ModelCfg, ctx: Ctx, plan: _Plan, dy, report, private: bool, serial_buckets: bool):
    """Backward of the recurrent stack in the bf16 training mode (packed gate records, bf16 dGx).  Per layer
        compute stream:  recurrence(l) | weight-gradient GEMMs of layer l+1 | dXn(l) = dGx W_ih | BatchNorm1d backward(l)
        side stream:     [from the start of recurrence(l)] transposing casts of dGx(l+1) (+ db_ih), d(hn)(l+1) (+ db_hn), h(l+1), Xn(l+1)
    Same kernels, same operands, same results as a one-stream schedule: only the streams and the issue order differ.
    Layers whose two recurrences ran as persistent launches (the default for c2 / c3 / c5 shapes) need none of those passes: the kernels
    wrote bf16 h / d(hn) / dGx and the bias partial sums themselves and the weight gradients are TN-form GEMMs on exactly those buffers
    (WGRAD_TN; how they are launched: WGRAD_SIDE, and _Plan.idle).  report(name): the bucket callback.  Returns the gradient wrt layer 0's input."""
    G, H, L = cfg.gates, cfg.hidden, cfg.layers
    B, T = ctx.B, ctx.T
    M = T * B
    lens_dev = ctx.lens_dev
    main = torch.cuda.current_stream()
    dev = ctx.lens_dev.device
    side = _side_stream(dev)

    def done(name):
        """A reducer may release MORE than the named bucket from the calling stream (the "conv" schedule holds fc and every recurrent layer
        until rnns.0 and then records ONE "gradients final" event on the stream it is called from): weight gradients that earlier layers
        left on the side stream must be ordered before that event — the calling stream joins the side stream first."""
        if name == "rnns.0" and ctx.side_used and not serial_buckets:
            torch.cuda.current_stream().wait_stream(side)
        report(name)

    def grads(l):
        return Gr[f"rnns.{l}.wih_cat"], Gr[f"rnns.{l}.whh_cat"]                                   # (2GH, I), (2, GH, H)

    def fold_epilogue(l):
        """BN_FOLD: the projection's operand was the centred yc, not BN(y): dW_ih = (dGx^T yc) diag(s) + db_ih (x) c, applied to the product in
        place on the stream that formed it (db_ih is final before any weight-gradient product of its layer is launched)"""
        f = fold_of.get(l)
        if f:
            ops.scale_rank1_(Gr[f"rnns.{l}.wih_cat"], f[0], Gr[f"rnns.{l}.bih_cat"].view(-1), f[1])

    # the side stream only pays beside a PERSISTENT recurrence (its resident workgroups leave registers and LDS for light kernels); beside
    # one-launch-per-step kernels (shapes whose W_hh^T slice does not fit: LSTM H = 1280) co-running passes delay every launch
    # (c4: 94.6 -> 99.5 ms per step), so there the passes stay on the compute stream.  What the library did for this shape is known from
    # the previous call (ds2_rnn_last_path); the first call of a shape assumes persistent.
    shape_key = (ops.rnn_ctx_key(dev), G, H, B)

    def operand_passes(l, lc_t, dgx_bf, start):
        """side stream, not before `start`: transposing casts of layer l's dGx (+ db_ih), d(hn) (+ db_hn), h and Xn"""
        aux, hbuf, xn = lc_t
        on_side = _BWD_PERSISTENT.get(shape_key, True)
        with torch.cuda.stream(side if on_side else main):
            if on_side:
                side.wait_event(start)
            dgxT, _ = ops.transpose_bf16(dgx_bf, colsum=Gr[f"rnns.{l}.bih_cat"].view(-1))          # + db_ih = column sums of dGx
            dbhh = Gr[f"rnns.{l}.bhh_cat"]                                                        # (2, GH)
            dbhh.copy_(Gr[f"rnns.{l}.bih_cat"].view(2, G * H))
            auxT = None
            if G == 3:
                dbn = torch.empty(2 * H, dtype=torch.float32, device=dev)
                auxT = ops.cast_transpose_bf16(aux, colsum=dbn)                                   # + d(b_hn) = column sums of d(hn)
                dbhh[:, 2 * H:] = dbn.view(2, H)
            hT = ops.cast_transpose_bf16(hbuf)                                                    # (2H, M)
            xnT = ops.transpose_bf16(xn[:, :W[f"rnns.{l}.wih_cat"].shape[1]])                     # xn is bf16 (M, pad8(I)) in this mode
            ready = torch.cuda.Event()
            ready.record(side if on_side else main)
        if on_side:
            for t in (dgx_bf, aux, hbuf, xn):                    # read on the side stream
                if t is not None:                                # (aux: None for the tanh cell)
                    t.record_stream(side)
        return (l, dgxT, hT, auxT, xnT, ready, (dgx_bf,))

    def weight_gradients(p):
        """layer p's dW_hh / dW_ih as NT-form GEMMs on the transposed copies, on the compute stream, behind the event of its operand passes"""
        l, dgxT, hT, auxT, xnT, ready, hold = p
        main.wait_event(ready)
        ih, hh = _wgrad_products(G, H, B, M, dgxT, auxT, hT, xnT, *grads(l), transposed=True)
        for d0, d1, out in hh:                                   # both directions per launch
            ops.gemm_bf16_nt_pair(d0[0], d1[0], d0[1], d1[1], out)
        ops.gemm_bf16_nt(ih[0], ih[1], out=ih[2])
        fold_epilogue(l)
        for t in (dgxT, hT, auxT, xnT) + hold:                   # allocated / last used on the other stream: tell the caching allocator
            if t is not None:
                t.record_stream(main)
        done(f"rnns.{l}")

    def weight_gradients_tn(l, dgx_bf, dhn_bf, h_bf, xn, bias_part):
        """layer l's bias / weight gradients from the row-major bf16 buffers: TN-form GEMMs, one launch per product and direction pair"""
        ops.rnn_bias_grads(G, bias_part, Gr[f"rnns.{l}.bih_cat"], Gr[f"rnns.{l}.bhh_cat"])           # sums over the batch rows
        dwih = Gr[f"rnns.{l}.wih_cat"]
        I = dwih.shape[1]
        _, hh = _wgrad_products(G, H, B, M, dgx_bf, dhn_bf, h_bf, xn, *grads(l))
        for d0, d1, out in hh:
            ops.gemm_bf16_tn_pair(d0[0], d1[0], d0[1], d1[1], out)
        if I % 8 == 0:
            ops.gemm_bf16_tn(dgx_bf, xn[:, :I], out=dwih)
        else:                                                    # xn is zero-padded to a multiple of 8 columns
            dwih.copy_(ops.gemm_bf16_tn(dgx_bf, xn)[:, :I])
        fold_epilogue(l)
        done(f"rnns.{l}")

    def weight_gradients_group(l, dgx_bf, dhn_bf, h_bf, xn, on_side, start):
        """the products of weight_gradients_tn as ONE grouped launch; on_side: on the side stream, not before `start` (an event of the
        compute stream) — the bucket is reported from that stream, behind the launch"""
        ih, hh = _wgrad_products(G, H, B, M, dgx_bf, dhn_bf, h_bf, xn[:, :Gr[f"rnns.{l}.wih_cat"].shape[1]], *grads(l))
        probs = [ih] + [p for d0, d1, _ in hh for p in (d0, d1)]
        f = fold_of.get(l)
        if WGRAD_SIDE == "sk" and f:
            # BN_FOLD: the epilogue of dW_ih (problem 0) rides in the reduce launch of the grouped split-K product
            def launch(pr):
                ops.gemm_bf16_tn_splitk_group(pr, epilogue=(0, f[0], Gr[f"rnns.{l}.bih_cat"].view(-1), f[1]))
        elif WGRAD_SIDE == "sk":
            launch = ops.gemm_bf16_tn_splitk_group
        else:
            def launch(pr):
                ops.gemm_bf16_tn_group(pr)
                fold_epilogue(l)
        if not on_side:
            launch(probs)
            done(f"rnns.{l}")
            return
        with torch.cuda.stream(side):
            side.wait_event(start)
            launch(probs)
            if not serial_buckets:
                done(f"rnns.{l}")                                # (a reducer records its "gradients final" event on the current = side stream)
        if serial_buckets:                                       # the "serial" data-parallel schedule orders every collective INTO the compute stream
            main.wait_stream(side)
            done(f"rnns.{l}")
        for t in (dgx_bf, dhn_bf, h_bf, xn):
            if t is not None:
                t.record_stream(side)
        ctx.side_used = True

    def main_event():
        ev = torch.cuda.Event()
        ev.record(main)
        return ev

    pending = None                                               # operand passes issued, their weight-gradient GEMMs not yet
    queued = None                                                # layer whose operand passes wait for the next recurrence launch
    queued_side = None                                           # layer whose grouped weight-gradient launch waits for the next recurrence
    queued_idle = None                                           # the same for the idle-CU schedule (_Plan.idle)
    fold_of = {l: ctx.layers[l].fold for l in range(L)}          # (kept apart: the layer contexts are cleared as backward moves down)
    ws_b = ops.rnn_ws("bwd", G, B, H, 1, dev)                    # (the top layer's: behind the fc block's backward, which is short)
    for l in range(L - 1, -1, -1):
        lc = ctx.layers[l]
        if queued_side is not None:
            weight_gradients_group(*queued_side, True, main_event())   # everything of the layer above that is on the compute stream is behind this event
            queued_side = None
        if queued is not None:
            # the compute stream is about to start this layer's recurrence: the operand passes of the layer above start WITH it (started
            # earlier they would only take CUs from the GEMMs in between, which fill the register file and leave them no room)
            pending = operand_passes(*queued, main_event())
            queued = None
        start_idle = main_event() if queued_idle is not None else None      # the layer above's operands are final; the recurrence launch follows
        dgx_bf = torch.empty(lc.gx.shape if lc.gx is not None else lc.gshape, dtype=torch.bfloat16, device=dev)
        want_tn = lc.h_bf is not None
        dhn_bf = torch.empty(M, 2 * H, dtype=torch.bfloat16, device=dev) if (want_tn and G == 3) else None
        bias_part = torch.empty(B, 2, 4, H, dtype=torch.float32, device=dev) if want_tn else None
        if isinstance(dy, BnGrad):
            ops.rnn_bwd_bn(G, dy.dyn, dy.x, dy.mean, dy.var, dy.gamma, dy.sums, lc.gx, lc.aux, lc.hbuf, lc.wpb, lens_dev, T, B, H, bf16=True,
                           dgx_bf16=dgx_bf, gates_bf16=lc.rec, dhn_bf16=dhn_bf, bias_part=bias_part, ws=ws_b)
        else:
            ops.rnn_bwd(G, dy, lc.gx, lc.aux, lc.hbuf, lc.wpb, lens_dev, T, B, H, bf16=True, dgx_bf16=dgx_bf, gates_bf16=lc.rec, dhn_bf16=dhn_bf,
                        bias_part=bias_part, ws=ws_b)
        _BWD_PERSISTENT[shape_key] = bool(ops.rnn_last_path(dev) & 2)
        if queued_idle is not None:
            # enqueued BEHIND the recurrence launch: the recurrence's workgroups are dispatched first, the GEMM's fill what is left
            weight_gradients_group(*queued_idle, _BWD_PERSISTENT[shape_key], start_idle)
            queued_idle = None
        tn = want_tn and _BWD_PERSISTENT[shape_key]              # (only a persistent launch writes d(hn) in bf16 and the bias sums)
        lc.rec = None
        if pending is not None:
            weight_gradients(pending)                            # heavy work of the layer above: on the compute stream, behind this launch
            pending = None
        if not tn:
            queued = (l, (lc.aux, lc.hbuf, lc.xn), dgx_bf)
        # ---- critical path: dXn = dGx W_ih -> BatchNorm1d backward -> the next layer's dy
        ws_b = ops.rnn_ws("bwd", G, B, H, 1, dev) if l > 0 else None     # the layer below's recurrence workspace, armed ahead of this GEMM
        dxn = ops.gemm_bf16_nt(dgx_bf, (lc.wihT if lc.wihT is not None else ops.cast_transpose_bf16(W[f"rnns.{l}.wih_cat"])))
        if l > 0:
            bp = f"rnns.{l}.batch_norm.module."
            dy = _bn_backward(dxn, lc.xin, lc.mean, lc.var, W[bp + "weight"], Gr[bp + "weight"], Gr[bp + "bias"], True, private)
        else:
            dy = dxn
        del dxn
        if tn and plan.group_ok:
            ops.rnn_bias_grads(G, bias_part, Gr[f"rnns.{l}.bih_cat"], Gr[f"rnns.{l}.bhh_cat"])
            operands = (l, dgx_bf, dhn_bf, lc.h_bf, lc.xn)
            if plan.side_ok:
                queued_side = operands                           # released with the next layer's recurrence launch (layer 0: below)
            elif plan.idle and l > 0:
                queued_idle = operands                           # launched behind the next layer's recurrence launch, on the CUs it leaves idle
            else:
                weight_gradients_group(*operands, False, None)
        elif tn:
            weight_gradients_tn(l, dgx_bf, dhn_bf, lc.h_bf, lc.xn, bias_part)    # nothing to prepare: straight behind the critical-path work of the layer
        lc.gx = lc.aux = lc.hbuf = lc.xn = lc.wpb = lc.h_bf = lc.wihT = None
    if queued_side is not None:
        weight_gradients_group(*queued_side, True, main_event())       # layer 0: beside the conv-stack backward
    if queued is not None:
        weight_gradients(operand_passes(*queued, main_event()))         # layer 0: nothing latency-bound follows; run its passes now
    return dy


def _layer_weight_gradients(W, Gr, cfg: ModelCfg, B: int, T: int, l: int, lc: LayerCtx, dgx, dgs, dgxT, dbih_sum, main, side, keep, after=None):
    """Layer-wise schedule: the bias and weight gradients of layer l, off the critical path, on `side` (which may be the compute stream) — not
    before the event `after`, or behind everything the compute stream holds now.  dgx: dGx (bf16 from the recurrence, or fp32); dgs: its split
    copy (fp32 mode, split-bf16 products); dgxT, dbih_sum: bf16 mode, the transposed bf16 copy and, for fp32 dGx, its column sums."""
    G, H = cfg.gates, cfg.hidden
    M = T * B
    bf = cfg.precision == "bf16"
    if after is not None:
        side.wait_event(after)
    else:
        side.wait_stream(main)
    keep.append((dgx, lc.aux, lc.hbuf, lc.xn))
    with torch.cuda.stream(side):
        dbih, dbhh = Gr[f"rnns.{l}.bih_cat"], Gr[f"rnns.{l}.bhh_cat"]                             # (2GH,), (2, GH)
        dwih, dwhh = Gr[f"rnns.{l}.wih_cat"], Gr[f"rnns.{l}.whh_cat"]                             # (2GH, I), (2, GH, H)
        Iw = dwih.shape[1]
        if dgx.dtype != torch.bfloat16:                          # (bf16 dGx: its transposing pass has put the column sums into dbih)
            dbih.copy_(dbih_sum if bf else ops.colsum(dgx))
        dbhh.copy_(dbih.view(2, G * H))
        if G == 3:
            dbhh[:, 2 * H:] = ops.colsum(lc.aux).view(2, H)     # d(b_hn) = column sums of d(hn)
        # dW_hh[dir] = sum_t dGh[t]^T h_prev[t]  (h_prev = h[t-1] fwd / h[t+1] reverse), dW_ih (2GH, I) = dGx^T Xn
        if dgs is not None:
            # every product = three terms (hi.hi, hi.lo, lo.hi) on row-pitched views of the split copies; ALL terms of ALL products of the
            # layer (dW_hh of both directions, a GRU's n rows, dW_ih) in ONE grouped split-K launch + one reduce (terms of a product
            # name the same output and are summed: ds2_gemm_bf16_tn_splitk_group)
            C2, Ip = 2 * G * H, lc.xs.shape[1] // 3
            hs = ops.split_bf16(lc.hbuf, 2) if T > 1 else None                                    # (M, 4H) = [hi | lo]
            axs = ops.split_bf16(lc.aux, 2) if (T > 1 and G == 3) else None                       # (M, 4H)
            hi_lo = lambda t, w: (None, None) if t is None else (t[:, :w], t[:, w:])
            (d_hi, d_lo), (h_hi, h_lo), (a_hi, a_lo) = (dgs[:, :C2], dgs[:, 2 * C2:]), hi_lo(hs, 2 * H), hi_lo(axs, 2 * H)
            x_hi, x_lo = lc.xs[:, :Iw], lc.xs[:, 2 * Ip:2 * Ip + Iw]
            terms = [_wgrad_products(G, H, B, M, d, a, h, x, dwih, dwhh)
                     for d, a, h, x in ((d_hi, a_hi, h_hi, x_hi), (d_hi, a_hi, h_lo, x_lo), (d_lo, a_lo, h_hi, x_hi))]
            probs = [hh[j][d] for j in range(len(terms[0][1])) for d in (0, 1) for _, hh in terms] + [ih for ih, _ in terms]
            if T > 1 and len(probs) <= 16 and Iw % 8 == 0:
                ops.gemm_bf16_tn_splitk_group(probs)
            else:                                                # T = 1 (dW_ih alone), or (never at the reference's shapes) term by term
                seen = set()
                for a, b, o in probs:
                    ops.gemm_bf16_tn(a, b, out=o, accumulate=o.data_ptr() in seen)
                    seen.add(o.data_ptr())
            keep.append((hs, axs, dgs, lc.xs))
        elif T > 1:
            # fp32 operands in place (fp32 mode, and bf16 mode with B % 8 != 0): both directions per launch, addressed as a batch of two
            K = (T - 1) * B
            ldg, ldh = 2 * G * H, 2 * H
            a0 = dgx.data_ptr() + 4 * (B * ldg)                 # dir 0: rows t >= 1
            b0 = lc.hbuf.data_ptr()                             #        h[t-1]
            a1 = dgx.data_ptr() + 4 * (G * H)                   # dir 1: rows t <= T-2, column block of dir 1
            b1 = lc.hbuf.data_ptr() + 4 * (H + B * ldh)         #        h[t+1]
            sA, sB = (a1 - a0) // 4, (b1 - b0) // 4
            ops.gemm_raw(True, False, _hh_gate_rows(G, H), H, K, a0, ldg, sA, b0, ldh, sB, dwhh.data_ptr(), H, G * H * H, dgx.device, batch=2)
            if G == 3:  # n-gate rows use d(hn) (aux) instead of dGx_n
                x0 = lc.aux.data_ptr() + 4 * (B * ldh)
                x1 = lc.aux.data_ptr() + 4 * H
                ops.gemm_raw(True, False, H, H, K, x0, ldh, (x1 - x0) // 4, b0, ldh, sB, dwhh.data_ptr() + 4 * (2 * H * H), H,
                             G * H * H, dgx.device, batch=2)
        if T == 1:
            dwhh.zero_()
        if bf:
            xnT = ops.transpose_bf16(lc.xn[:, :Iw])                                               # lc.xn is bf16 (M, pad8(I)) in this mode
            ops.gemm_bf16_nt(dgxT, xnT, out=dwih)
            keep.append((dgxT, xnT))
        elif dgs is None:
            ops.gemm(dgx, lc.xn, transA=True, out=dwih)
    lc.gx = lc.aux = lc.hbuf = lc.xn = lc.wpb = lc.xs = lc.wihT = None


def _backward_rnn_layerwise(W, Gr, cfg: ModelCfg, ctx: Ctx, plan: _Plan, dy, done, f32_key, main, side, keep):
    """Backward of the recurrent stack, layer by layer: the fp32 mode, and the bf16 mode where the deferred schedule does not apply (T = 1,
    B % 8 != 0).  side is main (one stream), or — fp32 mode under _Plan.idle_f32, once the backward recurrences of the shape are known to run as
    persistent launches — the side stream: a layer's weight gradients then run beside the next layer's recurrence."""
    G, H, L = cfg.gates, cfg.hidden, cfg.layers
    B, T, lens_dev = ctx.B, ctx.T, ctx.lens_dev
    M = T * B
    bf = cfg.precision == "bf16"
    defer = side is not main
    pending_off = None
    for l in range(L - 1, -1, -1):
        lc = ctx.layers[l]
        wih = W[f"rnns.{l}.wih_cat"]
        split = (not bf) and lc.xs is not None                   # fp32 mode, three-term split-bf16 products (forward decided: _f32_split_ok)
        # bf16 mode, B % 8 == 0: the recurrence writes dGx in bf16 (row-major) into a side buffer that the GEMMs consume directly
        dgx_bf = torch.empty(lc.gx.shape if lc.gx is not None else lc.gshape, dtype=torch.bfloat16, device=dy.device) if plan.pack else None
        ops.rnn_bwd(G, dy, lc.gx, lc.aux, lc.hbuf, lc.wpb, lens_dev, T, B, H, bf16=plan.rmode, dgx_bf16=dgx_bf, gates_bf16=lc.rec)
        if not bf:
            _BWD_PERSISTENT[f32_key] = bool(ops.rnn_last_path(dy.device) & 2)
        if pending_off is not None:
            fn, ev, pl = pending_off
            pending_off = None
            fn(after=ev)
            with torch.cuda.stream(side):
                done(f"rnns.{pl}")
        lc.rec = None
        dgx = dgx_bf if plan.pack else lc.gx                                                      # dGx (M, 2GH)
        # ---- critical path: dXn = dGx W_ih (feeds the next layer's backward) ---------------------------------------
        dgxT = dgs = dbih_sum = None
        if plan.pack:
            dxn = ops.gemm_bf16_nt(dgx_bf, (lc.wihT if lc.wihT is not None else ops.cast_transpose_bf16(wih)))
            # dW_ih = dGx^T Xn needs the transposed copy; the same read gives db_ih = column sums of dGx
            dgxT, dbih_sum = ops.transpose_bf16(dgx_bf, colsum=Gr[f"rnns.{l}.bih_cat"].view(-1))       # sums land in the gradient buffer
        elif bf:
            dgx_r, dgxT, dbih_sum = ops.cast_bf16_both(dgx, colsum=True)
            dxn = ops.gemm_bf16_nt(dgx_r, (lc.wihT if lc.wihT is not None else ops.cast_transpose_bf16(wih)))
            del dgx_r
        elif split:
            # dXn = dGx W_ih as [hi | hi | lo](dGx) x [hi | lo | hi](W_ih^T)^T; the split copy of dGx also feeds both weight-gradient products
            dgs = ops.split_bf16(dgx, 0, pad_rows=64)                                             # (M rounded up to 64 like lc.xs, 3 * 2GH)
            wT = ops.transpose_batched(wih.unsqueeze(0))[0]                                       # (I, 2GH)
            dxn = ops.gemm_bf16_nt(dgs[:M], ops.split_bf16(wT, 1))
            del wT
        else:
            dxn = ops.gemm(dgx, wih)                                                              # (M, I)
        # ---- off the critical path: bias and weight gradients ------------------------------------------------------
        off_path = partial(_layer_weight_gradients, W, Gr, cfg, B, T, l, lc, dgx, dgs, dgxT, dbih_sum, main, side, keep)
        if not defer:
            off_path()
        if l > 0:
            bp = f"rnns.{l}.batch_norm.module."
            dy = ops.bn1d_bwd(dxn, lc.xin, lc.mean, lc.var, W[bp + "weight"], Gr[bp + "weight"], Gr[bp + "bias"])
        else:
            dy = dxn
        del dxn
        if defer and l > 0:
            # launched behind the NEXT layer's recurrence launch (the loop's top): dispatched first, the GEMM's 256 x 256 workgroups would hold
            # every CU for their first round and the recurrence would wait for them
            ev = torch.cuda.Event()
            ev.record(main)                 # the layer's operands and its BatchNorm gradients are final
            pending_off = (off_path, ev, l)
            continue
        if defer:
            off_path()
            side.wait_stream(main)          # the bucket also holds this layer's BN grads (main stream)
        with torch.cuda.stream(side):
            done(f"rnns.{l}")
    return dy


def _conv1_backward_f32(W, Gr, ctx: Ctx, da1: Tensor):
    """fp32 mode: BatchNorm2d + Hardtanh backward behind conv1, conv1's bias and weight gradients"""
    cp = "conv.seq_module."
    m1, v1 = ctx.st1
    dy1 = ops.bn2d_act_bwd(ctx.y1, da1, ctx.lens_dev, m1, v1, W[cp + "1.weight"], W[cp + "1.bias"], Gr[cp + "1.weight"], Gr[cp + "1.bias"])
    del da1
    Gr[cp + "0.bias"].copy_(ops.chan_sum(dy1))
    ops.conv1_wgrad(ctx.x, dy1, ctx.lens_dev, Gr[cp + "0.weight"])


def _conv_backward(W, Gr, cfg: ModelCfg, ctx: Ctx, dy: Tensor):
    """dy (T*B, 32*D2): the gradient wrt recurrent layer 0's input.  Writes the conv stack's gradients."""
    B, T, D1, D2, lens_dev = ctx.B, ctx.T, ctx.D1, ctx.D2, ctx.lens_dev
    cp = "conv.seq_module."
    da2 = ops.transpose_bft(dy, B, 32 * D2, T, to_tbf=False).view(B, 32, D2, T)
    m2, v2 = ctx.st2
    bn2 = (W[cp + "4.weight"], W[cp + "4.bias"], Gr[cp + "4.weight"], Gr[cp + "4.bias"])
    if cfg.precision == "bf16":
        # dY2 leaves the BatchNorm backward directly as the channels-last bf16 operand conv2's weight gradient / input gradient take, together
        # with conv2's bias gradient (its per-channel sums); conv1's stage keeps fp32 dY1 (cast on the fly by conv1's weight gradient)
        _, _, dy2n = ops.bn2d_act_bwd_fused(ctx.y2, da2, lens_dev, m2, v2, *bn2, Gr[cp + "3.bias"], want_pad=False, want_nhwc=True)
        del da2
        ops.conv2_wgrad_nhwc_bf16(ctx.a1p, dy2n, lens_dev, Gr[cp + "3.weight"])
        da1 = ops.conv2_dgrad_bf16(dy2n, ctx.packs[1], ctx.packs[2], D1)
        del dy2n
        m1, v1 = ctx.st1
        dy1, _, _ = ops.bn2d_act_bwd_fused(ctx.y1, da1, lens_dev, m1, v1, W[cp + "1.weight"], W[cp + "1.bias"], Gr[cp + "1.weight"],
                                           Gr[cp + "1.bias"], Gr[cp + "0.bias"], want_f32=True)
        del da1
        ops.conv1_wgrad_bf16(ctx.x16t, dy1, lens_dev, Gr[cp + "0.weight"], ctx.x.shape[3])
        ctx.x16t = None
    elif F32_CONV == "split":
        dy2, dy2p, dy2n = ops.bn2d_act_bwd_fused(ctx.y2, da2, lens_dev, m2, v2, *bn2, Gr[cp + "3.bias"], want_f32=True, want_pad=True, want_nhwc=True)
        del da2
        r2 = ops.bf16_residual(dy2)
        del dy2
        dy2p_lo, dy2n_lo = ops.padcast_bf16(r2), ops.nhwc_bf16(r2)
        r2 = ops.bf16_residual(ctx.a1)
        a1p = (ops.padcast_bf16(ctx.a1), ops.padcast_bf16(r2))
        del r2
        ph = ops.conv2_pack_bf16(W[cp + "3.weight"])
        pl = ops.conv2_pack_bf16(ops.bf16_residual(W[cp + "3.weight"]))
        # dW2 = a_hi (x) dy_hi + a_lo (x) dy_hi + a_hi (x) dy_lo;  da1 = dy_hi * w_hi + dy_lo * w_hi + dy_hi * w_lo
        g2 = Gr[cp + "3.weight"]
        gb, gc = torch.empty_like(g2), torch.empty_like(g2)
        ops.conv2_wgrad_bf16(a1p[0], dy2p, lens_dev, g2, T)
        ops.conv2_wgrad_bf16(a1p[1], dy2p, lens_dev, gb, T)
        ops.conv2_wgrad_bf16(a1p[0], dy2p_lo, lens_dev, gc, T)
        ops.sum3_(g2, gb, gc)
        del a1p
        wd0, wd1, wl0, wl1 = ph[1], ph[2], pl[1], pl[2]
        da1 = ops.conv2_dgrad_bf16(dy2n, wd0, wd1, D1)
        ops.sum3_(da1, ops.conv2_dgrad_bf16(dy2n_lo, wd0, wd1, D1), ops.conv2_dgrad_bf16(dy2n, wl0, wl1, D1))
        del dy2p, dy2n, dy2p_lo, dy2n_lo
        _conv1_backward_f32(W, Gr, ctx, da1)
    else:
        dy2 = ops.bn2d_act_bwd(ctx.y2, da2, lens_dev, m2, v2, *bn2)
        del da2
        Gr[cp + "3.bias"].copy_(ops.chan_sum(dy2))
        ops.conv2_wgrad(ctx.a1, dy2, lens_dev, Gr[cp + "3.weight"])
        da1 = ops.conv2_dgrad(dy2, ctx.packs[0], D1)
        del dy2
        _conv1_backward_f32(W, Gr, ctx, da1)


def backward(W: Dict[str, Tensor], Gr: Dict[str, Tensor], cfg: ModelCfg, ctx: Ctx, dlogits: Tensor, on_bucket=None, serial_buckets: bool = False):
    """dlogits (T,B,C) contiguous.  Writes every parameter gradient into Gr[name] (same keys as W for
    parameters, plus the *_cat views).  Consumes ctx (gate buffers are overwritten in place).
    `on_bucket(name)` is called as soon as the gradients of 'fc', 'rnns.<l>', 'conv' are final (all
    kernels enqueued) — the data-parallel reducer launches that bucket's RCCL all-reduce there, so
    communication overlaps the rest of the backward pass.  serial_buckets: the reducer orders its collectives into the compute stream
    (its "serial" schedule), so on_bucket must be called from that stream."""
    done = on_bucket if on_bucket is not None else (lambda name: None)
    dev = dlogits.device
    plan = _plan_for(W, cfg, ctx.B, ctx.T, dev)
    main = torch.cuda.current_stream()
    # fp32 mode (_backward_rnn_layerwise): what the library did for the shape is known from the previous step (first step: one stream)
    f32_key = (ops.rnn_ctx_key(dev), cfg.gates, cfg.hidden, ctx.B, "f32")
    side = _side_stream(dev) if (plan.idle_f32 and _BWD_PERSISTENT.get(f32_key, False)) else main
    keep = []      # tensors used on the side stream must outlive it (caching-allocator reuse is per stream)
    dy = _fc_backward(W, Gr, ctx, dlogits.reshape(ctx.T * ctx.B, cfg.classes), plan.deferred, on_bucket is not None)
    done("fc")
    if plan.deferred:
        dy = _backward_rnn_deferred(W, Gr, cfg, ctx, plan, dy, done, on_bucket is not None, serial_buckets)
    else:
        dy = _backward_rnn_layerwise(W, Gr, cfg, ctx, plan, dy, done, f32_key, main, side, keep)
    _conv_backward(W, Gr, cfg, ctx, dy)
    done("conv")
    if side is not main:
        main.wait_stream(side)              # all weight gradients are final for whoever runs next on the main stream
    if ctx.side_used:
        main.wait_stream(_side_stream(dev))
    keep.clear()
