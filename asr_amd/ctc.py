"""`CTCLoss` — call-compatible with `torch.nn.CTCLoss` as the reference wires it
(trainers/__main__.py:53, called at trainers/deepspeech_trainer.py:111) and backed by the fused
log-softmax + CTC HIP kernels (asr_amd/csrc/ctc.hip).

Input may be log-probabilities (T,B,C) *or* raw logits: the kernel re-normalises each row (for
log-softmaxed input the row log-sum-exp is 0, so results are identical to torch's).  The gradient
returned w.r.t. the input is `softmax - occupancy`, exactly what aten's `_ctc_loss_backward`
produces for log-softmaxed input.

Imperfect transcripts (`CTCLoss(star=..., star_penalty=..., free_start=..., free_end=...)`): the wildcard loss of
ds2_ctc_star_loss_f32 (contract in include/ds2hip.h), the vocabulary of `CTCAligner.align`'s options over log-sum-exp.
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops


def _prep_targets_host(targets, target_lengths):
    """CPU int32 tensors (flat targets, per-utterance offsets, target lengths) and the longest target."""
    tl = torch.as_tensor(target_lengths).to(torch.int32).cpu()
    t = torch.as_tensor(targets).to(torch.int32).cpu()
    if t.dim() == 2:  # padded (B, S) form of torch.nn.CTCLoss
        t = torch.cat([t[i, : int(tl[i])] for i in range(t.size(0))]) if t.numel() else t.reshape(-1)
    off = torch.zeros(tl.numel(), dtype=torch.int32)
    if tl.numel() > 1:
        off[1:] = torch.cumsum(tl, 0)[:-1].to(torch.int32)
    max_u = int(tl.max()) if tl.numel() else 0
    if t.numel() == 0:
        t = torch.zeros(1, dtype=torch.int32)
    return t, off, tl, max_u


def _prep_star_targets_host(targets, target_lengths, star_id, free_start=False, free_end=False):
    """_prep_targets_host for the wildcard loss: the targets (flat or padded, the id star_id the wildcard) with runs of adjacent
    wildcards collapsed and, for free_start / free_end, a wildcard put at the front / back of every target unless one is there
    (decoders.wildcard_ends, the rule of CTCAligner.align).  Returns (flat targets, offsets, lengths, longest target, flags), CPU int32."""
    from .decoders import wildcard_ends
    tl = torch.as_tensor(target_lengths).to(torch.int32).cpu().reshape(-1)
    t = torch.as_tensor(targets).to(torch.int32).cpu()
    lens = [int(v) for v in tl.tolist()]
    if t.dim() == 2:
        seqs = [t[i, :n].tolist() for i, n in enumerate(lens)]
    else:
        flat, seqs, o = t.reshape(-1).tolist(), [], 0
        for n in lens:
            seqs.append(flat[o:o + n])
            o += n
    seqs, flags = wildcard_ends(seqs, int(star_id), free_start, free_end, distinct_paths=True)
    t_h, off_h, tl_h, max_u = _prep_targets_host(torch.tensor([i for s in seqs for i in s], dtype=torch.int32),
                                                 torch.tensor([len(s) for s in seqs], dtype=torch.int32))
    return t_h, off_h, tl_h, max_u, torch.tensor(flags, dtype=torch.int32)


def _check_star_penalty(star_penalty):
    sp = float(star_penalty)
    if not (sp <= 0.0 and math.isfinite(sp)):
        raise ValueError(f"star_penalty must be finite and <= 0, got {star_penalty}")
    return sp


def _prep_targets(targets, target_lengths, device):
    tl = torch.as_tensor(target_lengths).to(torch.int32).cpu()
    t = torch.as_tensor(targets).to(torch.int32).cpu()
    if t.dim() == 2:  # padded (B, S) form of torch.nn.CTCLoss
        t = torch.cat([t[i, : int(tl[i])] for i in range(t.size(0))]) if t.numel() else t.reshape(-1)
    off = torch.zeros(tl.numel(), dtype=torch.int32)
    if tl.numel() > 1:
        off[1:] = torch.cumsum(tl, 0)[:-1].to(torch.int32)
    max_u = int(tl.max()) if tl.numel() else 0
    if t.numel() == 0:
        t = torch.zeros(1, dtype=torch.int32)
    return t.to(device), off.to(device), tl.to(device), max_u


class _CTCFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, targets, input_lengths, target_lengths, want_grad):
        T, B, C = acts.shape
        dev = acts.device
        il = torch.as_tensor(input_lengths).to(torch.int32).to(dev)
        tg, off, tl, max_u = _prep_targets(targets, target_lengths, dev)
        x = acts.float()
        if not (x.stride(2) == 1 and x.stride(0) == B * x.stride(1)):
            x = x.contiguous()
        nll, grad = ops.ctc_loss(x, tg, off, il, tl, max_u, 1.0, want_grad=want_grad)
        ctx.grad = grad
        return nll

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        if grad is None:
            raise RuntimeError("CTC gradient was not requested in forward")
        return grad * g.view(1, -1, 1), None, None, None, None


class _CTCStarFunction(torch.autograd.Function):
    """_CTCFunction on ops.ctc_star_loss: `prepared` is _prep_star_targets_host's tuple."""

    @staticmethod
    def forward(ctx, acts, prepared, input_lengths, star_penalty, want_grad):
        T, B, C = acts.shape
        dev = acts.device
        il = torch.as_tensor(input_lengths).to(torch.int32).to(dev)
        t_h, off_h, tl_h, max_u, flags_h = prepared
        x = acts.float()
        if not (x.stride(2) == 1 and x.stride(0) == B * x.stride(1)):
            x = x.contiguous()
        nll, grad = ops.ctc_star_loss(x, t_h.to(dev), off_h.to(dev), il, tl_h.to(dev), max_u, 1.0, star_penalty=star_penalty,
                                      flags=flags_h.to(dev), want_grad=want_grad)
        ctx.grad = grad
        return nll

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        if grad is None:
            raise RuntimeError("CTC gradient was not requested in forward")
        return grad * g.view(1, -1, 1), None, None, None, None


class CTCLoss(torch.nn.Module):
    """torch.nn.CTCLoss's call on the HIP kernels.  For transcripts that do not account for all the audio (the options of
    CTCAligner.align, here summed over all alignments; with the four at their defaults nothing below applies and the plain entry is
    called):
      star=True        the target id C = log_probs.shape[2], one past the last class, is a WILDCARD: a token that takes at least one
                       frame and matches anything, each of its frames scoring star_penalty; such frames give no gradient of their own.
                       Runs of adjacent wildcards collapse to one.
      free_start / free_end  put a wildcard at the front / back of every target (unless one is there) and make that token optional.
      star_penalty     <= 0, finite, natural log; a plain attribute read at every call (a kernel argument: it may be annealed between
                       steps).  Which value serves real training is NOT measured: a fresh model gives every class about 1/C, so at
                       log(0.5) most frames prefer the wildcard until the labels sharpen; a schedule is the caller's knob.
    reduction="mean" divides by the caller's target_lengths as given, not by the lengths after the insertion."""

    def __init__(self, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False, star: bool = False,
                 star_penalty: float = math.log(0.5), free_start: bool = False, free_end: bool = False):
        super().__init__()
        if blank != 0:
            raise ValueError("the HIP CTC kernel fixes blank = 0 (the reference's only configuration)")
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(reduction)
        self.blank, self.reduction, self.zero_infinity = blank, reduction, zero_infinity
        self.star, self.free_start, self.free_end = bool(star), bool(free_start), bool(free_end)
        self.star_penalty = _check_star_penalty(star_penalty)

    @property
    def wildcards(self) -> bool:
        """True when any of star / star_penalty / free_start / free_end is set: the call takes ds2_ctc_star_loss_f32."""
        return self.star or self.free_start or self.free_end or self.star_penalty != math.log(0.5)

    def prepare_targets(self, targets, target_lengths, star_id):
        """The host half of a wildcard call (also DeepSpeechTrainer.step's): _prep_star_targets_host under this object's options."""
        return _prep_star_targets_host(targets, target_lengths, star_id, self.free_start, self.free_end)

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        if not log_probs.is_cuda:
            raise _lib.DS2LibraryError("asr_amd.CTCLoss needs GPU input (no CPU fallback; the CPU oracle is test-only)")
        want_grad = torch.is_grad_enabled() and log_probs.requires_grad
        if self.wildcards:
            prepared = self.prepare_targets(targets, target_lengths, int(log_probs.shape[2]))
            nll = _CTCStarFunction.apply(log_probs, prepared, input_lengths, _check_star_penalty(self.star_penalty), want_grad)
        else:
            nll = _CTCFunction.apply(log_probs, targets, input_lengths, target_lengths, want_grad)
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        tl = torch.as_tensor(target_lengths).to(nll.device).clamp_min(1).to(nll.dtype)
        return (nll / tl).mean()
