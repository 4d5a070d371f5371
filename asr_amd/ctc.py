"""`CTCLoss` — call-compatible with `torch.nn.CTCLoss` as the reference wires it
(trainers/__main__.py:53, called at trainers/deepspeech_trainer.py:111) and backed by the fused
log-softmax + CTC HIP kernels (asr_amd/csrc/ctc.hip).

Input may be log-probabilities (T,B,C) *or* raw logits: the kernel re-normalises each row (for
log-softmaxed input the row log-sum-exp is 0, so results are identical to torch's).  The gradient
returned w.r.t. the input is `softmax - occupancy`, exactly what aten's `_ctc_loss_backward`
produces for log-softmaxed input.

Imperfect transcripts (`CTCLoss(star=..., star_penalty=..., free_start=..., free_end=...)`): the wildcard loss of
ds2_ctc_star_loss_f32 (contract in include/ds2hip.h), the vocabulary of `CTCAligner.align`'s options over log-sum-exp.

`MWERLoss` — minimum-error-rate training on the n-best list of a `BeamCTCDecoder` (ds2_ctc_mwer_f32, contract in include/ds2hip.h).
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


class _MWERFunction(torch.autograd.Function):
    """_CTCFunction on MWERLoss.run: the gradient is stored in forward and scaled per utterance in backward."""

    @staticmethod
    def forward(ctx, acts, crit, targets, input_lengths, target_lengths, want_grad):
        T, B, C = acts.shape
        dev = acts.device
        il = torch.as_tensor(input_lengths).to(torch.int32).to(dev)
        tg, off, tl, max_u = _prep_targets(targets, target_lengths, dev)
        x = acts.float()
        if not (x.stride(2) == 1 and x.stride(0) == B * x.stride(1)):
            x = x.contiguous()
        value, grad = crit.run(x, tg, off, il, tl, max_u, 1.0, want_grad, targets_host=(targets, target_lengths))
        ctx.grad = grad
        return value

    @staticmethod
    def backward(ctx, g):
        grad = ctx.grad
        ctx.grad = None
        if grad is None:
            raise RuntimeError("MWER gradient was not requested in forward")
        return grad * g.view(1, -1, 1), None, None, None, None, None


class MWERLoss(torch.nn.Module):
    """Minimum-error-rate training: the expected risk of the decoder's n-best list under the model, per utterance
        sum_k p_k R_k,   p_k = p_ctc(y_k | x) / sum_j p_ctc(y_j | x)   over the `nbest` best beams of `decoder`,
    plus ctc_weight * nll of the reference (the usual interpolation that keeps the model from drifting off the transcripts).
    Called like CTCLoss: forward(log_probs_or_logits (T,B,C), targets, input_lengths, target_lengths).  Without gradient
    tracking it runs: ops.softmax_rows, ops.ctc_beam_decode with the decoder's own settings (its language model and hotwords
    included), the risks, then — when ctc_weight > 0 — ops.ctc_loss on the reference, which writes ctc_weight * (softmax - occ), and
    ops.ctc_mwer, which adds its gradient to that.

    The posteriors p_k come from the CTC likelihood RECOMPUTED for each hypothesis (ds2_ctc_mwer_f32's lattices), not from the
    decoder's scores: those hold language-model and hotword terms and are no function of the logits alone.  The search only chooses
    the list.  A slot is valid when its score is > -inf (the beam search fills fewer slots than beam_width on short utterances).

      nbest         slots kept, <= decoder.beam_width
      risk="label"  Levenshtein distance between the hypothesis' and the reference's label ids, spaces included (ops.edit_distance
                    on the device: the call makes no host synchronisation)
      risk="word"   Decoder.wer's word distance, packed by decoders.pack_scoring on the HOST: the hypotheses are copied to the host
                    first, one synchronisation per call (DeepSpeechTrainer.step refuses it for that reason)
      max_hyp_len   bound on a hypothesis' length, None = T (a beam search emits nothing longer than T_b).  It sizes the
                    workspace: 8 B nbest T (2 max_hyp_len + 1) bytes, about 1 GB at B = 64, nbest = 4, T = 501; a hypothesis longer
                    than the bound counts as infeasible.
      reduction     "sum" (default), "none" or "mean" (over the batch)
    `last_nbest` = (labels (B,nbest,T), lens, valid, risk, post (B,nbest)) of the last call, on the GPU.
    Whether this lowers the WER of a real corpus, and which nbest / ctc_weight serve it, is not measured here."""

    def __init__(self, decoder, nbest: int = 4, ctc_weight: float = 0.01, risk: str = "label", max_hyp_len=None, reduction: str = "sum"):
        super().__init__()
        if risk not in ("label", "word"):
            raise ValueError(f"MWERLoss: risk must be 'label' or 'word', got {risk!r}")
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(reduction)
        if not hasattr(decoder, "beam_width"):
            raise TypeError("MWERLoss needs a BeamCTCDecoder: the n-best list is its beam")
        if not 1 <= int(nbest) <= int(decoder.beam_width):
            raise ValueError(f"MWERLoss: nbest = {nbest} must lie in 1 .. decoder.beam_width = {decoder.beam_width}")
        if decoder.blank_index != 0:
            raise ValueError("the HIP CTC kernels fix blank = 0")
        cw = float(ctc_weight)
        if not (cw >= 0.0 and math.isfinite(cw)):
            raise ValueError(f"MWERLoss: ctc_weight must be finite and >= 0, got {ctc_weight}")
        if max_hyp_len is not None and int(max_hyp_len) < 0:
            raise ValueError(f"MWERLoss: max_hyp_len must be >= 0, got {max_hyp_len}")
        self.decoder, self.nbest, self.ctc_weight, self.risk = decoder, int(nbest), cw, risk
        self.max_hyp_len = None if max_hyp_len is None else int(max_hyp_len)
        self.reduction = reduction
        self.last_nbest = None

    def _word_risk(self, labels, lens, targets_host, B, K, dev):
        """Decoder.wer's distance of every kept beam to its reference -> (B, K) fp32 on dev.  Copies the beams to the host."""
        from .decoders import pack_scoring
        if targets_host is None:
            raise ValueError("MWERLoss(risk='word') needs the host targets")
        t_h, off_h, tl_h, _ = _prep_targets_host(*targets_host)
        dec = self.decoder
        lab_h, len_h = labels[:, :K].cpu(), lens.cpu()                       # the synchronisation
        refs = ["".join(dec._char(int(i)) for i in t_h[int(off_h[b]):int(off_h[b]) + int(tl_h[b])].tolist()) for b in range(B)]
        hyps = dec.convert_to_strings(lab_h, len_h)
        seq, a_off, a_len, b_off, b_len, _, _ = pack_scoring([h for b in range(B) for h in hyps[b]], [refs[b] for b in range(B) for _ in range(K)])
        P = B * K                                                            # the first P problems are the word problems
        seq_dev = torch.from_numpy(seq).to(dev) if seq.size else torch.zeros(1, dtype=torch.int32, device=dev)
        dist = ops.edit_distance(seq_dev, torch.from_numpy(a_off[:P]), torch.from_numpy(a_len[:P]), torch.from_numpy(b_off[:P]),
                                 torch.from_numpy(b_len[:P]))
        return dist.to(torch.float32).view(B, K)

    def run(self, x, tg, off, il, tl, max_u, scale, want_grad, targets_host=None):
        """The device half of a call (also DeepSpeechTrainer.step's): x (T,B,C) fp32 logits or log-probabilities as ops.ctc_loss
        takes them; tg / off / il / tl the flat targets, their offsets, the input and the target lengths as int32 GPU tensors;
        max_u the longest target.  Returns (value (B) = loss_b + ctc_weight * nll_ref_b, gradient of sum_b value_b times `scale`
        or None).  With risk="label" nothing here waits for the device."""
        T, B, C = x.shape
        dev = x.device
        dec, K, Kw = self.decoder, self.nbest, int(self.decoder.beam_width)
        if K > Kw:
            raise ValueError(f"MWERLoss: nbest = {K} exceeds decoder.beam_width = {Kw}")
        rows = x.view(T * B, C) if x.is_contiguous() else x.as_strided((T * B, C), (x.stride(1), 1))
        probs = ops.softmax_rows(rows).view(T, B, C)
        # one int32 buffer: the beams' labels (B, Kw, T) in front, the flat references behind, so that every offset is affine in
        # (b, k) and one edit-distance launch sees both sides
        n_hyp = B * Kw * T
        if n_hyp + tg.numel() >= 2 ** 31:
            raise ValueError("MWERLoss: B * beam_width * T too large")
        buf = torch.empty(n_hyp + tg.numel(), dtype=torch.int32, device=dev)
        buf[n_hyp:].copy_(tg)
        labels = buf[:n_hyp].view(B, Kw, T)
        _, _, lens, scores = ops.ctc_beam_decode(probs.transpose(0, 1), il, dec.blank_index, Kw, dec.cutoff_top_n, dec.cutoff_prob, dec.lm,
                                                 dec.alpha, dec.beta, dec.hotwords, labels_out=labels)
        hyp_lens = lens[:, :K].contiguous()
        valid = (scores[:, :K] > -math.inf).to(torch.int32).contiguous()
        slot = torch.arange(B * K, device=dev, dtype=torch.int64)
        hyp_off = ((torch.div(slot, K, rounding_mode="floor") * Kw + slot % K) * T).view(B, K)
        if self.risk == "label":
            ref_off = (off.to(torch.int64) + n_hyp).repeat_interleave(K)
            ref_len = tl.repeat_interleave(K)
            dist = ops.edit_distance(buf, hyp_off.view(-1), hyp_lens.view(-1), ref_off, ref_len, max_len=max(T, int(max_u)))
            risk = dist.to(torch.float32).view(B, K)
        else:
            risk = self._word_risk(labels, hyp_lens, targets_host, B, K, dev)
        grad, nll_ref = None, None
        if self.ctc_weight > 0:
            nll_ref, grad = ops.ctc_loss(x, tg, off, il, tl, max_u, self.ctc_weight * scale, want_grad=want_grad)
        mh = T if self.max_hyp_len is None else self.max_hyp_len
        loss, _, post, grad = ops.ctc_mwer(x, buf, hyp_off, hyp_lens, valid, il, mh, risk, scale, want_grad=want_grad, grad=grad)
        self.last_nbest = (labels[:, :K], hyp_lens, valid, risk, post)
        value = loss if nll_ref is None else torch.add(loss, nll_ref, alpha=self.ctc_weight)
        return value, grad

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        if not log_probs.is_cuda:
            raise _lib.DS2LibraryError("asr_amd.MWERLoss needs GPU input (no CPU fallback; the CPU oracle is test-only)")
        want_grad = torch.is_grad_enabled() and log_probs.requires_grad
        value = _MWERFunction.apply(log_probs, self, targets, input_lengths, target_lengths, want_grad)
        if self.reduction == "none":
            return value
        return value.sum() if self.reduction == "sum" else value.mean()
