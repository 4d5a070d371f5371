"""`DeepSpeech` with the reference's constructor, `forward`, `get_seq_lens`, `get_loader`, eval
`__call__`, `finetune_from` and state_dict keys (asr_deepspeech/modules/deepspeech.py:24-288), whose
forward/backward run on the hand-written MI355X kernels (asr_amd/engine.py, libds2hip).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch
from torch import nn

from .. import _lib, engine, ops
from ..device import resolve_device
from ..params import FlatParams
from ..vars import resolve_rnn_type
from .blocks import BatchRNN, InferenceBatchSoftmax, Lookahead, MaskConv, SequenceWise


def _read_labels(label_path):
    """deepspeech.py:48 — {char: row index} from the `label` column of labels.csv (row 0 = CTC blank)."""
    import pandas as pd
    return dict([(v, k) for k, v in pd.read_csv(label_path).to_dict()["label"].items()])


class _DS2Function(torch.autograd.Function):
    """Whole-network autograd node: forward = kernel schedule, backward = hand-derived schedule.
    Parameters are passed as inputs so that `loss.backward()` populates `p.grad` like the reference."""

    @staticmethod
    def forward(ctx, model, x, lens_dev, *params):
        W = model._flat.tensors(model)
        logits, saved = engine.forward(W, model._cfg, x, lens_dev, training=model.training, save=True)
        ctx.model, ctx.saved = model, saved
        # backward runs on autograd's worker thread: it must go through the recurrence context of THIS thread (whose enable switches the
        # trainer set, and whose starvation record / cooldown the trainer reads), not through a fresh one of the worker's own
        ctx.rnn_ctx, ctx.device = ops.rnn_ctx(x.device), x.device
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        model = ctx.model
        W = model._flat.tensors(model)
        flat = model._flat
        # autograd installs the returned tensors as `p.grad` without a copy, i.e. p.grad then ALIASES the flat
        # gradient buffer (the zero-copy normal case: zero_grad(set_to_none=True) -> backward -> step).  If some
        # p.grad is still alive (gradient accumulation, zero_grad(set_to_none=False)) the kernels must not
        # overwrite it: compute into a scratch buffer and let autograd add.
        accumulating = any(p.grad is not None for p in model.parameters())
        if accumulating:
            if model._on_bucket is not None:
                # the data-parallel reducer all-reduces the flat gradient buffer bucket by bucket as backward fills it; gradients that
                # autograd adds up outside that buffer would silently stay un-reduced
                raise RuntimeError("asr_amd.DeepSpeech: gradient accumulation (p.grad still set when backward runs) is not supported "
                                   "under data parallelism; call optimizer.zero_grad() (set_to_none=True) before every backward")
            keep, flat.flat_grad = flat.flat_grad, torch.empty_like(flat.flat_grad)
        try:
            Gr = flat.tensors(model, grads=True)
            with ops.use_rnn_ctx(ctx.rnn_ctx, ctx.device), torch.cuda.device(ctx.device):
                engine.backward(W, Gr, model._cfg, ctx.saved, dlogits.contiguous(),
                                on_bucket=None if accumulating else model._on_bucket, serial_buckets=model._serial_buckets)
        finally:
            if accumulating:
                flat.flat_grad = keep
        ctx.saved = None
        grads = tuple(Gr[n] for n in model._param_names)
        return (None, None, None) + grads


class DeepSpeech(nn.Module):
    def __init__(self, audio_conf, decoder, label_path, id="asr", rnn_type="nn.LSTM", rnn_hidden_size=768, rnn_hidden_layers=5,
                 bidirectional=True, context=20, version="0.0.1", model_path=None, restart_from=None):
        super().__init__()
        self.version = version
        self.id = id
        self.decoder, self.audio_conf = decoder, audio_conf
        self.context = context
        self.rnn_hidden_size = rnn_hidden_size
        self.rnn_hidden_layers = rnn_hidden_layers
        self.rnn_type = resolve_rnn_type(rnn_type)
        self.labels = _read_labels(label_path)
        self.bidirectional = bidirectional
        self.sample_rate = self.audio_conf.sample_rate
        self.window_size = self.audio_conf.window_size
        self.num_classes = len(self.labels)
        self.model_path = model_path
        self.build_network()
        from ..decoders import GreedyDecoder
        self.decoder = GreedyDecoder(self.labels)
        self._flat: Optional[FlatParams] = None
        self._on_bucket = None          # DP hook: called as each layer's gradients become final
        self._serial_buckets = False    # ... by a reducer that orders its collectives into the compute stream (engine.backward)
        self._param_names = [n for n, _ in self.named_parameters()]
        kind = {nn.GRU: "gru", nn.LSTM: "lstm", nn.RNN: "rnn"}.get(self.rnn_type)
        self._cfg = engine.ModelCfg(rnn=kind or "unsupported", hidden=rnn_hidden_size, layers=rnn_hidden_layers,
                                    classes=self.num_classes, freq=int(math.floor(self.sample_rate * self.window_size / 2) + 1))

    # -- structure (deepspeech.py:58-110) -----------------------------------------------------------
    def build_network(self):
        self.conv = MaskConv(nn.Sequential(
            nn.Conv2d(1, 32, kernel_size=(41, 11), stride=(2, 2), padding=(20, 5)),
            nn.BatchNorm2d(32),
            nn.Hardtanh(0, 20, inplace=True),
            nn.Conv2d(32, 32, kernel_size=(21, 11), stride=(2, 1), padding=(10, 5)),
            nn.BatchNorm2d(32),
            nn.Hardtanh(0, 20, inplace=True),
        ))
        f = int(math.floor((self.sample_rate * self.window_size) / 2) + 1)
        f = int(math.floor(f + 2 * 20 - 41) / 2 + 1)
        f = int(math.floor(f + 2 * 10 - 21) / 2 + 1)
        rnn_input_size = f * 32
        rnns = [("0", BatchRNN(rnn_input_size, self.rnn_hidden_size, rnn_type=self.rnn_type, bidirectional=self.bidirectional,
                               batch_norm=False))]
        for i in range(self.rnn_hidden_layers - 1):
            rnns.append((str(i + 1), BatchRNN(self.rnn_hidden_size, self.rnn_hidden_size, rnn_type=self.rnn_type,
                                              bidirectional=self.bidirectional)))
        self.rnns = nn.Sequential(OrderedDict(rnns))
        self.lookahead = (nn.Sequential(Lookahead(self.rnn_hidden_size, context=self.context), nn.Hardtanh(0, 20, inplace=True))
                          if not self.bidirectional else None)
        fully_connected = nn.Sequential(nn.BatchNorm1d(self.rnn_hidden_size),
                                        nn.Linear(self.rnn_hidden_size, self.num_classes, bias=False))
        self.fc = nn.Sequential(SequenceWise(fully_connected))
        self.inference_softmax = InferenceBatchSoftmax()

    # -- flat parameter storage -------------------------------------------------------------------
    @property
    def precision(self) -> str:
        """"fp32" (default; the parity path) or "bf16" (bf16 MFMA operands for the input-to-hidden GEMMs, fp32
        accumulation / state / BN / CTC — the BASELINE configs[2],[4] setting)."""
        return self._cfg.precision

    @precision.setter
    def precision(self, value: str):
        if value not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self._cfg.precision = value

    def _ensure_flat(self, device):
        device = torch.device(device)
        if self._flat is None or self._flat.device != device or not self._flat.owns(self):
            old = self._flat
            self._flat = FlatParams(self, self.rnn_hidden_layers, device)
            for b_name, b in list(self.named_buffers()):
                if b.device != device:
                    mod, _, leaf = b_name.rpartition(".")
                    setattr(self.get_submodule(mod), leaf, b.to(device))
            del old
        return self._flat

    def flat_parameters(self):
        """(flat params, flat grads) fp32 buffers — the fused optimizer / RCCL all-reduce operate on these."""
        assert self._flat is not None, "call model.to(device) and run one forward (or _ensure_flat) first"
        return self._flat.flat, self._flat.flat_grad

    def finetune_from(self, model_path, nlayers=1):
        """deepspeech.py:112-128: shape-checked partial load, then freeze all but the last n tensors."""
        state_dict = self.state_dict()
        loaded = torch.load(model_path, map_location="cpu")
        loaded = loaded.get("state_dict", loaded) if isinstance(loaded, dict) else loaded
        for k, v in loaded.items():
            if k in state_dict and state_dict[k].shape == v.shape:
                state_dict[k] = v
            else:
                print(k, state_dict.get(k, torch.empty(0)).shape, v.shape)
        self.load_state_dict(state_dict)
        print(f"finetune from {model_path} (last {nlayers} layers)")
        if nlayers is not None:
            for m in list(self.parameters())[:-nlayers]:
                m.requires_grad = False

    # -- forward (deepspeech.py:130-149) ----------------------------------------------------------
    def forward(self, x: torch.Tensor, lengths: torch.Tensor):
        lengths = torch.as_tensor(lengths).cpu().int()
        output_lengths = self.get_seq_lens(lengths)
        if not self.bidirectional:
            return self._forward_unidirectional(x, output_lengths)
        if self._cfg.rnn == "unsupported":
            raise NotImplementedError(f"no MI355X kernels for rnn_type {self.rnn_type!r}: the cells of asr_amd.vars.supported_rnns "
                                      "(nn.GRU, nn.LSTM, nn.RNN) are")
        if not x.is_cuda:
            raise _lib.DS2LibraryError(
                "asr_amd.DeepSpeech.forward needs GPU input: the MI355X HIP kernels are the only implementation. "
                "(The CPU restatement used for parity checks lives in oracle/ and is test infrastructure.)")
        _lib.load()
        self._ensure_flat(x.device)
        lens_dev = output_lengths.to(x.device, non_blocking=True)
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if needs_grad:
            params = [p for _, p in self.named_parameters()]
            logits = _DS2Function.apply(self, x, lens_dev, *params)
        else:
            if not self.training and ops.rnn_poison_seen(x.device):
                # an EARLIER inference forward of this process was handed NaN logits (below) and nobody has settled the starvation since:
                # settle it now — raises DS2LibraryError naming the launch, clears the record and moves the next recurrence calls onto the
                # step kernels, so a caller that only ever calls forward() sees the failure once and then keeps working
                ops.rnn_persistent_check(x.device)
            W = self._flat.tensors(self)
            logits, _ = engine.forward(W, self._cfg, x, lens_dev, training=self.training, save=False)
            if not self.training:
                # A persistent recurrence launch that could not get all of its workgroups resident leaves invalid activations.  Inference
                # must never return them, and must not pay a device synchronisation per forward either (streaming / batched inference
                # would lose all host-device overlap), nor consume the starvation record of a trainer's un-settled step: a kernel in
                # stream order turns the logits into NaN if a launch before it starved (fp32 shapes take the persistent kernels too),
                # and the record stays for the next check at a natural sync point (evaluate() below, the trainer's step / synchronize,
                # the decoders' device-to-host copy) — or, for callers that only ever call forward(), the NEXT forward: the poison kernel
                # raises a pinned host flag that the test above reads without synchronising.
                ops.rnn_poison_if_starved(logits)
        out = logits.transpose(0, 1)            # (B,T,C) view, like the reference's x.transpose(0, 1)
        out = self.inference_softmax(out)       # identity in train, HIP softmax in eval
        return out, output_lengths

    def _forward_unidirectional(self, x, output_lengths):
        """`bidirectional=False` (+ Lookahead, deepspeech.py:83-101, :142-143): not on any BASELINE configuration and not a kernel target
        ("keep as PyTorch fallback") — the reference's op sequence on torch ops with torch autograd, on whatever device
        the module lives on, so that a unidirectional checkpoint of the reference loads, evaluates and fine-tunes behind the same class.
        The MI355X kernels, the fused `trainer.step` and the data-parallel reducer are for the bidirectional model only."""
        if not getattr(self, "_uni_note", False):
            self._uni_note = True
            print("[asr_amd] unidirectional DeepSpeech: this variant runs on torch ops (no MI355X kernels; SURVEY.md §2 row 1)", flush=True)
        keep = (torch.arange(int(output_lengths.max()) if output_lengths.numel() else 0, device=x.device).view(1, 1, 1, -1)
                < output_lengths.to(x.device).view(-1, 1, 1, 1))
        h = x
        for m in self.conv.seq_module:                       # MaskConv (blocks.py:42-56): every stage's output is zeroed beyond each utterance
            h = m(h)
            t = h.size(3)
            live = keep[..., :t] if keep.size(3) >= t else torch.nn.functional.pad(keep, (0, t - keep.size(3)))
            h = h * live
        b, c, d, t = h.shape
        h = h.reshape(b, c * d, t).permute(2, 0, 1).contiguous()                     # (T, N, c*D + d)
        for rnn in self.rnns:
            h = rnn(h, output_lengths)
        h = self.lookahead(h)
        h = self.fc(h).transpose(0, 1)
        if not self.training:
            h = torch.softmax(h, dim=-1)
        return h, output_lengths

    def get_loader(self, manifest, batch_size, num_workers, caching=False, front_end="host", perturb=False, prefetch=0,
                   resample=False, star=None):
        from ..data import get_loader
        return get_loader(self.audio_conf, self.labels, manifest, batch_size, num_workers, caching=caching, front_end=front_end,
                          perturb=perturb, prefetch=prefetch, resample=resample, star=star)

    def get_seq_lens(self, input_length: torch.Tensor) -> torch.Tensor:
        """deepspeech.py:275-288: true division per Conv2d on the time axis, one truncation at the end."""
        seq_len = input_length
        for m in self.conv.modules():
            if isinstance(m, nn.modules.conv.Conv2d):
                seq_len = (seq_len + 2 * m.padding[1] - m.dilation[1] * (m.kernel_size[1] - 1) - 1) / m.stride[1] + 1
        return seq_len.int()

    # -- forced alignment (no counterpart in the reference) --------------------------------------
    def align(self, inputs, input_sizes, transcripts, star=None, star_penalty=math.log(0.5), unknown="error", free_start=False,
              free_end=False):
        """When each transcript was spoken: the eval-mode forward, then CTCAligner on its output.  inputs (B,1,F,T) and input_sizes
        (B) as forward() takes them, transcripts B strings (or label-id sequences).  Returns CTCAligner.align's records with every
        token and word tuple extended by (start_s, end_s): output frame t covers input frame 2t (the conv stack's time stride,
        get_seq_lens), so seconds = frame * 2 * audio_conf.window_stride.  The model is left in eval mode.
        star / star_penalty / unknown / free_start / free_end: CTCAligner.align's options for imperfect transcripts (a wildcard token,
        optional ends; see there, also for what the default penalty is not); the "unaligned" spans gain seconds too."""
        from ..decoders import CTCAligner, add_seconds
        self.eval()
        with torch.no_grad():
            out, output_sizes = self.forward(inputs, input_sizes)
            records = CTCAligner(self.labels).align(out, output_sizes, transcripts, star=star, star_penalty=star_penalty, unknown=unknown,
                                                    free_start=free_start, free_end=free_end)
        return add_seconds(records, 2.0 * float(self.audio_conf.window_stride))

    def posteriors_long(self, spect, window=2000, overlap=200, batch_size=32):
        """Posteriors of ONE recording of any length: spect (F,T) or (1,1,F,T), on the host or the device -> (T_out, C) fp32
        probabilities on the device, T_out = (T - 1) // 2 + 1.  The recording is cut into overlapping windows
        (functional.long_windows; window and overlap in input frames), the windows are stacked batch_size at a time, in order and
        zero-padded (the short last window sits last in its batch), run through the eval-mode forward() with their lengths, and each
        window's kept frames are copied into the result: no new model arithmetic, and no recurrence over more than window // 2 steps.
        The starvation check of evaluate() runs once after the last batch.  NOT CLAIMED: what a window edge costs in accuracy is
        unmeasured; the frames next to an inner edge were computed with `overlap` input frames of context on that side, and the overlap
        is the caller's knob.  The defaults (20 s windows, 2 s overlap at a 10 ms stride) keep the model near its training lengths.
        The model is left in eval mode."""
        probs = None
        for chunk, out, t_out in self._long_batches("posteriors_long", spect, window, overlap, batch_size):
            if probs is None:
                probs = torch.empty((t_out, out.size(2)), dtype=torch.float32, device=out.device)
            for n, (_, _, out_start, keep_from, keep_to) in enumerate(chunk):
                probs[out_start:out_start + keep_to - keep_from] = out[n, keep_from:keep_to]
        ops.rnn_persistent_check(probs.device)          # raise if a persistent recurrence of any batch starved (its rows are NaN then)
        return probs

    def _long_batches(self, who, spect, window, overlap, batch_size):
        """The window loop of posteriors_long and stream_long: yields (windows, out, t_out) per batch: the batch's windows as
        functional.long_windows lists them (start, length, out_start, keep_from, keep_to), the eval-mode forward's output for them
        (computed without gradients) and the recording's output frames.  The argument checks run when the first batch is asked for."""
        from ..functional import long_windows
        spect = torch.as_tensor(spect)
        if spect.dim() == 4 and spect.size(0) == 1 and spect.size(1) == 1:
            spect = spect[0, 0]
        if spect.dim() != 2:
            raise ValueError(f"{who}: spect must be (F,T) or (1,1,F,T), got {tuple(spect.shape)}")
        if int(batch_size) < 1:
            raise ValueError(f"{who}: batch_size must be positive")
        wins = long_windows(spect.size(1), window, overlap)
        self.eval()
        dev = spect.device if spect.is_cuda else next(self.parameters()).device
        for i in range(0, len(wins), int(batch_size)):
            chunk = wins[i:i + int(batch_size)]
            with torch.no_grad():
                x = torch.zeros((len(chunk), 1, spect.size(0), max(w[1] for w in chunk)), dtype=torch.float32, device=dev)
                for n, (start, length, _, _, _) in enumerate(chunk):
                    x[n, 0, :, :length] = spect[:, start:start + length]
                out, _ = self.forward(x, torch.tensor([w[1] for w in chunk], dtype=torch.int32))
            yield chunk, out, (spect.size(1) - 1) // 2 + 1

    def stream_long(self, spect, window=2000, overlap=200, batch_size=32, decoder=None, commit=False, max_lag=None):
        """The text of ONE recording of any length while it is being computed: a generator.  The forward of posteriors_long runs batch
        by batch (see there for the windows and for what is not claimed about their edges); each window's kept frames go, in time
        order, into one decoders.BeamStream of `decoder or self.decoder`, which must be a BeamCTCDecoder (TypeError otherwise; there is
        no streaming GreedyDecoder): ONE beam search over the whole recording, so a language model's context is never reset.  After
        each batch it yields {"text": the best text so far, "stable_text": the part of it no later item changes, "frames", "seconds":
        the output frames consumed and their time, "final": False}; the last item has "final": True, the text BeamCTCDecoder.decode()
        gives for posteriors_long's result, and "words": [(word, start, end, start_s, end_s)] as transcribe() gives them.  The
        starvation check of evaluate() runs with every item.  NOT MEASURED: whether this lowers WER against the segmented
        transcribe_long with a language model, and how far "stable_text" lags "text" on real recordings.  commit / max_lag go to
        BeamCTCDecoder.open_stream (see BeamStream): commit=True keeps the search's memory to its live tree and yields the same
        items; max_lag (frames) forces the text older than that, and then items may differ.  The model is left in eval mode."""
        from ..decoders import BeamCTCDecoder
        dec = decoder or self.decoder
        if not isinstance(dec, BeamCTCDecoder):
            raise TypeError(f"stream_long: needs a BeamCTCDecoder (given or self.decoder), got {type(dec).__name__}")
        return self._stream_long(dec.open_stream(commit=commit, max_lag=max_lag), spect, window, overlap, batch_size)

    def _stream_long(self, stream, spect, window, overlap, batch_size):
        from ..decoders import words_from_offsets
        fs = 2.0 * float(self.audio_conf.window_stride)
        for chunk, out, _ in self._long_batches("stream_long", spect, window, overlap, batch_size):
            kept = [n for n, w in enumerate(chunk) if w[4] > w[3]]      # (a short last window may keep no frame)
            for n in kept:
                rec = stream.feed(out[n, chunk[n][3]:chunk[n][4]], partial=n == kept[-1])
            if kept:
                yield {"text": rec[0]["text"], "stable_text": rec[0]["stable_text"], "frames": rec[0]["frames"],
                       "seconds": rec[0]["frames"] * fs, "final": False}
        frames = stream.frames[0]
        strings, offsets = stream.finish()
        text = strings[0][0]
        yield {"text": text, "stable_text": text, "frames": frames, "seconds": frames * fs, "final": True,
               "words": [w + (w[1] * fs, w[2] * fs) for w in words_from_offsets(text, offsets[0][0])]}

    def align_long(self, spect, transcript, window=2000, overlap=200, batch_size=32, star=None, star_penalty=math.log(0.5),
                   unknown="error", free_start=False, free_end=False):
        """When a transcript was spoken in ONE recording of any length: posteriors_long (see there for the windows and for what is not
        claimed about their edges), then the tiled lattice (CTCAligner.align(..., variant=3)), which has no limit on the frames or on
        the transcript's length beyond device memory.  Returns one record as align() does, seconds = frame * 2 * window_stride.
        star / star_penalty / unknown / free_start / free_end as in align()."""
        from ..decoders import CTCAligner, add_seconds
        probs = self.posteriors_long(spect, window, overlap, batch_size)
        records = CTCAligner(self.labels).align(probs[None], None, [transcript], variant=3, star=star, star_penalty=star_penalty,
                                                unknown=unknown, free_start=free_start, free_end=free_end)
        return add_seconds(records, 2.0 * float(self.audio_conf.window_stride))[0]

    # -- keyword search (no counterpart in the reference) -----------------------------------------
    def spot(self, inputs, input_sizes, keywords, threshold=0.5, max_hits=32):
        """Where the keywords were said: the eval-mode forward, then KeywordSpotter on its output.  inputs (B,1,F,T) and input_sizes
        (B) as forward() takes them, keywords a list of strings.  Returns KeywordSpotter.search's records per utterance with
        "start_s" / "end_s" added, seconds = frame * 2 * audio_conf.window_stride as in align().  threshold / max_hits: see
        KeywordSpotter, also for what the default threshold is not (a measured one) and for the missing word boundary.  The model is
        left in eval mode."""
        from ..decoders import KeywordSpotter
        spotter = KeywordSpotter(self.labels, keywords, threshold=threshold, max_hits=max_hits)
        self.eval()
        with torch.no_grad():
            out, output_sizes = self.forward(inputs, input_sizes)
            return spotter.search(out, output_sizes, frame_seconds=2.0 * float(self.audio_conf.window_stride))

    def spot_long(self, spect, keywords, window=2000, overlap=200, batch_size=32, threshold=0.5, max_hits=32):
        """Where the keywords were said in ONE recording of any length: posteriors_long (see there for the windows and for what is not
        claimed about their edges), then KeywordSpotter.search on the whole recording as one lattice per keyword: the kernel keeps no
        back-pointers, so nothing is tiled and the frames have no limit beyond device memory (12 bytes per keyword and frame).  Returns
        the recording's list of records as spot() does."""
        from ..decoders import KeywordSpotter
        spotter = KeywordSpotter(self.labels, keywords, threshold=threshold, max_hits=max_hits)
        probs = self.posteriors_long(spect, window, overlap, batch_size)
        return spotter.search(probs[None], None, frame_seconds=2.0 * float(self.audio_conf.window_stride))[0]

    def spot_stream(self, spect, keywords, window=2000, overlap=200, batch_size=32, threshold=0.5, max_hits=32, max_lag=None):
        """Where the keywords were said in ONE recording of any length, while it is being computed: a generator shaped like stream_long.
        The forward of posteriors_long runs batch by batch (see there for the windows and for what is not claimed about their edges);
        each window's kept frames go, in time order, into one decoders.KeywordStream (see there for max_lag and for what is not
        measured about it).  After each batch it yields {"detections": the records, as spot_long gives them, that became final in this
        step, each in exactly one item, "tentative": the detections on the frames so far that a later frame may still replace,
        "frames", "seconds": the output frames consumed and their time, "final": False}; the last item, after the stream's finish(),
        has "final": True and no tentative record.  Without max_lag the "detections" of all items together are spot_long's records.
        The model is left in eval mode."""
        from ..decoders import KeywordSpotter
        stream = KeywordSpotter(self.labels, keywords, threshold=threshold, max_hits=max_hits).open_stream(max_lag=max_lag)
        return self._spot_stream(stream, spect, window, overlap, batch_size)

    def _spot_stream(self, stream, spect, window, overlap, batch_size):
        fs = 2.0 * float(self.audio_conf.window_stride)
        plain = lambda recs, final: [{k: v for k, v in r.items() if k != "final"} for r in recs if r["final"] == final]
        for chunk, out, _ in self._long_batches("spot_stream", spect, window, overlap, batch_size):
            kept = [n for n, w in enumerate(chunk) if w[4] > w[3]]      # (a short last window may keep no frame)
            done = []
            for n in kept:
                recs = stream.feed(out[n, chunk[n][3]:chunk[n][4]], frame_seconds=fs)[0]
                done += plain(recs, True)
            if kept:
                yield {"detections": done, "tentative": plain(recs, False), "frames": stream.frames[0], "seconds": stream.frames[0] * fs,
                       "final": False}
        recs = stream.finish(frame_seconds=fs)[0]
        yield {"detections": plain(recs, True), "tentative": [], "frames": stream.frames[0], "seconds": stream.frames[0] * fs, "final": True}

    # -- transcription with times (no counterpart in the reference) -------------------------------
    def transcribe(self, inputs, input_sizes, decoder=None):
        """The text of each utterance with word times: the eval-mode forward, then `decoder or self.decoder or GreedyDecoder(labels)`
        on its output.  inputs (B,1,F,T) and input_sizes (B) as forward() takes them.  Returns one {"text", "words"} record per
        utterance: the best string and [(word, start, end, start_s, end_s)] (decoders.words_from_offsets: the frames are where a
        character was first emitted, not spans; align() gives spans), seconds = frame * 2 * audio_conf.window_stride as in align().
        The model is left in eval mode."""
        from ..decoders import GreedyDecoder, words_from_offsets
        dec = decoder or self.decoder or GreedyDecoder(self.labels)
        fs = 2.0 * float(self.audio_conf.window_stride)
        self.eval()
        with torch.no_grad():
            out, output_sizes = self.forward(inputs, input_sizes)
            strings, offsets = dec.decode(out, output_sizes)
        return [{"text": s[0], "words": [w + (w[1] * fs, w[2] * fs) for w in words_from_offsets(s[0], o[0])]}
                for s, o in zip(strings, offsets)]

    def transcribe_long(self, spect, window=2000, overlap=200, batch_size=32, decoder=None, threshold=0.9, min_gap=25, pad=5, max_len=1000,
                        decode_batch=64):
        """The text of ONE recording of any length, in timed segments: posteriors_long (see there for the windows and for what is not
        claimed about their edges), ops.ctc_segment (a frame whose blank probability is >= threshold is silent; silent runs of min_gap
        frames are pauses; segments are padded by up to `pad` frames and cut at their most silent frame when longer than max_len; the
        contract: include/ds2hip.h, ds2_ctc_segment_f32), one device-to-host copy of the segment list, then per batch of at most
        decode_batch segments (decoders.plan_segment_batches: longest first, so a batch pads to its own longest segment) one
        ops.ctc_segment_gather and one decoder.decode, spread over the GPU instead of one workgroup walking the whole recording.
        decoder: `decoder or self.decoder or GreedyDecoder(labels)`.  Returns {"text", "segments": [{"start", "end", "start_s", "end_s",
        "text", "words": [(word, start, end, start_s, end_s)], "forced"}]} (decoders.assemble_transcript), frames counted in the whole
        recording, seconds = frame * 2 * window_stride; with a BeamCTCDecoder every segment has "score", its best beam's.
        NOT MEASURED: the defaults are starting points — the threshold 0.9, the 0.5 s pause, the 0.1 s pad and the 20 s cap (at a 10 ms
        stride; the cap sits at the model's training lengths) have not been tuned, and which values serve real recordings is unmeasured;
        so is what the window edges cost (inherited from posteriors_long).  With a language model every segment starts from the <s>
        context; what that costs in WER against a whole-recording decode is unmeasured.  The model is left in eval mode."""
        from ..decoders import GreedyDecoder, check_segment_options, transcribe_posteriors
        dec = decoder or self.decoder or GreedyDecoder(self.labels)
        check_segment_options("transcribe_long", threshold, min_gap, pad, max_len, decode_batch)     # before the forward passes
        probs = self.posteriors_long(spect, window, overlap, batch_size)
        return transcribe_posteriors(probs, dec, threshold, min_gap, pad, max_len, decode_batch, 2.0 * float(self.audio_conf.window_stride))

    # -- word and character confidences (no counterpart in the reference) -------------------------
    def confidence(self, inputs, input_sizes, decoder=None, unit="word", margin=0):
        """How sure the text of each utterance is of its words: what transcribe() does, then CTCConfidence.score on the same
        posteriors with the decoded texts.  Returns one {"text", "words", "confidence"} record per utterance, "text" and "words" as
        transcribe() gives them; with unit="word", "confidence" is a list parallel to "words"; with unit="char" it has one entry per
        character of "text".  An entry is the probability that the utterance spells the text, given that the audio outside the unit's
        aligned span (widened by `margin` frames) spells the rest; NaN where it was not scored (a unit above 63 labels, a text whose
        alignment is infeasible).  NOT MEASURED: how the number calibrates on real recordings and which margin serves them (see
        decoders.CTCConfidence).  The model is left in eval mode."""
        from ..decoders import CTCConfidence, GreedyDecoder, words_from_offsets
        dec = decoder or self.decoder or GreedyDecoder(self.labels)
        fs = 2.0 * float(self.audio_conf.window_stride)
        self.eval()
        with torch.no_grad():
            out, output_sizes = self.forward(inputs, input_sizes)
            strings, offsets = dec.decode(out, output_sizes)
            scored = CTCConfidence(self.labels).score(out, output_sizes, [s[0] for s in strings], unit=unit, margin=margin)
        records = []
        for s, o, r in zip(strings, offsets, scored):
            words = [w + (w[1] * fs, w[2] * fs) for w in words_from_offsets(s[0], o[0])]
            want = len(words) if unit == "word" else len(s[0])
            conf = [u[3] for u in r["units"]] if r["units"] else [float("nan")] * want
            assert len(conf) == want, (len(conf), want)
            records.append({"text": s[0], "words": words, "confidence": conf})
        return records

    def confidence_long(self, spect, window=2000, overlap=200, batch_size=32, decoder=None, threshold=0.9, min_gap=25, pad=5, max_len=1000,
                        decode_batch=64, unit="word", margin=0):
        """transcribe_long() with confidences: posteriors_long once, decoders.transcribe_posteriors for the segments and their texts,
        then per batch of decoders.plan_segment_batches one ops.ctc_segment_gather and one CTCConfidence.score.  Returns
        transcribe_long's record in which every segment gains "confidence" (as in confidence(): parallel to the segment's "words", or
        one entry per character of its "text") and "units": [(text, start, end, confidence)] with the frames counted in the whole
        recording.  What is not measured about transcribe_long's defaults and about the confidence holds here too."""
        from ..decoders import CTCConfidence, GreedyDecoder, check_segment_options, plan_segment_batches, transcribe_posteriors
        dec = decoder or self.decoder or GreedyDecoder(self.labels)
        check_segment_options("confidence_long", threshold, min_gap, pad, max_len, decode_batch)     # before the forward passes
        probs = self.posteriors_long(spect, window, overlap, batch_size)
        result = transcribe_posteriors(probs, dec, threshold, min_gap, pad, max_len, decode_batch, 2.0 * float(self.audio_conf.window_stride))
        segs = result["segments"]
        scorer = CTCConfidence(self.labels)
        for idx in plan_segment_batches([s["end"] - s["start"] for s in segs], decode_batch):
            host = torch.zeros((3, len(idx)), dtype=torch.int32)          # one int32 image: utterance indices (all 0), starts, lengths
            host[1] = torch.tensor([segs[i]["start"] for i in idx], dtype=torch.int32)
            host[2] = torch.tensor([segs[i]["end"] - segs[i]["start"] for i in idx], dtype=torch.int32)
            d = host.to(probs.device)
            packed, sizes = ops.ctc_segment_gather(probs[None], d[0], d[1], d[2], int(host[2, 0]))
            for i, r in zip(idx, scorer.score(packed, sizes, [segs[i]["text"] for i in idx], unit=unit, margin=margin)):
                seg = segs[i]
                want = len(seg["words"]) if unit == "word" else len(seg["text"])
                conf = [u[3] for u in r["units"]] if r["units"] else [float("nan")] * want
                assert len(conf) == want, (len(conf), want)
                seg["confidence"] = conf
                seg["units"] = [(u[0], u[1] + seg["start"], u[2] + seg["start"], u[3]) for u in r["units"]]
        return result

    # -- evaluation loop (deepspeech.py:161-273) --------------------------------------------------
    def evaluate(self, loader=None, manifest=None, batch_size=None, device="auto", num_workers=32, verbose=False, half=False,
                 output_file=None, main_proc=True, errors=None, **_unused):
        """errors: a decoders.ErrorReport (None, the default: nothing below happens).  Every batch is then also aligned
        (decoder.align_batch: which words and characters are hits, substitutions, deletions, insertions) and fed to it, and
        errors.format() is appended to output_file's report.  The return value is the same either way.  A decoder that overrides
        wer or cer refuses it (ValueError): its own scoring is not what the kernel aligns."""
        from ..decoders import BeamCTCDecoder, Decoder, GreedyDecoder
        device = resolve_device(device)
        if errors is not None and not (type(self.decoder).wer is Decoder.wer and type(self.decoder).cer is Decoder.cer):
            raise ValueError("evaluate: errors= needs the built-in scoring; this decoder overrides wer or cer, which the alignment kernel "
                             "does not follow")
        with torch.no_grad():
            if loader is None:
                loader, _ = self.get_loader(manifest=manifest, batch_size=batch_size, num_workers=num_workers)
            decoder = self.decoder
            # WER / CER of the whole batch in one HIP launch (Decoder.score_batch, integers equal to wer / cer); a decoder that overrides
            # either method keeps the per-utterance calls, so its own scoring is what gets counted
            gpu_scoring = type(decoder).wer is Decoder.wer and type(decoder).cer is Decoder.cer
            self.eval()
            self.to(device)
            total_cer = total_wer = num_tokens = num_chars = 0
            output_data = []
            # per-utterance report (deepspeech.py:224-244): best / last / worst transcript by CER and a 10-bucket CER histogram
            hist = [0] * 10
            best = (float("inf"), "")
            worst = (-1.0, "")
            last_str = ""
            for data in loader:
                inputs, targets, input_percentages, target_sizes = data
                input_sizes = input_percentages.mul_(int(inputs.size(3))).int()
                inputs = inputs.to(device)
                split_targets, offset = [], 0
                for size in target_sizes:
                    split_targets.append(targets[offset:offset + size])
                    offset += size
                out, output_sizes = self.forward(inputs, input_sizes)
                decoded_output, _ = decoder.decode(out, output_sizes)   # (copies to the host: the device is idle behind it)
                ops.rnn_persistent_check(inputs.device)                 # raise if a persistent recurrence of this batch starved (the logits are NaN then)
                # a BeamCTCDecoder's convert_to_strings takes (beams, lengths): the targets are spelt by the greedy one on the same labels
                target_strings = (GreedyDecoder(self.labels) if isinstance(decoder, BeamCTCDecoder) else decoder).convert_to_strings(split_targets)
                if output_file is not None:
                    output_data.append((out.detach().cpu().numpy(), output_sizes.numpy(), target_strings))
                scores = None
                if gpu_scoring:
                    scores = decoder.score_batch([decoded_output[i][0] for i in range(len(target_strings))],
                                                 [target_strings[i][0] for i in range(len(target_strings))]).tolist()
                if errors is not None:
                    errors.add(decoder.align_batch([decoded_output[i][0] for i in range(len(target_strings))],
                                                   [target_strings[i][0] for i in range(len(target_strings))]))
                for i in range(len(target_strings)):
                    transcript, reference = decoded_output[i][0], target_strings[i][0]
                    if scores is not None:
                        wer_inst, n_tok, cer_inst, n_chr = scores[i]
                    else:
                        wer_inst, cer_inst = decoder.wer(transcript, reference), decoder.cer(transcript, reference)
                        n_tok, n_chr = len(reference.split()), len(reference.replace(" ", ""))
                    total_wer += wer_inst
                    total_cer += cer_inst
                    num_tokens += n_tok
                    num_chars += n_chr
                    wer_pct = min(100.0 * wer_inst / max(n_tok, 1), 100.0)
                    cer_pct = min(100.0 * cer_inst / max(n_chr, 1), 100.0)
                    hist[min(int(cer_pct // 10), 9)] += 1
                    last_str = f"Ref:{reference.lower()}\nHyp:{transcript.lower()}\nWER:{wer_pct}  - CER:{cer_pct}"
                    if cer_pct < best[0]:
                        best = (cer_pct, last_str)
                    if cer_pct > worst[0]:
                        worst = (cer_pct, last_str)
                    if verbose:
                        print(last_str)
            wer = float(total_wer) / max(num_tokens, 1)
            cer = float(total_cer) / max(num_chars, 1)
            if main_proc and output_file is not None:
                # same sections as the reference's report (deepspeech.py:249-271); its histogram is drawn by the third-party ascii_graph
                # package, this one by the loop below (same buckets and counts)
                peak = max(max(hist), 1)
                bars = [f"{k * 10:>3}-{k * 10 + 10:<3} | {'#' * round(40 * v / peak):<40} {v}" for k, v in enumerate(hist)]
                with open(output_file, "w") as f:
                    f.write("\n".join([f"===== {wer * 100:.2f}/{cer * 100:.2f} =====", "----- BEST -----", best[1], "----- LAST -----", last_str,
                                       "----- WORST -----", worst[1], "CER histogram"] + bars
                                      + ["=============================================\n"]))
                    if errors is not None:
                        f.write(errors.format())
                print(f"saved output to {output_file}")
            return wer * 100, cer * 100, output_data

    def tune_decoder(self, loader=None, manifest=None, batch_size=None, num_workers=32, decoder=None, lm=None,
                     alphas=tuple(0.25 * i for i in range(21)), betas=tuple(0.2 * i - 2.0 for i in range(21)), metric="wer", confirm=False,
                     device="auto"):
        """Choose the LM weights (alpha, beta) of a BeamCTCDecoder on a dev set from ONE decode of it: the eval forward per batch, the
        decoder's n-best lists rescored at every point of the alphas x betas grid (decoders.NBestRescorer, decoders.tune_lm_weights),
        instead of one evaluate() per grid point.  decoder: a BeamCTCDecoder (None: self.decoder); lm: the rescoring model, an ARPA
        path or an NgramLM (None: the decoder's own).  Returns tune_lm_weights' dict.  With confirm=True and a decoder that carries an
        LM the set is decoded once more with the chosen weights fused into the search, and that evaluate()'s (wer, cer) is reported
        under "confirmed": the number that rescoring only approximates; the decoder's own weights are restored afterwards.
        NOT measured: whether the weights chosen this way lower the WER of a real corpus, and how far they lie from the optimum of
        decoding again at every grid point.  Hotword terms are not part of the rescoring score."""
        from ..decoders import BeamCTCDecoder, GreedyDecoder, NBestRescorer, tune_lm_weights
        decoder = self.decoder if decoder is None else decoder
        if not isinstance(decoder, BeamCTCDecoder):
            raise ValueError("tune_decoder: the decoder must be a BeamCTCDecoder")
        rescorer = NBestRescorer(decoder, lm=lm)
        device = resolve_device(device)
        if loader is None:
            loader, _ = self.get_loader(manifest=manifest, batch_size=batch_size, num_workers=num_workers)
        spell = GreedyDecoder(self.labels)

        def batches():
            for inputs, targets, input_percentages, target_sizes in loader:
                input_sizes = input_percentages.mul(int(inputs.size(3))).int()
                out, output_sizes = self.forward(inputs.to(device), input_sizes)
                ops.rnn_persistent_check(out.device)
                split, offset = [], 0
                for size in target_sizes:
                    split.append(targets[offset:offset + size])
                    offset += size
                yield out, output_sizes, spell.convert_to_strings(split)

        with torch.no_grad():
            self.eval()
            self.to(device)
            result = tune_lm_weights(rescorer, batches(), alphas, betas, metric)
            if confirm and decoder.lm is not None:
                kept = (self.decoder, decoder.alpha, decoder.beta)
                try:
                    self.decoder, decoder.alpha, decoder.beta = decoder, result["alpha"], result["beta"]
                    result["confirmed"] = self.evaluate(loader=loader, device=device)[:2]
                finally:
                    self.decoder, decoder.alpha, decoder.beta = kept
        return result

    def fit_lm(self, manifest, order=3, mode=None, path=None, alpha=None, beta=None, decoder=None, device=None, prune=None,
               min_count=None):
        """Estimate an n-gram language model from the `text` column of a manifest CSV and load it into a BeamCTCDecoder (None:
        self.decoder): BeamCTCDecoder.fit_lm on the transcripts, whose arguments these are.  Returns the NgramEstimate.  The transcripts
        should be spelt as the labels spell them (the manifests the loaders read are).  tune_decoder then finds alpha and beta."""
        from ..decoders import BeamCTCDecoder
        from ..decoders.lm_train import manifest_sentences
        decoder = self.decoder if decoder is None else decoder
        if not isinstance(decoder, BeamCTCDecoder):
            raise ValueError("fit_lm: the decoder must be a BeamCTCDecoder")
        return decoder.fit_lm(manifest_sentences(manifest), order=order, mode=mode, path=path, alpha=alpha, beta=beta, device=device,
                              prune=prune, min_count=min_count)

    def __call__(self, *args, **kwargs):
        """The reference overrides __call__ with its eval loop (deepspeech.py:161).  Keep that calling
        convention (`model(loader=..., device=...)`) and fall through to nn.Module for tensors."""
        if args and torch.is_tensor(args[0]):
            return super().__call__(*args, **kwargs)
        return self.evaluate(*args, **kwargs)
