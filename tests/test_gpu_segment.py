"""GPU (-m gpu): the pause segmentation (csrc/ctc_segment.h, `ds2_ctc_segment_f32`) against tests/ctc_segment_oracle.py, every output to
the integer, at the smallest shapes that cross the 64-frame word seams; the gather (`ds2_ctc_segment_gather_f32`) against torch slicing,
bit for bit; the segment -> gather -> batched decode -> assemble pipeline against whole-recording and per-slice decodes; and
DeepSpeech.transcribe / transcribe_long through a tiny model.  The problems and their oracle results live in tests/segment_problems.py
(checked on the CPU by tests/test_cpu_segment.py)."""
import numpy as np
import pytest
import torch

import ctc_segment_oracle as O
import segment_problems as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def run_segment(dev, c, x_dev=None):
    from asr_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(c["x"])).to(dev) if x_dev is None else x_dev
    sizes = None if c["in_lens"] is None else torch.tensor(c["in_lens"], dtype=torch.int32)
    out = ops.ctc_segment(x, sizes, c["blank"], c["thr"], c["min_gap"], c["pad"], c["max_len"], c["is_log"], max_segs=c["max_segs"])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def assert_equal_to_the_integer(got, want, what):
    for name, g, w in zip(("seg_start", "seg_end", "seg_flags", "n_segs"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name, g, w)


# ---- segmentation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.gpu_cases()))
def test_segments_equal_the_oracle(dev, name):
    c = P.gpu_cases()[name]
    assert_equal_to_the_integer(run_segment(dev, c), c["want"], name)


def test_overflow_reports_the_full_count(dev):
    c = P.gpu_cases()["overflow"]
    got = run_segment(dev, c)
    b = int(got[3].argmax())
    assert got[3][b] == c["max_segs"] + 3 and got[0].shape == (3, c["max_segs"]) and (got[0][b] >= 0).all()    # every slot used, three dropped


def test_strided_view_gives_the_same_segments(dev):
    c = P.gpu_cases()["ragged.257"]
    tbc = torch.from_numpy(c["x"]).to(dev).transpose(0, 1).contiguous()          # (T,B,C) storage, as the model's eval output
    view = tbc.transpose(0, 1)
    assert view.shape == c["x"].shape and view.stride(2) == 1 and view.stride(0) < view.stride(1)
    assert_equal_to_the_integer(run_segment(dev, c, x_dev=view), c["want"], "strided")


def test_default_max_segs_is_never_exceeded(dev):
    from asr_amd import ops
    c = P.gpu_cases()["random.257"]
    x = torch.from_numpy(c["x"]).to(dev)
    start, end, flags, n = ops.ctc_segment(x, torch.tensor(c["in_lens"]), 0, c["thr"], 1, 0, 2)     # the most segments any options give
    assert start.shape == (3, ops.segment_max_segs(257, 1, 2)) and int(n.max()) <= start.shape[1]
    want = O.segment_batch(c["x"], c["in_lens"], 0, np.float32(c["thr"]), 1, 0, 2, start.shape[1])
    assert_equal_to_the_integer([t.cpu().numpy() for t in (start, end, flags, n)], want, "max_len = 2")


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def test_gather_equals_slicing_bit_for_bit(dev):
    from asr_amd import ops
    x = P.gpu_cases()["ragged.257"]["x"].copy()
    x[1, 40, 3], x[2, 7, 0] = np.float32("nan"), np.float32(-0.0)               # bits, not values
    B, T, C = x.shape
    t_max = 70
    #       a segment of t_max frames exactly ......... the last frame ... rejected: b = B, b < 0, start < 0, len < 0, beyond T, len > t_max
    seg_b = [0, 1, 2, 1, 0, 2, B, -1, 0, 1, 2, 0]
    seg_s = [0, 30, 187, 64, 256, 0, 0, 0, -1, 5, 250, 10]
    seg_n = [70, 33, 70, 1, 1, 0, 4, 4, 4, -2, 8, 71]
    want_out, want_sizes = O.gather(x, seg_b, seg_s, seg_n, t_max)
    assert want_sizes.tolist() == [70, 33, 70, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    xd = torch.from_numpy(x).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    for src in (xd, xd.transpose(0, 1).contiguous().transpose(0, 1)):
        out, sizes = ops.ctc_segment_gather(src, i32(seg_b), i32(seg_s), i32(seg_n), t_max)
        torch.cuda.synchronize()
        assert out.shape == (12, t_max, C) and out.is_contiguous() and sizes.cpu().tolist() == want_sizes.tolist()
        assert np.array_equal(out.cpu().numpy().view(np.int32), want_out.view(np.int32))
        for s in range(5):                                                       # against torch slicing on the device
            assert torch.equal(out[s, :seg_n[s]].view(torch.int32), xd[seg_b[s], seg_s[s]:seg_s[s] + seg_n[s]].view(torch.int32))
            assert not out[s, seg_n[s]:].view(torch.int32).any()
    empty, none = ops.ctc_segment_gather(xd, i32([]), i32([]), i32([]), 4)
    assert empty.shape == (0, 4, C) and none.shape == (0,)


# ---- the pipeline on planted posteriors -------------------------------------------------------------------------------------------
def recording(cls, *args, **kwargs):
    """A decoder that keeps what every decode() call returned: (sizes, strings, offsets, scores or None) per call."""
    class Recording(cls):
        def decode(self, probs, sizes=None):
            out = super().decode(probs, sizes)
            self.calls.append((sizes.cpu().tolist(), out[0], out[1], getattr(self, "last_scores", None)))
            return out
    dec = Recording(*args, **kwargs)
    dec.calls = []
    return dec


def run_pipeline(dev, dec, decode_batch=5):
    """-> (record, the oracle's segments, per segment in time order the (string, offsets + start, score) that the batched decodes gave)"""
    from asr_amd.decoders import plan_segment_batches, transcribe_posteriors
    x, _ = P.pipeline_problem()
    rec = transcribe_posteriors(torch.from_numpy(x).to(dev), dec, P.PIPE["thr"], P.PIPE["min_gap"], P.PIPE["pad"], P.PIPE["max_len"],
                                decode_batch=decode_batch, frame_seconds=0.02)
    segs = O.segment_one(x[:, 0], np.float32(P.PIPE["thr"]), P.PIPE["min_gap"], P.PIPE["pad"], P.PIPE["max_len"])
    assert [(s["start"], s["end"], s["forced"]) for s in rec["segments"]] == segs and len(segs) >= 12
    batches = plan_segment_batches([e - s for s, e, _ in segs], decode_batch)
    assert len(dec.calls) == len(batches) == -(-len(segs) // decode_batch)
    decoded = [None] * len(segs)
    for idx, (sizes, strings, offsets, scores) in zip(batches, dec.calls):
        assert sizes == [segs[i][1] - segs[i][0] for i in idx]                   # longest first: the batch pads to its first segment
        for j, i in enumerate(idx):
            decoded[i] = (strings[j][0], [int(o) + segs[i][0] for o in offsets[j][0]], None if scores is None else float(scores[j, 0]))
    return rec, segs, decoded


def test_pipeline_with_the_greedy_decoder_equals_the_whole_recording_decode(dev):
    from asr_amd.decoders import GreedyDecoder, words_from_offsets
    x, _ = P.pipeline_problem()
    dec = recording(GreedyDecoder, P.LABELS)
    rec, segs, decoded = run_pipeline(dev, dec)
    strings, offsets = GreedyDecoder(P.LABELS).decode(torch.from_numpy(x).to(dev)[None])
    assert "".join(t for t, _, _ in decoded) == strings[0][0] == "".join(P.PHRASES)
    assert [o for _, offs, _ in decoded for o in offs] == offsets[0][0].tolist()
    for s, (text, offs, _) in zip(rec["segments"], decoded):                     # the record holds what the decodes gave, in time order
        assert s["text"] == text and "score" not in s
        assert [w[:3] for w in s["words"]] == words_from_offsets(text, offs)
        assert all(w[3] == w[1] * 0.02 and w[4] == w[2] * 0.02 for w in s["words"])
    assert rec["text"] == " ".join(t for t in (s["text"].strip() for s in rec["segments"]) if t)
    assert [s["text"] for s in rec["segments"] if not s["forced"]] == [p for p in P.PHRASES if p not in (P.PHRASES[2], "all good things")]          # (those two are longer than max_len)


def test_pipeline_with_the_beam_decoder_equals_each_slice_decoded_alone(dev):
    from asr_amd.decoders import BeamCTCDecoder, words_from_offsets
    x, _ = P.pipeline_problem()
    xd = torch.from_numpy(x).to(dev)
    rec, segs, decoded = run_pipeline(dev, recording(BeamCTCDecoder, P.LABELS, beam_width=8))
    alone = BeamCTCDecoder(P.LABELS, beam_width=8)
    for s, (text, offs, score) in zip(rec["segments"], decoded):
        strings, offsets = alone.decode(xd[None, s["start"]:s["end"]])
        want = (strings[0][0], [int(o) + s["start"] for o in offsets[0][0]], float(alone.last_scores[0, 0]))
        assert (text, offs, score) == want, (s["start"], s["end"])
        assert s["text"] == text and s["score"] == score and [w[:3] for w in s["words"]] == words_from_offsets(text, offs)


# ---- the model methods -----------------------------------------------------------------------------------------------------------
def test_transcribe_and_transcribe_long_through_a_tiny_model(dev):
    from asr_amd import ops
    from asr_amd.decoders import BeamCTCDecoder
    from test_gpu_align_long import spectrogram, tiny_model
    model = tiny_model()
    x = torch.stack((spectrogram(100), spectrogram(100).flip(1)))[:, None]
    recs = model.transcribe(x.to(dev), torch.tensor([100, 77], dtype=torch.int32))
    assert len(recs) == 2 and all(set(r) == {"text", "words"} for r in recs) and not model.training
    with torch.no_grad():
        out, sizes = model.forward(x.to(dev), torch.tensor([100, 77], dtype=torch.int32))
        strings, _ = model.decoder.decode(out, sizes)
    assert [r["text"] for r in recs] == [s[0] for s in strings]
    for r in recs:
        assert [w[0] for w in r["words"]] == r["text"].split()
        assert all(w[3] == w[1] * 0.02 and w[4] == w[2] * 0.02 and 0 <= w[1] < w[2] <= 50 for w in r["words"])

    spect = spectrogram(437)
    opts = dict(threshold=0.05, min_gap=2, pad=1, max_len=30)                   # a random-init model: a low bar makes pauses at all
    for decoder in (None, BeamCTCDecoder(model.labels, beam_width=4)):
        rec = model.transcribe_long(spect, window=128, overlap=16, batch_size=3, decoder=decoder, decode_batch=4, **opts)
        probs = model.posteriors_long(spect, window=128, overlap=16, batch_size=3)
        start, end, flags, n = (t.cpu().numpy() for t in ops.ctc_segment(probs[None], None, 0, **opts))
        assert set(rec) == {"text", "segments"} and len(rec["segments"]) == int(n[0]) >= 1
        keys = {"start", "end", "start_s", "end_s", "text", "words", "forced"} | ({"score"} if decoder is not None else set())
        for i, s in enumerate(rec["segments"]):
            assert set(s) == keys and (s["start"], s["end"], s["forced"]) == (start[0, i], end[0, i], flags[0, i])
            assert s["start_s"] == s["start"] * 0.02 and s["end_s"] == s["end"] * 0.02
            assert all(w[3] == w[1] * 0.02 and w[4] == w[2] * 0.02 and s["start"] <= w[1] < w[2] <= s["end"] for w in s["words"])
        assert rec["text"] == " ".join(t for t in (s["text"].strip() for s in rec["segments"]) if t)
    for bad in (dict(threshold=0.0), dict(threshold=1.5), dict(min_gap=0), dict(pad=-1), dict(max_len=1), dict(decode_batch=0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            model.transcribe_long(spect, window=128, overlap=16, **bad)
    with pytest.raises(ValueError, match="spect"):
        model.transcribe_long(torch.zeros(3, 161, 50))
