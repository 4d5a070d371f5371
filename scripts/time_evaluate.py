"""Time DeepSpeech.evaluate() with the WER / CER scoring on the host and on the GPU, in one process, at c3's shape: 5x1024 BiGRU,
B = 64 utterances of T_in = 1001 frames, 29 classes (blank, apostrophe, a-z, space), a randomly initialised model and synthetic
references of about 150 labels with a space every ~6.  Per batch it reports:
  - evaluate() with the host scoring: a GreedyDecoder subclass whose wer / cer are plain super() calls (evaluate() then keeps its
    per-utterance Decoder.wer / Decoder.cer loop);
  - evaluate() with the GPU scoring (the plain GreedyDecoder: Decoder.score_batch, one launch per batch);
  - eval forward + greedy decode alone, and the score_batch call alone on that batch's strings.
Both evaluate() runs must return the same (wer, cer).  Prints one JSON line.  Usage: python scripts/time_evaluate.py [--batches N] [--reps N]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return ms[len(ms) // 2], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=2, help="batches per evaluate() call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-labels", type=int, default=150)
    args = ap.parse_args()
    import bench
    from asr_amd import DeepSpeech
    from asr_amd.decoders import GreedyDecoder

    class HostScoring(GreedyDecoder):
        def wer(self, s1, s2):
            return super().wer(s1, s2)

        def cer(self, s1, s2):
            return super().cer(s1, s2)

    rnn, H, L, C, B, tin = bench.WORKLOADS["c3"]
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        with open(path, "w") as f:    # written by hand: the space label must be quoted, or read_csv drops it as a blank line
            f.write("label\n" + "\n".join(["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + ['" "']) + "\n")
        model = DeepSpeech(audio_conf=bench.audio_conf(), decoder=None, label_path=path, rnn_type=rnn, rnn_hidden_size=H,
                           rnn_hidden_layers=L, bidirectional=True)
    assert model.num_classes == C and model.labels[" "] == C - 1
    model.cuda().eval()
    x, _, pct, _ = bench.synthetic_batch(B, tin, C, 1)
    g = torch.Generator().manual_seed(2)
    tsz = torch.full((B,), args.ref_labels, dtype=torch.int32)
    targets = torch.randint(1, C - 1, (B * args.ref_labels,), generator=g, dtype=torch.int32)
    targets[torch.rand(targets.shape, generator=g) < 1 / 6] = C - 1     # the space label
    loader = [(x, targets, pct.clone(), tsz)] * args.batches
    lens = (pct * x.size(3)).int()
    xd = x.cuda()

    def fwd_decode():
        with torch.no_grad():
            out, out_lens = model.forward(xd, lens)
            return model.decoder.decode(out, out_lens)[0]

    res = dict(workload="c3", batch=B, input_frames=tin, classes=C, ref_labels=args.ref_labels, batches_per_call=args.batches, reps=args.reps)
    model.decoder = GreedyDecoder(model.labels)
    fd_ms, hyps = _wall(fwd_decode, args.reps)
    hyps = [h[0] for h in hyps]
    refs = [s[0] for s in model.decoder.convert_to_strings([targets[i * args.ref_labels:(i + 1) * args.ref_labels] for i in range(B)])]
    res["hyp_chars_mean"] = round(sum(len(h) for h in hyps) / B, 1)
    res["forward_decode_ms"] = round(fd_ms, 3)
    res["score_batch_ms"] = round(_wall(lambda: model.decoder.score_batch(hyps, refs), max(args.reps, 20))[0], 3)
    out = {}
    for name, dec in (("host", HostScoring(model.labels)), ("gpu", GreedyDecoder(model.labels))):
        model.decoder = dec
        ms, r = _wall(lambda: model.evaluate(loader=[(a, b, c.clone(), d) for a, b, c, d in loader], device="cuda")[:2], args.reps)
        res[f"evaluate_{name}_scoring_ms_per_batch"] = round(ms / args.batches, 3)
        out[name] = r
    res["same_wer_cer"] = out["host"] == out["gpu"]
    res["wer_cer"] = [round(v, 6) for v in out["gpu"]]
    print(json.dumps(res))
    if not res["same_wer_cer"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
