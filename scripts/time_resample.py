"""Time the sample-rate conversion of the waveform feed (ops.wave_resample, ds2_wave_resample_f32) against the plain unpack pass
(ops.wave_unpack) on the same audio already at 16 kHz.
  kernel legs  one packed int16 batch of B = 64 utterances of 10 s at 48 kHz (480000 samples each), the same at 44.1 kHz, and at
               16 kHz for the unpack pass; every leg ends in the same (64, 160000) fp32 batch shape.  Per leg: `--iters` calls between
               two device events, after `--warmup` calls; the legs are alternated over `--rounds` rounds in one process; mean and
               round-to-round spread (max - min) of the ms per call, and the bytes the pass has to move (packed in + fp32 out) over it.
  --feed       a feed run in the manner of scripts/time_feed.py: ms per iteration of `for data in loader: trainer.step(data)` at the
               metric config c3 with prefetch=2 over `--batches` batches of 64 files of 10 s, once from a 16 kHz corpus (resample=False)
               and once from the same corpus at 48 kHz (resample=True), alternated; the floor is the step on a resident batch.
Prints one JSON line.  Usage: python scripts/time_resample.py [--iters N] [--warmup N] [--rounds N] [--feed] [--batches N] [--workers N]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

B, SECONDS, TARGET = 64, 10, 16000


def batch_at(rate, dev):
    from asr_amd.data import pack_waveforms
    n = rate * SECONDS
    rng = np.random.default_rng(rate)
    t = np.arange(n) / rate
    base = (8000 * np.sin(2 * np.pi * 220.0 * t) + 5000 * np.sin(2 * np.pi * 1700.0 * t) + 1500 * rng.standard_normal(n)).astype(np.int16)
    buf, off, ln, _ = pack_waveforms([(np.roll(base, 977 * i), []) for i in range(B)])
    return buf.to(dev), off, ln


def kernel_legs(args, dev):
    from asr_amd import ops
    legs, moved = {}, {}
    for rate in (16000, 48000, 44100):
        buf, off, ln = batch_at(rate, dev)
        if rate == TARGET:
            legs["unpack_16k_ms"] = lambda buf=buf, off=off, ln=ln: ops.wave_unpack(buf, off, ln)
        else:
            legs[f"resample_{rate // 1000}k_ms"] = lambda buf=buf, off=off, ln=ln, r=rate: ops.wave_resample(buf, off, ln, [r] * B, None, TARGET)
        moved[list(legs)[-1]] = buf.numel() * 2 + B * TARGET * SECONDS * 4
    times = {k: [] for k in legs}
    for k, fn in legs.items():
        out = fn()
        assert tuple((out[0] if isinstance(out, tuple) else out).shape) == (B, TARGET * SECONDS), k
    for _ in range(args.rounds):                                     # alternate so that drift on a shared host hits all legs
        for k, fn in legs.items():
            for _ in range(args.warmup):
                fn()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop) / args.iters)
    res = {}
    for k in legs:
        res[k] = round(float(np.mean(times[k])), 4)
        res[k + "_rounds"] = [round(v, 4) for v in times[k]]
        res[k.replace("_ms", "_spread_ms")] = round(max(times[k]) - min(times[k]), 4)
        res[k.replace("_ms", "_MB_moved")] = round(moved[k] / 1e6, 1)
        res[k.replace("_ms", "_TBps")] = round(moved[k] / (res[k] * 1e-3) / 1e12, 3)
    return res


def feed_legs(args, dev):
    import pandas as pd
    from scipy.io import wavfile
    from time_feed import CLASSES, conf
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW
    from asr_amd.data import get_loader, write_manifest
    from asr_amd.trainers import DeepSpeechTrainer
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        letters = list("abcdefghijklmnopqrstuvwxyz")
        texts = ["".join(rng.choice(letters, size=50)) for _ in range(args.batches * B)]
        manifests = {}
        for rate in (16000, 48000):
            n = rate * SECONDS
            t = np.arange(n) / rate
            base = [(8000 * np.sin(2 * np.pi * (110.0 + 13 * i) * t) + 5000 * np.sin(2 * np.pi * (700.0 + 31 * i) * t + i)
                     + 1500 * rng.standard_normal(n)).astype(np.int16) for i in range(8)]
            os.mkdir(os.path.join(tmp, str(rate)))
            rows = []
            for i, text in enumerate(texts):
                path = os.path.join(tmp, str(rate), f"u{i:05d}.wav")
                wavfile.write(path, rate, np.roll(base[i % 8], 977 * i))
                rows.append((path, float(SECONDS), rate, text))
            manifests[rate] = os.path.join(tmp, f"manifest{rate}.csv")
            write_manifest(rows, manifests[rate])
        labels = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": (["_", "'"] + letters + ["|"])[:CLASSES]}).to_csv(labels, index=False)
        torch.manual_seed(0)
        model = DeepSpeech(audio_conf=conf(), decoder=None, label_path=labels, rnn_type="gru", rnn_hidden_size=1024, rnn_hidden_layers=5,
                           bidirectional=True)
        model.to(dev).train()
        model.precision = "bf16"
        opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
        tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)

        def loader(rate):
            np.random.seed(1)
            return get_loader(conf(), labels, manifests[rate], batch_size=B, num_workers=args.workers, front_end="gpu", prefetch=2,
                              resample=rate != TARGET)[0]

        def epoch(ld):
            t0, k = None, 0
            for k, data in enumerate(ld, 1):
                tr.step(data)
                if k == args.feed_warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (k - args.feed_warmup)

        resident = next(iter(loader(16000)))

        def floor():
            x, tg, pct, tsz = resident
            for k in range(1, args.batches + 1):
                tr.step((x, tg, pct.clone(), tsz))
                if k == args.feed_warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (args.batches - args.feed_warmup)

        legs = {"floor_resident_ms": floor, "feed_16k_ms": lambda ld=loader(16000): epoch(ld), "feed_48k_resample_ms": lambda ld=loader(48000): epoch(ld)}
        floor()
        times, starved = {k: [] for k in legs}, {k: 0 for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                s0 = DeepSpeechTrainer.starved_steps
                times[k].append(fn())
                starved[k] += DeepSpeechTrainer.starved_steps - s0
        res = dict(feed_batches=args.batches, feed_warmup=args.feed_warmup, workers=args.workers, prefetch=2)
        for k in legs:
            res[k] = round(float(np.mean(times[k])), 3)
            res[k + "_rounds"] = [round(v, 3) for v in times[k]]
            res[k.replace("_ms", "_starved_steps")] = starved[k]
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--feed", action="store_true")
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--feed-warmup", type=int, default=4)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_resample.py measures on the GPU"
    assert 0 <= args.workers <= 8 and args.feed_warmup < args.batches
    dev = torch.device("cuda:0")
    res = dict(batch=B, seconds=SECONDS, iters=args.iters, warmup=args.warmup, rounds=args.rounds)
    res.update(kernel_legs(args, dev))
    if args.feed:
        res.update(feed_legs(args, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
