"""Time the waveform feed in front of the train step: how long an iteration of `for data in loader: trainer.step(data)` takes with the
synchronous GPU-front-end loader (prefetch=0) and with the pipelined feed (prefetch=2), against the step alone on a resident batch.
  dataset   `--batches` x 64 synthetic 16-bit mono WAV files of 10 s (160000 samples) in a temporary directory, 50-character transcripts;
  model     the metric config c3 (5 x 1024 BiGRU, 29 classes) in bf16 with FusedAdamW, as bench.py builds it;
  legs      floor: trainer.step on ONE resident batch of the plain loader (what bench.py times);
            sync / feed: a whole epoch through get_loader(front_end="gpu", prefetch=0 / 2), `--workers` workers (at most 8), with plain
            settings and with noise on every utterance + SpecAugment + perturb=True.
Per leg: wall time from the end of the `--warmup`-th iteration (after a trainer.synchronize()) to a final trainer.synchronize(), divided
by the iterations in between.  The five legs are alternated over `--rounds` rounds in one process; per leg the mean over the rounds, the
round-to-round spread (max - min) and the DeepSpeechTrainer.starved_steps it added are reported.  `--trace` runs one short pipelined
epoch only, for a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/time_feed.py --trace).
Prints one JSON line.  Usage: python scripts/time_feed.py [--batches N] [--warmup N] [--rounds N] [--workers N] [--trace]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, SR, CLASSES = 64, 160000, 16000, 29


def write_corpus(tmp, n_files):
    import pandas as pd
    from scipy.io import wavfile
    from asr_amd.data import write_manifest
    rng = np.random.default_rng(0)
    t = np.arange(N) / SR
    base = [(8000 * np.sin(2 * np.pi * (110.0 + 13 * i) * t) + 5000 * np.sin(2 * np.pi * (700.0 + 31 * i) * t + i) + 1500 * rng.standard_normal(N))
            for i in range(16)]
    letters = list("abcdefghijklmnopqrstuvwxyz")
    rows = []
    for i in range(n_files):
        path = os.path.join(tmp, f"u{i:05d}.wav")
        wavfile.write(path, SR, np.roll(base[i % 16], 977 * i).astype(np.int16))
        rows.append((path, N / SR, SR, "".join(rng.choice(letters, size=50))))
    write_manifest(rows, os.path.join(tmp, "manifest.csv"))
    chars = ["_", "'"] + letters + ["|"]
    pd.DataFrame({"label": chars[:CLASSES]}).to_csv(os.path.join(tmp, "labels.csv"), index=False)
    os.mkdir(os.path.join(tmp, "noise"))
    for i, seconds in enumerate((60, 90, 45)):
        wavfile.write(os.path.join(tmp, "noise", f"n{i}.wav"), SR, (rng.standard_normal(SR * seconds) * 4000).astype(np.int16))
    return os.path.join(tmp, "manifest.csv"), os.path.join(tmp, "labels.csv"), os.path.join(tmp, "noise")


def conf(**kw):
    c = dict(sample_rate=SR, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert args.batches >= 30 or args.trace, "at least 30 batches of 64"
    assert 0 <= args.workers <= 8 and args.warmup < args.batches
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW
    from asr_amd.data import get_loader
    from asr_amd.trainers import DeepSpeechTrainer
    assert torch.cuda.is_available(), "time_feed.py measures on the GPU"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        manifest, labels, noise_dir = write_corpus(tmp, (8 if args.trace else args.batches) * B)
        torch.manual_seed(0)
        model = DeepSpeech(audio_conf=conf(), decoder=None, label_path=labels, rnn_type="gru", rnn_hidden_size=1024, rnn_hidden_layers=5,
                           bidirectional=True)
        model.to(dev).train()
        model.precision = "bf16"
        opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
        tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)
        plain = conf()
        full = conf(noise_dir=noise_dir, noise_prob=1.0, noise_levels=(0.1, 0.5), spec_augment=True, speed_volume_perturb=True)

        def loader(c, perturb, prefetch):
            np.random.seed(1)
            return get_loader(c, labels, manifest, batch_size=B, num_workers=args.workers, front_end="gpu", perturb=perturb, prefetch=prefetch)[0]

        def epoch(ld, warmup):
            """ms per iteration after the warm-up iterations"""
            t0, k = None, 0
            for k, data in enumerate(ld, 1):
                tr.step(data)
                if k == warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (k - warmup)

        if args.trace:
            ms = epoch(loader(full, True, 2), 2)
            print(json.dumps({"trace": True, "batches": 8, "calls_of_wave_unpack": 8, "feed_augmented_ms": round(ms, 3)}))
            return
        resident = next(iter(loader(plain, False, 0)))
        assert tuple(resident[0].shape) == (B, 1, 161, 1 + N // 160)

        def floor():
            x, tg, pct, tsz = resident
            n = args.batches
            for k in range(1, n + 1):
                tr.step((x, tg, pct.clone(), tsz))
                if k == args.warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (n - args.warmup)

        legs = {"floor_resident_ms": floor,
                "sync_plain_ms": lambda ld=loader(plain, False, 0): epoch(ld, args.warmup),
                "feed_plain_ms": lambda ld=loader(plain, False, 2): epoch(ld, args.warmup),
                "sync_augmented_ms": lambda ld=loader(full, True, 0): epoch(ld, args.warmup),
                "feed_augmented_ms": lambda ld=loader(full, True, 2): epoch(ld, args.warmup)}
        floor()                                                          # code objects, workspaces, the persistent kernels' first launch
        times, starved = {k: [] for k in legs}, {k: 0 for k in legs}
        for _ in range(args.rounds):                                     # alternate so that drift on a shared host hits all legs
            for k, fn in legs.items():
                s0 = DeepSpeechTrainer.starved_steps
                times[k].append(fn())
                starved[k] += DeepSpeechTrainer.starved_steps - s0
        res = dict(batch=B, samples=N, batches=args.batches, warmup=args.warmup, rounds=args.rounds, workers=args.workers, prefetch=2)
        for k in legs:
            res[k] = round(float(np.mean(times[k])), 3)
            res[k + "_rounds"] = [round(v, 3) for v in times[k]]
            res[k.replace("_ms", "_spread_ms")] = round(max(times[k]) - min(times[k]), 3)
            res[k.replace("_ms", "_starved_steps")] = starved[k]
        for kind in ("plain", "augmented"):
            res[f"feed_minus_floor_{kind}_ms"] = round(res[f"feed_{kind}_ms"] - res["floor_resident_ms"], 3)
            res[f"sync_minus_floor_{kind}_ms"] = round(res[f"sync_{kind}_ms"] - res["floor_resident_ms"], 3)
            res[f"sync_minus_feed_{kind}_ms"] = round(res[f"sync_{kind}_ms"] - res[f"feed_{kind}_ms"], 3)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
