"""Time the reverberation kernel (ds2_reverb_f32, csrc/reverb.h) against an independent yardstick on the same device, and the waveform
feed with and without it.
  kernel legs  B = 64 utterances of 10 s (160000 samples), every row reverberated, one response per row of 256 / 2048 / 4096 / 8000 taps.
               `reverb_<P>`: the C entry point on resident arguments (the metadata is uploaded once), into a preallocated output.
               `fft_<P>`: overlap-add FFT convolution with torch.fft.rfft / irfft on the same batch (blocks of nfft = the power of two >=
               4 P samples), cut to the utterance's length like the kernel.  Before timing, the two are compared on the same inputs.
               Per leg: `--iters` calls between two device events, after `--warmup` calls; the legs are alternated over `--rounds` rounds
               in one process; mean and round-to-round spread (max - min) of the ms per call.  The multiply-adds the truncated convolution
               needs, B * sum_i min(i + 1, P), over the kernel's time give its rate; its share of the 157.3 TFLOP/s fp32 matrix peak
               is that rate over the peak (the kernel is bound by arithmetic: 41 MB in + 41 MB out take 10 us at 8 TB/s).
  --feed       a feed run in the manner of scripts/time_feed.py: ms per iteration of `for data in loader: trainer.step(data)` at the
               metric config c3 with prefetch=2 over `--batches` batches of 64 files of 10 s, plain, once without and once with a
               synthetic bank (ImpulseResponses.synthetic(8), reverb_prob = 0.5), alternated; the floor is the step on a resident batch.
Prints one JSON line.  Usage: python scripts/time_reverb.py [--iters N] [--warmup N] [--rounds N] [--feed] [--batches N] [--workers N]"""
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

B, N = 64, 160000
TAPS = (256, 2048, 4096, 8000)
PEAK_TFLOPS = 157.3


def macs(P):
    """Multiply-adds of the truncated convolution of one batch: B * sum_{i < N} min(i + 1, P)."""
    return B * (P * (P + 1) // 2 + (N - P) * P)


def fft_overlap_add(x, h):
    """x (B, N), h (B, P) -> the first N samples of each row's convolution, by overlap-add in blocks of nfft - P + 1 samples."""
    P = h.size(1)
    nfft = 1 << int(np.ceil(np.log2(4 * P)))
    L = nfft - P + 1
    nb = -(-x.size(1) // L)
    blocks = torch.nn.functional.pad(x, (0, nb * L - x.size(1))).view(x.size(0), nb, L)
    y = torch.fft.irfft(torch.fft.rfft(blocks, nfft) * torch.fft.rfft(h, nfft)[:, None, :], nfft)          # (B, nb, nfft)
    out = y[:, :, :L].reshape(x.size(0), nb * L).clone()
    tail = torch.nn.functional.pad(y[:, :-1, L:], (0, L - (nfft - L)))                                      # P - 1 <= L samples into the next block
    out[:, L:] += tail.reshape(x.size(0), (nb - 1) * L)
    return out[:, :x.size(1)]


def kernel_legs(args, dev):
    from asr_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal((B, N)) * 0.2).astype(np.float32)).to(dev)
    n_dev = torch.full((B,), N, dtype=torch.int32, device=dev)
    out = torch.empty((B, N), dtype=torch.float32, device=dev)
    legs, res = {}, {}
    for P in TAPS:
        h = rng.standard_normal((B, P)) * np.exp(-6.9078 * np.arange(P) / P)
        h = torch.from_numpy((h / np.sqrt((h * h).sum(axis=1, keepdims=True))).astype(np.float32)).to(dev)
        base = (torch.arange(B, dtype=torch.int64, device=dev) * P)
        taps = torch.full((B,), P, dtype=torch.int32, device=dev)

        def run(h=h, base=base, taps=taps):
            _lib.check(lib.ds2_reverb_f32(x.data_ptr(), N, n_dev.data_ptr(), h.data_ptr(), h.numel(), base.data_ptr(), taps.data_ptr(), B, N,
                                          out.data_ptr(), N, torch.cuda.current_stream().cuda_stream), "ds2_reverb_f32")
        legs[f"reverb_{P}_ms"] = run
        legs[f"fft_{P}_ms"] = lambda h=h: fft_overlap_add(x, h)
        run()
        ref = fft_overlap_add(x, h)
        res[f"max_abs_diff_{P}"] = float((out - ref).abs().max())             # two fp32 routes to one result (|y| is about 0.2)
        assert res[f"max_abs_diff_{P}"] < 1e-4, (P, res[f"max_abs_diff_{P}"])
    times = {k: [] for k in legs}
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
    for k in legs:
        res[k] = round(float(np.mean(times[k])), 4)
        res[k + "_rounds"] = [round(v, 4) for v in times[k]]
        res[k.replace("_ms", "_spread_ms")] = round(max(times[k]) - min(times[k]), 4)
    for P in TAPS:
        tflops = 2.0 * macs(P) / (res[f"reverb_{P}_ms"] * 1e-3) / 1e12
        res[f"reverb_{P}_TFLOPs"] = round(tflops, 2)
        res[f"reverb_{P}_share_of_fp32_matrix_peak"] = round(tflops / PEAK_TFLOPS, 3)
        res[f"fft_over_reverb_{P}"] = round(res[f"fft_{P}_ms"] / res[f"reverb_{P}_ms"], 3)
    return res


def feed_legs(args, dev):
    from time_feed import B as FB, conf, write_corpus
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW
    from asr_amd.data import GpuAudioDataLoader, ImpulseResponses, get_loader
    from asr_amd.trainers import DeepSpeechTrainer
    assert FB == B
    with tempfile.TemporaryDirectory() as tmp:
        manifest, labels, _ = write_corpus(tmp, args.batches * B)
        torch.manual_seed(0)
        model = DeepSpeech(audio_conf=conf(), decoder=None, label_path=labels, rnn_type="gru", rnn_hidden_size=1024, rnn_hidden_layers=5,
                           bidirectional=True)
        model.to(dev).train()
        model.precision = "bf16"
        opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
        tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)
        bank = ImpulseResponses.synthetic(8)

        def loader(reverb):
            from asr_amd.data import GpuSpectrogramFrontEnd
            np.random.seed(1)
            ld = get_loader(conf(reverb_prob=0.5), labels, manifest, batch_size=B, num_workers=args.workers, front_end="gpu", prefetch=2)[0]
            if reverb:                                               # the loader's own front-end settings, plus the bank
                fe = GpuSpectrogramFrontEnd(conf(reverb_prob=0.5), normalize=True, augment=True, seed=1, reverb=bank)
                ld = GpuAudioDataLoader(ld.dataset, ld.batch_sampler, args.workers, fe, prefetch=2)
            return ld

        def epoch(ld):
            t0, k = None, 0
            for k, data in enumerate(ld, 1):
                tr.step(data)
                if k == args.feed_warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (k - args.feed_warmup)

        resident = next(iter(loader(False)))

        def floor():
            x, tg, pct, tsz = resident
            for k in range(1, args.batches + 1):
                tr.step((x, tg, pct.clone(), tsz))
                if k == args.feed_warmup:
                    tr.synchronize()
                    t0 = time.perf_counter()
            tr.synchronize()
            return (time.perf_counter() - t0) * 1e3 / (args.batches - args.feed_warmup)

        legs = {"floor_resident_ms": floor, "feed_plain_ms": lambda ld=loader(False): epoch(ld), "feed_reverb_ms": lambda ld=loader(True): epoch(ld)}
        floor()
        times, starved = {k: [] for k in legs}, {k: 0 for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                s0 = DeepSpeechTrainer.starved_steps
                times[k].append(fn())
                starved[k] += DeepSpeechTrainer.starved_steps - s0
        res = dict(feed_batches=args.batches, feed_warmup=args.feed_warmup, workers=args.workers, prefetch=2, reverb_prob=0.5,
                   bank_taps=bank.lengths.tolist())
        for k in legs:
            res[k] = round(float(np.mean(times[k])), 3)
            res[k + "_rounds"] = [round(v, 3) for v in times[k]]
            res[k.replace("_ms", "_starved_steps")] = starved[k]
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--feed", action="store_true")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--feed-warmup", type=int, default=6)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_reverb.py measures on the GPU"
    assert 0 <= args.workers <= 8 and args.feed_warmup < args.batches
    dev = torch.device("cuda:0")
    res = dict(batch=B, samples=N, iters=args.iters, warmup=args.warmup, rounds=args.rounds)
    res.update(kernel_legs(args, dev))
    if args.feed:
        res.update(feed_legs(args, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
