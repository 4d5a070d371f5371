"""Time the GPU spectrogram front-end with and without augmentation at the metric config's input shape, B = 64 utterances of 10 s
(160000 samples, 1001 frames), normalised, with a synthetic noise bank of five minutes.  Per call it reports:
  - ops.spectrogram (ds2_spectrogram_f32) on a batch already on the device;
  - ops.spectrogram_augmented (ds2_spectrogram_aug_f32) on the same batch, noise on every utterance and the default masks
    (one frequency mask of up to 27 bins, one time mask of up to 70 frames), per-utterance parameters already on the device;
  - GpuSpectrogramFrontEnd, plain and augmented, from a list of host waveforms (host batching, copies and draws included).
Device time is taken with events around `--iters` back-to-back calls, median over `--reps`.  Prints one JSON line.
Usage: python scripts/time_augment.py [--iters N] [--reps N]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ms.sort()
    return ms[len(ms) // 2]


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return ms[len(ms) // 2]


class _Bank:
    """Stands in for asr_amd.data.NoiseInjection (no files needed): the same attributes GpuSpectrogramFrontEnd reads."""

    def __init__(self, lengths, rng):
        self.lengths = np.array(lengths, np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.samples = (rng.standard_normal(int(self.lengths.sum())) * 0.1).astype(np.float32)
        self.noise_levels = (0.0, 0.5)
        self._dev = {}

    def __len__(self):
        return len(self.lengths)

    def device_samples(self, device):
        if str(device) not in self._dev:
            self._dev[str(device)] = torch.from_numpy(self.samples).to(device)
        return self._dev[str(device)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from asr_amd import ops
    from asr_amd.data import GpuSpectrogramFrontEnd
    dev = torch.device("cuda:0")
    B, n = 64, 160000
    rng = np.random.default_rng(0)
    waves = [(rng.standard_normal(n) * 0.3).astype(np.float32) for _ in range(B)]
    bank = _Bank([16000 * 60, 16000 * 90, 16000 * 45, 16000 * 105], rng)      # five minutes in four files
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", spec_augment=True, noise_dir=None,
                           noise_prob=1.0, noise_levels=(0.0, 0.5))
    batch = torch.from_numpy(np.stack(waves)).to(dev)
    lens = torch.full((B,), n, dtype=torch.int32)
    fe_aug = GpuSpectrogramFrontEnd(conf, normalize=True, device=dev, augment=True, seed=0, noise=bank)
    fe_plain = GpuSpectrogramFrontEnd(conf, normalize=True, device=dev)
    p = fe_aug.draw([n] * B)
    assert (p["level"] > 0).all()
    kw = dict(noise=bank.device_samples(dev), noise_base=torch.from_numpy(p["base"]).to(dev),
              noise_period=torch.from_numpy(p["period"]).to(dev), noise_start=torch.from_numpy(p["start"]).to(dev),
              noise_level=torch.from_numpy(p["level"]).to(dev), freq_masks=torch.from_numpy(p["freq"]).to(dev),
              time_masks=torch.from_numpy(p["time"]).to(dev))
    plain = lambda: ops.spectrogram(batch, lens, 320, 160, "hamming", "constant", True)                     # noqa: E731
    aug = lambda: ops.spectrogram_augmented(batch, lens, 320, 160, "hamming", "constant", True, **kw)        # noqa: E731
    x, _ = aug()
    assert x.shape == (B, 1, 161, 1001) and bool(torch.isfinite(x).all())
    res = dict(batch=B, samples=n, frames=int(x.size(3)), noise_bank_samples=int(len(bank.samples)), iters=args.iters, reps=args.reps)
    # alternate the two so that drift on a shared host hits both
    t = {"plain": [], "aug": []}
    for _ in range(3):
        t["plain"].append(_events(plain, args.iters, args.reps))
        t["aug"].append(_events(aug, args.iters, args.reps))
    res["spectrogram_ms"] = round(sorted(t["plain"])[1], 4)
    res["spectrogram_augmented_ms"] = round(sorted(t["aug"])[1], 4)
    res["augment_overhead_ms"] = round(res["spectrogram_augmented_ms"] - res["spectrogram_ms"], 4)
    res["extra_bytes_mb"] = round(2 * B * n * 4 / 1e6, 1)      # one more read of the audio and of the noise segments (energy pass)
    res["front_end_plain_ms"] = round(_wall(lambda: fe_plain(waves), args.reps), 3)
    res["front_end_augmented_ms"] = round(_wall(lambda: fe_aug(waves), args.reps), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
