"""Time the tempo / gain perturbation (ds2_tempo_gain_f32) at the metric config's input shape, B = 64 utterances of 10 s (160000 samples on
the 16-bit grid), tempo factors spread over [0.85, 1.15] (K = 125 .. 169 segments), gains over [-6, 8] dB.  Per call it reports:
  - ops.tempo_gain alone on a batch already on the device (both kernels, the host-side sizing and the 1.5 kB parameter upload included);
  - ops.spectrogram_augmented (noise on every utterance, default masks) on the unperturbed batch: the front-end without this feature;
  - ops.tempo_gain followed by ops.spectrogram_augmented on its output: the front-end with it;
  - GpuSpectrogramFrontEnd augmented, without and with the perturbation, from a list of host waveforms (host batching, copies, draws).
Device time is taken with events around `--iters` back-to-back calls, median over `--reps`, the three legs alternated over three rounds
(the middle round is reported).  `--trace` runs a few calls only, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...):
tempo_chain_kernel's time / (Kmax - 1) is the time of one chain step, tempo_synth_kernel moves about 2 x 4 x n bytes per utterance.
Prints one JSON line.  Usage: python scripts/time_tempo.py [--iters N] [--reps N] [--trace]"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_augment import _Bank, _events, _wall          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    from asr_amd import ops
    from asr_amd.data import GpuSpectrogramFrontEnd
    dev = torch.device("cuda:0")
    B, n = 64, 160000
    rng = np.random.default_rng(0)
    t = np.arange(n) / 16000.0
    waves = []
    for i in range(B):
        w = 0.25 * np.sin(2 * np.pi * (110.0 + 13 * i) * t) + 0.15 * np.sin(2 * np.pi * (700.0 + 31 * i) * t + i) + 0.05 * rng.standard_normal(n)
        waves.append((np.rint(w * 32768) / 32768).astype(np.float32))
    tempo = rng.permutation(np.linspace(0.85, 1.15, B))
    gain = np.linspace(-6.0, 8.0, B)
    bank = _Bank([16000 * 60, 16000 * 90, 16000 * 45, 16000 * 105], rng)
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", spec_augment=True, noise_dir=None,
                           noise_prob=1.0, noise_levels=(0.0, 0.5), speed_volume_perturb=True)
    batch = torch.from_numpy(np.stack(waves)).to(dev)
    lens = [n] * B
    n_out = [ops.tempo_out_samples(n, f) for f in tempo]
    S, R, O = ops.tempo_sizes(16000)
    fe_aug = GpuSpectrogramFrontEnd(conf, normalize=True, device=dev, augment=True, seed=0, noise=bank)
    fe_all = GpuSpectrogramFrontEnd(conf, normalize=True, device=dev, augment=True, seed=0, noise=bank, speed_volume_perturb=True)

    def aug_args(lengths):
        p = fe_aug.draw(lengths)
        return dict(noise=bank.device_samples(dev), noise_base=torch.from_numpy(p["base"]).to(dev),
                    noise_period=torch.from_numpy(p["period"]).to(dev), noise_start=torch.from_numpy(p["start"]).to(dev),
                    noise_level=torch.from_numpy(p["level"]).to(dev), freq_masks=torch.from_numpy(p["freq"]).to(dev),
                    time_masks=torch.from_numpy(p["time"]).to(dev))
    kw0, kw1 = aug_args(lens), aug_args(n_out)
    lens_t, n_out_t = torch.tensor(lens, dtype=torch.int32), torch.tensor(n_out, dtype=torch.int32)
    tempo_only = lambda: ops.tempo_gain(batch, lens, tempo, gain, 16000)                                           # noqa: E731
    aug_only = lambda: ops.spectrogram_augmented(batch, lens_t, 320, 160, "hamming", "constant", True, **kw0)       # noqa: E731

    def both():
        y, _, _ = ops.tempo_gain(batch, lens, tempo, gain, 16000)
        return ops.spectrogram_augmented(y, n_out_t, 320, 160, "hamming", "constant", True, **kw1)
    y, n_dev, offsets = tempo_only()
    x, _ = both()
    assert n_dev.tolist() == n_out and bool(torch.isfinite(x).all()) and x.size(3) == 1 + max(n_out) // 160
    res = dict(batch=B, samples=n, S=S, R=R, O=O, segments_min=-(-min(n_out) // (S - O)), segments_max=int(offsets.size(1)),
               iters=args.iters, reps=args.reps)
    if args.trace:
        for _ in range(5):
            tempo_only()
        torch.cuda.synchronize()
        res["trace_calls_of_tempo_gain"] = 7                       # two above (one inside both()), five here
        print(json.dumps(res))
        return
    legs = {"tempo_gain_ms": tempo_only, "spectrogram_augmented_ms": aug_only, "tempo_gain_plus_spectrogram_augmented_ms": both}
    times = {k: [] for k in legs}
    for _ in range(3):                                              # alternate so that drift on a shared host hits all legs
        for k, fn in legs.items():
            times[k].append(_events(fn, args.iters, args.reps))
    for k in legs:
        res[k] = round(sorted(times[k])[1], 4)
        res[k + "_rounds"] = [round(v, 4) for v in times[k]]
    res["perturbation_overhead_ms"] = round(res["tempo_gain_plus_spectrogram_augmented_ms"] - res["spectrogram_augmented_ms"], 4)
    res["synth_bytes_mb"] = round(4 * (B * n + sum(n_out)) / 1e6, 1)       # one read of the input, one write of the output
    res["front_end_augmented_ms"] = round(_wall(lambda: fe_aug(waves), args.reps), 3)
    res["front_end_augmented_perturbed_ms"] = round(_wall(lambda: fe_all(waves), args.reps), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
