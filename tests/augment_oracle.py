"""fp64 restatement of the augmented spectrogram front-end's contract (include/ds2hip.h, asr_amd.data.GpuSpectrogramFrontEnd) —
TEST INFRASTRUCTURE ONLY.  Written from the contract, not from asr_amd's code:

  draws   per utterance, in batch order: [noise bank] coin = binomial(1, p); if coin: file = integers(n_files), level = uniform(lo, hi),
          u = random()   [spec_augment] Mf x (f = min(int(uniform(0, F)), bins), f0 = integers(0, bins - f, endpoint=True)),
          Mt x (t = min(int(uniform(0, T)), tau), t0 = integers(0, tau - t, endpoint=True)), tau = 1 + n // hop
  mix     y = x + level * seg * rms(x) / rms(seg), seg[j] = noise[(s + j) mod L], s = floor(u (L - n)) if L >= n else floor(u L);
          rms(seg) == 0: unmixed.  Then the plain spectrogram of y (oracle.stft_oracle.batch_spectrogram), padding of the mixed signal.
  masks   after the (optional) normalisation: rows [f0, f0 + f) and columns [t0, t0 + t) of the utterance's own frames set to 0.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import stft_oracle as S


def reference_inject_noise_sample(data, noise_dst, noise_level):
    """asr_deepspeech/data/noise_injection.py:33-38, literally (the segment is given: the reference cuts it with sox)."""
    data = np.array(data, copy=True)
    assert len(data) == len(noise_dst)
    noise_energy = np.sqrt(noise_dst.dot(noise_dst) / noise_dst.size)
    data_energy = np.sqrt(data.dot(data) / data.size)
    data += noise_level * noise_dst * data_energy / noise_energy
    return data


def start_of(L, n, u):
    return int(math.floor(u * (L - n))) if L >= n else int(math.floor(u * L))


def segment(noise_file, n, u):
    noise_file = np.asarray(noise_file, dtype=np.float64)
    L = len(noise_file)
    return noise_file[(start_of(L, n, u) + np.arange(n)) % L]


def mix(x, noise_file, level, u):
    """fp64 mixed waveform of one utterance."""
    x = np.asarray(x, dtype=np.float64)
    seg = segment(noise_file, len(x), u)
    rn = math.sqrt(seg.dot(seg) / len(x)) if len(x) else 0.0
    if rn == 0.0:
        return x.copy()
    rx = math.sqrt(x.dot(x) / len(x))
    return x + level * seg * rx / rn


def draws(rng, lengths, hop, bins, n_files=0, noise_prob=0.0, levels=(0.0, 0.5), spec_augment=False, F=27, T=70, Mf=1, Mt=1):
    """List of per-utterance dicts: file (None = no noise), level, u, freq [(lo, hi)], time [(lo, hi)]."""
    out = []
    for n in lengths:
        d = dict(file=None, level=0.0, u=0.0, freq=[], time=[])
        if n_files and rng.binomial(1, noise_prob):
            d["file"] = int(rng.integers(n_files))
            d["level"] = float(rng.uniform(*levels))
            d["u"] = float(rng.random())
        if spec_augment:
            tau = 1 + n // hop
            for _ in range(Mf):
                f = min(int(rng.uniform(0.0, F)), bins)
                f0 = int(rng.integers(0, bins - f, endpoint=True))
                d["freq"].append((f0, f0 + f))
            for _ in range(Mt):
                t = min(int(rng.uniform(0.0, T)), tau)
                t0 = int(rng.integers(0, tau - t, endpoint=True))
                d["time"].append((t0, t0 + t))
        out.append(d)
    return out


def apply_masks(spect, frames, freq, time):
    """(B,1,bins,T) in place: per utterance b, rows in freq[b] and columns in time[b] (t < frames[b]) set to 0."""
    for b in range(spect.shape[0]):
        f = frames[b]
        for lo, hi in freq[b]:
            spect[b, 0, lo:hi, :f] = 0.0
        for lo, hi in time[b]:
            spect[b, 0, :, lo:min(hi, f)] = 0.0
    return spect


def augmented_spectrogram(waves, noise_files, levels, us, files, freq, time, n_fft=320, hop=160, window="hamming", pad_mode="constant",
                          normalize=False):
    """fp64 (B,1,bins,T), frames: utterance b mixed with noise_files[files[b]] (files[b] None or level 0 = unmixed), then the plain
    spectrogram, then the masks."""
    mixed = [mix(x, noise_files[f], lv, u) if (f is not None and lv != 0.0) else np.asarray(x, dtype=np.float64)
             for x, f, lv, u in zip(waves, files, levels, us)]
    spect, frames = S.batch_spectrogram(mixed, n_fft, hop, window, pad_mode, normalize)
    return apply_masks(spect, frames, freq, time), frames
