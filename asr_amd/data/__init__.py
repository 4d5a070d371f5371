"""Data-side API surface kept by name: SpectrogramDataset, BucketingSampler,
DistributedBucketingSampler, AudioDataLoader, get_loader; plus the true length-bucketing samplers of SURVEY §8(f)4
(LengthBucketingSampler, DistributedLengthBucketingSampler).  Host-side / I-O bound; not accelerated.

`SpectrogramDataset` reads the reference's manifest CSV (`audio_filepath`, `text`).  Audio decoding:
pre-computed spectrograms (`.npy` / `.pt`, shape (161, T)) are loaded as-is; `.wav` files go through a
numpy STFT restatement of data/parsers/spectrogram_parser.py:36-62 (n_fft = win = sr*window_size,
hop = sr*window_stride, centred zero-padded frames, log1p magnitude, per-utterance mean/std).
`GpuSpectrogramFrontEnd` does the same for a whole batch on the GPU (csrc/stft.hip), optionally with noise injection
(`NoiseInjection`) and SpecAugment; `get_loader(..., front_end="gpu")` feeds it from workers that only read WAV files.
Parity with librosa 0.11.0 itself is UNPINNED (librosa is not installable here); both are held to
oracle/stft_oracle.py, which is cross-checked against torch.stft and scipy.signal.stft.
"""
from __future__ import annotations

import math
import os
import warnings

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.sampler import Sampler

from ..functional import _collate_fn
from ..ops import WAVE_ALIGN, WAVE_MAX_ELEMS      # the packed layout: offsets are multiples of WAVE_ALIGN elements and fit the device's int32


def _stft_spectrogram(y: np.ndarray, sample_rate: int, window_size: float, window_stride: float, window: str = "hamming",
                      pad_mode: str = "constant"):
    """Host (numpy) restatement used by the per-item dataset path, like the reference's CPU librosa call.  Zero padding is
    librosa's default since 0.10 (the reference pins 0.11.0); pass pad_mode="reflect" for the pre-0.10 behaviour."""
    from scipy.signal import get_window
    n_fft = int(sample_rate * window_size)
    hop = int(sample_rate * window_stride)
    win = get_window(window, n_fft, fftbins=True).astype(np.float32)
    y = np.pad(y.astype(np.float32), n_fft // 2, mode=pad_mode)
    n_frames = 1 + (len(y) - n_fft) // hop
    frames = np.lib.stride_tricks.as_strided(y, shape=(n_frames, n_fft), strides=(y.strides[0] * hop, y.strides[0]))
    spect = np.abs(np.fft.rfft(frames * win, axis=1)).T.astype(np.float32)  # (n_fft/2+1, frames)
    return np.log1p(spect)


def _mono_float32(y):
    """wavfile.read's samples -> mono float32, scaled like soundfile (audio/functional.py:11): integer PCM / 2^(bits-1), 8-bit unsigned PCM
    centred on 128; channels averaged."""
    if y.dtype.kind == "i":
        y = y.astype(np.float32) / float(2 ** (8 * y.dtype.itemsize - 1))
    elif y.dtype.kind == "u":
        y = (y.astype(np.float32) - 128.0) / 128.0
    if y.ndim > 1:
        y = y.mean(axis=1)
    return y.astype(np.float32, copy=False)


def _read_wav(path):
    """(sample_rate, mono float32 waveform) of a WAV file, scaled like soundfile (audio/functional.py:11): integer PCM / 2^(bits-1),
    8-bit unsigned PCM centred on 128; channels averaged."""
    from scipy.io import wavfile
    sr, y = wavfile.read(path)
    return sr, _mono_float32(y)


def _read_wav_raw(path):
    """(sample_rate, samples) for the packed feed: the int16 samples themselves when the file is 16-bit mono PCM (the GPU scales them by
    2^-15, which is exact), else `_read_wav`'s float32 waveform (8 / 24 / 32-bit, float and multi-channel files)."""
    from scipy.io import wavfile
    sr, y = wavfile.read(path)
    if y.dtype == np.int16 and y.ndim == 1:
        return sr, y
    return sr, _mono_float32(y)


def resample_waveform(y, fs, ft):
    """Host sample-rate conversion, fs -> ft Hz: the sum of the ds2_wave_resample_f32 contract (include/ds2hip.h) — the same fp32 table
    (ops.resample_taps), y[m] = sum_j tab[p][j] x[i0 - J + 1 + j] with i0 = (m M) div L, p = (m M) mod L, x = 0 outside the utterance —
    in vectorised numpy fp64, rounded to fp32 once; ceil(n L / M) samples.  fs == ft returns the input's float32 samples bit for bit.
    ValueError for an unsupported rate pair (ops.resample_ratio).  Used where there is no GPU batch: the noise bank and the host front-end."""
    from .. import ops
    y = np.ascontiguousarray(y, dtype=np.float32)
    if y.ndim != 1:
        raise ValueError(f"resample_waveform: expected a 1-D waveform, got shape {y.shape}")
    L, M, J = ops.resample_ratio(fs, ft)
    if L == 1 and M == 1:
        return y
    tab = ops.resample_taps(fs, ft).astype(np.float64)
    n, P = len(y), 2 * J
    n_out = -(-n * L // M)
    x = np.concatenate([np.zeros(P, np.float64), y.astype(np.float64), np.zeros(P + 1, np.float64)])      # x[i] is at i + P
    out = np.empty(n_out, dtype=np.float32)
    j = np.arange(P, dtype=np.int64)[None, :]
    for lo in range(0, n_out, 16384):
        t = np.arange(lo, min(lo + 16384, n_out), dtype=np.int64) * M
        i0, p = t // L, t % L                           # i0 - J + 1 >= -J + 1 and i0 + J <= n - 1 + J: inside the padding
        out[lo:lo + len(t)] = (tab[p] * x[(i0 - J + 1 + P)[:, None] + j]).sum(axis=1)
    return out


def noise_levels_of(audio_conf):
    """(lo, hi) noise level range: audio_conf.noise_levels, else (noise_min, noise_max) — the keys of the reference's config.yml, on which
    the reference's own NoiseInjection(audio_conf.noise_levels) would fail — else the reference's default (0, 0.5)."""
    lv = getattr(audio_conf, "noise_levels", None)
    if lv is not None:
        lo, hi = lv
    elif getattr(audio_conf, "noise_min", None) is not None or getattr(audio_conf, "noise_max", None) is not None:
        lo, hi = getattr(audio_conf, "noise_min", 0.0), getattr(audio_conf, "noise_max", 0.5)
    else:
        lo, hi = 0.0, 0.5
    return float(lo), float(hi)


def noise_start(period: int, n: int, u: float) -> int:
    """First noise sample of an utterance of n samples: floor(u * (L - n)) when the file is at least as long, else floor(u * L) (the segment
    then wraps around the file: this port's choice — the reference fails on noise shorter than the utterance)."""
    return int(math.floor(u * (period - n))) if period >= n else int(math.floor(u * period))


_AUDIO_EXTS = ("aac", "au", "flac", "m4a", "mp3", "ogg", "wav")     # librosa.util.find_files' default extensions


class NoiseInjection:
    """The reference's NoiseInjection (asr_deepspeech/data/noise_injection.py:9-38) as ONE noise bank: every `.wav` under `path` (recursively,
    sorted, as librosa.util.find_files lists them) is read once with the scaling of SpectrogramDataset.parse_audio and the files are kept
    concatenated — `samples` (fp32, host) plus `starts` / `lengths` per file; `device_samples(device)` is the same bank in one device buffer
    (uploaded once per device) for GpuSpectrogramFrontEnd.  Other audio formats are skipped with a warning (no sox here: no decoding, no
    resampling); files must be at `sample_rate`, unless `resample=True`: an off-rate file is then converted once, here, on the host
    (`resample_waveform`), so the bank, `starts` and `lengths` are at `sample_rate` and nothing downstream changes.

    `inject_noise(data)` keeps the reference's host method and its draws from numpy's global state (file, level ~ U(noise_levels), u ~ U[0,1));
    the mix is `data + level * seg * rms(data) / rms(seg)` with seg = noise[(s + j) mod L], s = noise_start(L, n, u); a silent segment leaves
    the data unmixed (the reference divides by zero there)."""

    def __init__(self, path=None, sample_rate=16000, noise_levels=(0, 0.5), resample=False):
        if path is None or not os.path.exists(path):
            print("Directory doesn't exist: {}".format(path))
            raise IOError(f"noise directory does not exist: {path}")
        found = []
        for root, _dirs, files in os.walk(path):
            for f in files:
                if f.rsplit(".", 1)[-1].lower() in _AUDIO_EXTS and "." in f:
                    found.append(os.path.abspath(os.path.join(root, f)))
        found.sort()
        skipped = [f for f in found if not f.lower().endswith(".wav")]
        if skipped:
            warnings.warn(f"asr_amd.data.NoiseInjection: {len(skipped)} non-WAV noise file(s) skipped (no decoder / resampler here), e.g. {skipped[0]}")
        self.paths = [f for f in found if f.lower().endswith(".wav")]
        if not self.paths:
            raise ValueError(f"NoiseInjection: no .wav file under {path}")
        self.sample_rate, self.noise_levels = int(sample_rate), tuple(float(v) for v in noise_levels)
        waves = []
        for f in self.paths:
            sr, y = _read_wav(f)
            if sr != self.sample_rate:
                if not resample:
                    raise ValueError(f"NoiseInjection: {f} is sampled at {sr} Hz, expected {self.sample_rate} Hz (no resampling here)")
                y = resample_waveform(y, sr, self.sample_rate)   # once per off-rate file: the bank is at the target rate
            if len(y) == 0:
                raise ValueError(f"NoiseInjection: {f} holds no samples")
            waves.append(y)
        self.lengths = np.array([len(y) for y in waves], dtype=np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.samples = np.concatenate(waves).astype(np.float32)
        self._device = {}

    def __len__(self):
        return len(self.paths)

    def device_samples(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.samples).to(device)
        return self._device[key]

    def segment(self, index: int, n: int, u: float) -> np.ndarray:
        """The n noise samples file `index` contributes to an utterance of n samples for draw u."""
        L, b = int(self.lengths[index]), int(self.starts[index])
        return self.samples[b + (noise_start(L, n, u) + np.arange(n)) % L]

    def inject_noise(self, data):
        index = np.random.choice(len(self.paths))
        noise_level = np.random.uniform(*self.noise_levels)
        return self.inject_noise_sample(data, index, noise_level, np.random.rand())

    def inject_noise_sample(self, data, index, noise_level, u):
        seg = self.segment(index, len(data), u).astype(np.float64)
        x = np.asarray(data, dtype=np.float64)
        noise_energy = np.sqrt(seg.dot(seg) / seg.size)
        data_energy = np.sqrt(x.dot(x) / x.size)
        if noise_energy == 0.0:
            return np.asarray(data)
        return (x + noise_level * seg * data_energy / noise_energy).astype(np.asarray(data).dtype)


class ImpulseResponses:
    """A bank of room impulse responses (RIRs) for reverberation, modelled on NoiseInjection: every `.wav` under `path` (recursively,
    sorted) is read once and the prepared responses are kept concatenated — `taps` (fp32, host) plus `starts` / `lengths` per file;
    `device_taps(device)` is the same bank in one device buffer (uploaded once per device) for ops.reverb.  Of a multi-channel file
    CHANNEL 0 is taken (averaging the channels of an RIR would smear it).  Files must be at `sample_rate`, unless `resample=True`: an
    off-rate file is then converted once, here, on the host (`resample_waveform`).

    Preparation of one response, in fp64 on the host (`prepare`; tests/reverb_oracle.py restates it):
      1. d = argmax |h|, the lowest index on ties; h[d:] is kept, so the direct path sits at lag 0 and a reverberated utterance is not
         shifted in time.  THE SAMPLES BEFORE THE PEAK ARE DROPPED.
      2. the length P is the smallest P >= 1 with sum_{k >= P} h[k]^2 <= 10^(tail_db / 10) * sum h^2, capped at
         int(max_seconds * sample_rate) and at ops.reverb_max_taps() (16384): a longer response is truncated.
      3. h /= sqrt(sum h^2): unit energy.  This is the level convention here: the loader's spectrograms are normalised per utterance and
         the noise is mixed relative to the rms of the reverberated signal, so no device-side level pass is needed.
      4. rounded to fp32.
    A file that is all zeros (or empty) raises."""

    def __init__(self, path, sample_rate=16000, max_seconds=0.5, tail_db=-60.0, resample=False):
        if path is None or not os.path.exists(path):
            raise IOError(f"impulse-response directory does not exist: {path}")
        found = []
        for root, _dirs, files in os.walk(path):
            for f in files:
                if f.lower().endswith(".wav"):
                    found.append(os.path.abspath(os.path.join(root, f)))
        found.sort()
        if not found:
            raise ValueError(f"ImpulseResponses: no .wav file under {path}")
        from scipy.io import wavfile
        responses = []
        for f in found:
            sr, y = wavfile.read(f)
            y = _mono_float32(y[:, 0] if y.ndim > 1 else y)
            if sr != int(sample_rate):
                if not resample:
                    raise ValueError(f"ImpulseResponses: {f} is sampled at {sr} Hz, expected {int(sample_rate)} Hz (pass resample=True)")
                y = resample_waveform(y, sr, int(sample_rate))
            try:
                responses.append(self.prepare(y, sample_rate, max_seconds, tail_db))
            except ValueError as e:
                raise ValueError(f"ImpulseResponses: {f}: {e}") from None
        self._set(responses, found, sample_rate, max_seconds, tail_db)

    def _set(self, responses, paths, sample_rate, max_seconds, tail_db):
        self.paths = list(paths)
        self.sample_rate, self.max_seconds, self.tail_db = int(sample_rate), float(max_seconds), float(tail_db)
        self.lengths = np.array([len(h) for h in responses], dtype=np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.taps = np.concatenate(responses).astype(np.float32)
        self._device = {}

    @staticmethod
    def prepare(h, sample_rate=16000, max_seconds=0.5, tail_db=-60.0):
        """Steps 1 to 4 of the class docstring on one raw response: the prepared fp32 taps."""
        from .. import ops
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size == 0 or not np.any(h):
            raise ValueError("an impulse response must hold a non-zero sample")
        h = h[int(np.argmax(np.abs(h))):]
        e = h * h
        tail = np.concatenate([np.cumsum(e[::-1])[::-1][1:], [0.0]])         # tail[P - 1] = sum_{k >= P} h[k]^2
        P = int(np.argmax(tail <= 10.0 ** (tail_db / 10.0) * e.sum())) + 1
        P = max(1, min(P, int(max_seconds * sample_rate), ops.reverb_max_taps()))
        h = h[:P]
        return (h / np.sqrt((h * h).sum())).astype(np.float32)

    @classmethod
    def synthetic(cls, count, sample_rate=16000, t60_range=(0.2, 0.8), drr_db_range=(-2.0, 12.0), seed=0, **kw):
        """`count` synthetic responses, for users without an RIR corpus and for the tests: h[0] = 1 (the direct path) and, for k >= 1,
        h[k] = g N(0, 1) exp(-6.9078 k / (T60 sample_rate)) — exponentially decaying Gaussian noise, 60 dB down after T60 seconds — with g
        set so that the direct-to-reverberant energy ratio equals the drawn DRR; 2 T60 seconds are synthesised.  Per response, from ONE
        np.random.default_rng(seed): T60 ~ U(*t60_range), then DRR ~ U(*drr_db_range) dB, then the Gaussian block.  The result goes through
        `prepare` (`max_seconds`, `tail_db` in **kw).  A CRUDE MODEL — no early reflections, no room geometry; whether training on it helps
        far-field WER is UNMEASURED."""
        rng = np.random.default_rng(seed)
        max_seconds, tail_db = float(kw.pop("max_seconds", 0.5)), float(kw.pop("tail_db", -60.0))
        if kw:
            raise TypeError(f"ImpulseResponses.synthetic: unexpected arguments {sorted(kw)}")
        responses = []
        for _ in range(int(count)):
            t60 = rng.uniform(*t60_range)
            drr_db = rng.uniform(*drr_db_range)
            n = max(int(2.0 * t60 * sample_rate), 2)
            tail = rng.standard_normal(n - 1) * np.exp(-6.9078 * np.arange(1, n, dtype=np.float64) / (t60 * sample_rate))
            g = np.sqrt(10.0 ** (-drr_db / 10.0) / (tail * tail).sum())
            responses.append(cls.prepare(np.concatenate([[1.0], g * tail]), sample_rate, max_seconds, tail_db))
        self = cls.__new__(cls)
        self._set(responses, [f"synthetic:{seed}:{i}" for i in range(int(count))], sample_rate, max_seconds, tail_db)
        return self

    def __len__(self):
        return len(self.paths)

    def device_taps(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.taps).to(device)
        return self._device[key]


def draw_reverb(rng, B, bank, prob):
    """Which impulse response each utterance of one batch gets, drawn from `rng` (numpy Generator) on the host: per utterance in batch
    order, coin = rng.binomial(1, prob); if coin: file = rng.integers(len(bank)).  One block, drawn AFTER draw_perturbation's and BEFORE
    draw_augmentation's for the same batch.  Returns (file (B,) int64, -1 = not reverberated; base (B,) int64; taps (B,) int32): the
    arguments of ops.reverb."""
    file, base, taps = np.full(B, -1, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int32)
    for b in range(B):
        if rng.binomial(1, prob):
            i = int(rng.integers(len(bank)))
            file[b], base[b], taps[b] = i, int(bank.starts[i]), int(bank.lengths[i])
    return file, base, taps


def draw_perturbation(rng, B, tempo_range=(0.85, 1.15), gain_range=(-6, 8)):
    """Tempo factors and gains (dB) of one batch, drawn from `rng` (numpy Generator) on the host: per utterance, in the order given,
    tempo = rng.uniform(*tempo_range) then gain = rng.uniform(*gain_range) (load_randomly_augmented_audio's ranges, audio/functional.py:94-104).
    One block of 2 B numbers, drawn BEFORE draw_augmentation's for the same batch.  Returns (tempo (B,) float64, gain (B,) float64)."""
    tempo, gain = np.zeros(B, np.float64), np.zeros(B, np.float64)
    for b in range(B):
        tempo[b] = rng.uniform(*tempo_range)
        gain[b] = rng.uniform(*gain_range)
    return tempo, gain


def draw_augmentation(rng, n_samples, hop, n_bins, noise=None, noise_prob=0.0, spec_augment=False, freq_mask_param=27, time_mask_param=70,
                      freq_masks=1, time_masks=1):
    """Per-utterance augmentation parameters of one batch, drawn from `rng` (numpy Generator) on the host.  Order, per utterance in batch
    order (after the batch is sorted by frame count):
      with a noise bank:  coin = rng.binomial(1, noise_prob); if coin: file = rng.integers(len(bank)), level = rng.uniform(*levels),
                          u = rng.random()
      with spec_augment:  freq_masks x (f = min(int(rng.uniform(0, F)), n_bins), f0 = rng.integers(0, n_bins - f, endpoint=True)),
                          then time_masks x (t = min(int(rng.uniform(0, T_param)), tau), t0 = rng.integers(0, tau - t, endpoint=True)),
                          tau = the utterance's own frame count 1 + n // hop.
    Returns a dict of numpy arrays: file (-1 = no noise), level, u, base, period, start, freq (B, Mf, 2), time (B, Mt, 2) [lo, hi) ranges."""
    B = len(n_samples)
    p = dict(file=np.full(B, -1, np.int64), level=np.zeros(B, np.float32), u=np.zeros(B), base=np.zeros(B, np.int64),
             period=np.ones(B, np.int32), start=np.zeros(B, np.int32), freq=np.zeros((B, freq_masks if spec_augment else 0, 2), np.int32),
             time=np.zeros((B, time_masks if spec_augment else 0, 2), np.int32))
    for b, n in enumerate(int(v) for v in n_samples):
        if noise is not None and rng.binomial(1, noise_prob):
            i = int(rng.integers(len(noise)))
            level = rng.uniform(*noise.noise_levels)
            u = rng.random()
            L = int(noise.lengths[i])
            p["file"][b], p["level"][b], p["u"][b] = i, level, u
            p["base"][b], p["period"][b], p["start"][b] = int(noise.starts[i]), L, noise_start(L, n, u)
        if spec_augment:
            tau = 1 + n // hop if n > 0 else 0
            for m in range(freq_masks):
                f = min(int(rng.uniform(0.0, freq_mask_param)), n_bins)
                f0 = int(rng.integers(0, n_bins - f, endpoint=True))
                p["freq"][b, m] = (f0, f0 + f)
            for m in range(time_masks):
                t = min(int(rng.uniform(0.0, time_mask_param)), tau)
                t0 = int(rng.integers(0, tau - t, endpoint=True))
                p["time"][b, m] = (t0, t0 + t)
    return p


class GpuSpectrogramFrontEnd:
    """Batch spectrogram front-end on the GPU (csrc/stft.hip, `ds2_spectrogram_f32`): a list of 1-D waveforms in, the
    `_collate_fn` contract out — `(inputs (B,1,161,T) on the GPU, input_percentages (B,) float32)` — i.e. what
    SpectrogramParser.parse_audio (spectrogram_parser.py:36-62) + _collate_fn (functional.py:9-32) produce per batch, with
    the STFT, log1p, per-utterance mean/std and zero padding done in four kernels instead of per item in DataLoader workers.

    `augment=True` (ds2_spectrogram_aug_f32) honours the augmentations audio_conf asks for:
      * noise injection when `audio_conf.noise_dir` is set: with probability `noise_prob` an utterance is mixed with a segment of a noise
        file before the STFT, y = x + level * seg * rms(x) / rms(seg) (NoiseInjection; levels from noise_levels or noise_min / noise_max);
      * SpecAugment when `audio_conf.spec_augment`: `freq_masks` frequency masks of up to `freq_mask_param` bins and `time_masks` time
        masks of up to `time_mask_param` frames of the utterance's own length, set to 0 after the normalisation (upstream deepspeech.pytorch's
        spec_augment without time warp; time warp is not implemented).  Padding frames stay 0.
      * tempo / gain perturbation when `audio_conf.speed_volume_perturb` AND `speed_volume_perturb=True` here: every utterance is
        time-stretched by tempo ~ U(*tempo_range) (WSOLA, pitch kept) and scaled by gain ~ U(*gain_range) dB, clipped to [-1, 1], first of
        all (ops.tempo_gain, ds2_tempo_gain_f32) — noise and masks then follow the perturbed utterance of floor(n / tempo + 0.5) samples.
        Modelled on sox's `tempo` / `gain` effects that the reference runs per file; parity with sox is unpinned, and its 16-bit
        requantisation with dither is not reproduced.  Its draws (draw_perturbation) come as one block before draw_augmentation's.
      * reverberation when a bank of room impulse responses is given (`reverb=`, an ImpulseResponses, or `audio_conf.rir_dir`, from which
        one is built): with probability `audio_conf.reverb_prob` (default 0.5: a starting point — which value serves real recordings is
        UNMEASURED) an utterance is convolved with a response of the bank (ops.reverb, ds2_reverb_f32), cut to its own length, after
        tempo / gain and before the noise: the noise is then scaled by the rms of the REVERBERATED signal.  The responses have unit
        energy and the spectrograms are normalised per utterance, so there is no level pass.
    DRAW ORDER per batch: the perturbation block (draw_perturbation), the reverb block (draw_reverb), then draw_augmentation's.  Without
    a bank there is no reverb draw and no launch: the Generator's stream and the batches are what they are without the feature.
    The draws are made on the host from the front-end's own numpy Generator, in the order documented at `draw_augmentation`; `seed=None`
    takes the seed from numpy's global state (offset by the rank under torch.distributed; only when there is something to draw), a fixed
    seed gives bit-identical batches.
    With augment=False (default) the output is that of the plain front-end.  `resample=True` lets the noise bank it builds from
    audio_conf.noise_dir hold off-rate files (NoiseInjection(resample=True)); the front-end itself always works at audio_conf.sample_rate."""

    def __init__(self, audio_conf, normalize=False, pad_mode="constant", device=None, augment=False, seed=None, freq_mask_param=27,
                 time_mask_param=70, freq_masks=1, time_masks=1, noise=None, speed_volume_perturb=False, tempo_range=(0.85, 1.15),
                 gain_range=(-6, 8), resample=False, reverb=None):
        self.sample_rate = int(audio_conf.sample_rate)
        self.n_fft = int(audio_conf.sample_rate * audio_conf.window_size)
        self.hop = int(audio_conf.sample_rate * audio_conf.window_stride)
        self.window, self.normalize, self.pad_mode, self.device = audio_conf.window, normalize, pad_mode, device
        self.augment = bool(augment)
        self.noise, self.noise_prob, self.spec_augment, self.perturb = None, 0.0, False, False
        self.reverb, self.reverb_prob = None, 0.0
        if self.augment:
            self.perturb = bool(speed_volume_perturb) and bool(getattr(audio_conf, "speed_volume_perturb", False))
            self.tempo_range = (float(tempo_range[0]), float(tempo_range[1]))
            self.gain_range = (float(gain_range[0]), float(gain_range[1]))
            if self.perturb and not 0.5 <= self.tempo_range[0] <= self.tempo_range[1] <= 2.0:
                raise ValueError(f"tempo_range={tempo_range}: tempo factors lie in [0.5, 2]")
            if not (0 <= int(freq_masks) <= 8 and 0 <= int(time_masks) <= 8):
                raise ValueError(f"freq_masks={freq_masks}, time_masks={time_masks}: at most 8 masks of each kind")
            self.freq_mask_param, self.time_mask_param = float(freq_mask_param), float(time_mask_param)
            self.freq_masks, self.time_masks = int(freq_masks), int(time_masks)
            self.spec_augment = bool(getattr(audio_conf, "spec_augment", False))
            if noise is None and getattr(audio_conf, "noise_dir", None) is not None:
                noise = NoiseInjection(audio_conf.noise_dir, audio_conf.sample_rate, noise_levels_of(audio_conf), resample=resample)
            self.noise = noise
            self.noise_prob = float(getattr(audio_conf, "noise_prob", 0.4)) if noise is not None else 0.0
            if reverb is None and getattr(audio_conf, "rir_dir", None) is not None:
                reverb = ImpulseResponses(audio_conf.rir_dir, audio_conf.sample_rate, resample=resample)
            if reverb is not None and reverb.sample_rate != self.sample_rate:
                raise ValueError(f"reverb: the bank is at {reverb.sample_rate} Hz, the front-end at {self.sample_rate} Hz")
            self.reverb = reverb
            self.reverb_prob = float(getattr(audio_conf, "reverb_prob", 0.5)) if reverb is not None else 0.0
            if seed is None and (noise is not None or self.spec_augment or self.perturb or reverb is not None):     # (nothing to draw: numpy's global state is left alone)
                seed = int(np.random.randint(0, 2 ** 31 - 1))
                if torch.distributed.is_available() and torch.distributed.is_initialized():
                    seed += torch.distributed.get_rank()
            self.seed = None if seed is None else int(seed)
            self.rng = np.random.default_rng(self.seed)

    def _dev(self):
        from ..device import resolve_device
        return torch.device(self.device) if self.device is not None else resolve_device("auto")

    def __call__(self, waves, perturb=None):
        """`perturb`: an already drawn (tempo, gain dB) pair of arrays for this batch (GpuAudioDataLoader draws before it sorts); None draws
        here when the perturbation is on."""
        n = [int(len(w)) for w in waves]
        batch = torch.zeros(len(waves), max(n), dtype=torch.float32)
        for i, w in enumerate(waves):
            batch[i, :n[i]] = torch.as_tensor(w, dtype=torch.float32)
        return self.from_device_batch(batch.to(self._dev()), n, perturb=perturb)

    def from_device_batch(self, batch, n, perturb=None):
        """The same front-end on a batch that is on the device already: `batch` (B, >= max(n)) fp32, zeros beyond each utterance's
        n[b] samples (what ops.wave_unpack makes), `n` (B) host integers; `perturb` as in `__call__`.  Every draw is made here, in
        `__call__`'s order."""
        from .. import ops
        dev = batch.device
        n = [int(v) for v in n]
        if self.perturb:
            tempo, gain = perturb if perturb is not None else self.draw_perturbation(len(n))
            batch, _, _ = ops.tempo_gain(batch, n, tempo, gain, self.sample_rate)
            n = self.perturbed_lengths(n, tempo)
        elif perturb is not None:
            raise ValueError("perturb= given, but this front-end does not perturb (augment, speed_volume_perturb and audio_conf.speed_volume_perturb)")
        if self.reverb is not None:
            _, base, taps = self.draw_reverb(len(n))
            if max(n) > 0:
                batch = ops.reverb(batch, n, self.reverb.device_taps(dev), base, taps, max(n))
        if self.augment and (self.noise is not None or self.spec_augment):
            p = self.draw(n)
            nz = {}
            if self.noise is not None:
                nz = dict(noise=self.noise.device_samples(dev), noise_base=p["base"], noise_period=p["period"], noise_start=p["start"],
                          noise_level=p["level"])
            spect, frames = ops.spectrogram_augmented(batch, torch.tensor(n), self.n_fft, self.hop, self.window, self.pad_mode,
                                                      self.normalize, freq_masks=p["freq"] if self.spec_augment else None,
                                                      time_masks=p["time"] if self.spec_augment else None, **nz)
        else:
            spect, frames = ops.spectrogram(batch, torch.tensor(n), self.n_fft, self.hop, self.window, self.pad_mode, self.normalize)
        return spect, frames.float() / float(spect.size(3))

    def draw_perturbation(self, B):
        """The next batch's (tempo, gain dB) arrays (draw_perturbation with this front-end's ranges and Generator)."""
        return draw_perturbation(self.rng, B, self.tempo_range, self.gain_range)

    def draw_reverb(self, B):
        """The next batch's (file, base, taps) arrays (draw_reverb with this front-end's bank, probability and Generator)."""
        return draw_reverb(self.rng, B, self.reverb, self.reverb_prob)

    @staticmethod
    def perturbed_lengths(n_samples, tempo):
        """floor(n / tempo + 0.5) per utterance: the lengths ops.tempo_gain produces (a host computation)."""
        from .. import ops
        return [ops.tempo_out_samples(n, f) for n, f in zip(n_samples, tempo)]

    def draw(self, n_samples):
        """The next batch's augmentation parameters (draw_augmentation with this front-end's settings and Generator)."""
        return draw_augmentation(self.rng, n_samples, self.hop, self.n_fft // 2 + 1, self.noise, self.noise_prob, self.spec_augment,
                                 self.freq_mask_param, self.time_mask_param, self.freq_masks, self.time_masks)


def _check_star(star, labels):
    """get_loader's `star`: None, or a single character outside the label set (the rule of decoders.encode_transcripts)."""
    if star is None:
        return None
    if not isinstance(star, str) or len(star) != 1:
        raise ValueError(f"star must be a single character, got {star!r}")
    if star in labels:
        raise ValueError(f"star {star!r} is a label: choose a character outside the label set")
    return star


class _ManifestDataset(Dataset):
    """What SpectrogramDataset and WaveformDataset share: the manifest, the label map, the star check, the transcript parser and the
    cached item (a subclass's parse_audio, parse_transcript)."""

    def __init__(self, audio_conf, manifest_filepath, labels, caching, resample, star):
        import pandas as pd
        self.df = pd.read_csv(manifest_filepath)
        self.size = len(self.df)
        if isinstance(labels, str):
            labels = dict([(v, k) for k, v in pd.read_csv(labels).to_dict()["label"].items()])
        self.labels_map = labels
        self.star = _check_star(star, labels)
        self.audio_conf, self.caching, self.resample = audio_conf, caching, bool(resample)
        self._cache = {}

    def parse_transcript(self, transcript):
        """spectrogram_dataset.py:70-73: unknown chars and the index-0 (blank) label are dropped.
        With `star` (a single character that is not a label) that character becomes the wildcard id len(labels), one past the last
        class, for CTCLoss(star=True): every other unknown character is dropped first, then runs of wildcards collapse to one."""
        transcript = transcript.replace("\n", "")
        star = getattr(self, "star", None)
        if star is None:
            return list(filter(None, [self.labels_map.get(x) for x in list(transcript)]))
        star_id = len(self.labels_map)
        ids = list(filter(None, [star_id if x == star else self.labels_map.get(x) for x in list(transcript)]))
        return [i for k, i in enumerate(ids) if not (i == star_id and k > 0 and ids[k - 1] == star_id)]

    def _cached(self, cache, index, make):
        """item `index` = make(its manifest row), kept in `cache` with caching=True"""
        if self.caching and index in cache:
            return cache[index]
        item = make(self.df.iloc[index])
        if self.caching:
            cache[index] = item
        return item

    def __getitem__(self, index):
        return self._cached(self._cache, index, lambda row: (self.parse_audio(row.audio_filepath), self.parse_transcript(row.text)))

    def __len__(self):
        return self.size


class SpectrogramDataset(_ManifestDataset):
    def __init__(self, audio_conf, manifest_filepath, labels, normalize=False, spec_augment=False, caching=False, resample=False,
                 star=None):
        super().__init__(audio_conf, manifest_filepath, labels, caching, resample, star)
        self.normalize = normalize                       # (resample: an off-rate WAV file is converted on the host, resample_waveform)
        # spectrogram_parser.py:29-44 / :64-80: noise injection, tempo/gain perturbation and SpecAugment are host-side augmentations of
        # the reference's parser that this loader does not implement — say so instead of training silently without them
        unsupported = [k for k, on in (("noise_dir", getattr(audio_conf, "noise_dir", None) is not None),
                                       ("rir_dir", getattr(audio_conf, "rir_dir", None) is not None),
                                       ("speed_volume_perturb", bool(getattr(audio_conf, "speed_volume_perturb", False))),
                                       ("spec_augment", bool(spec_augment))) if on]
        if unsupported:
            import warnings
            warnings.warn("asr_amd.data.SpectrogramDataset: augmentation(s) requested by audio_conf but not implemented here, ignored: "
                          + ", ".join(unsupported))

    def parse_audio(self, path):
        if path.endswith(".npy"):
            spect = torch.from_numpy(np.load(path)).float()
        elif path.endswith(".pt"):
            spect = torch.load(path).float()
        else:
            sr, y = _read_wav(path)
            if self.resample and sr != self.audio_conf.sample_rate:
                sr, y = int(self.audio_conf.sample_rate), resample_waveform(y, sr, self.audio_conf.sample_rate)
            assert sr == self.audio_conf.sample_rate, f"expected {self.audio_conf.sample_rate} Hz audio"
            spect = torch.from_numpy(_stft_spectrogram(y, sr, self.audio_conf.window_size, self.audio_conf.window_stride,
                                                       self.audio_conf.window))
        if self.normalize:
            spect = (spect - spect.mean()) / spect.std()
        return spect


class WaveformDataset(_ManifestDataset):
    """The dataset behind `get_loader(front_end="gpu")`: the manifest and labels of SpectrogramDataset, but an item is `(waveform (n,) float32
    CPU tensor, transcript ids)` — workers only read WAV files (same scaling as SpectrogramDataset.parse_audio) and transcripts; the
    spectrogram is made per batch on the GPU.  Pre-computed spectrograms (`.npy` / `.pt`) cannot be augmented as waveforms and are refused.
    `caching=True` keeps waveforms, not spectrograms, so the augmentation is drawn anew every epoch.
    `resample=True` accepts WAV files at any supported rate (ops.resample_ratio): the rate in the FILE HEADER counts, the manifest's `fq`
    column is not trusted.  Raw items then carry it — `get_raw` returns `(samples, rate, ids)` and the loader converts the batch on the
    GPU (ops.wave_resample) — while `__getitem__` returns the waveform converted on the host (`resample_waveform`)."""

    def __init__(self, audio_conf, manifest_filepath, labels, caching=False, perturb=False, resample=False, star=None):
        super().__init__(audio_conf, manifest_filepath, labels, caching, resample, star)
        self._raw_cache = {}
        for f in self.df.audio_filepath:
            if str(f).endswith((".npy", ".pt")):
                raise ValueError(f"front_end='gpu' reads waveforms, but the manifest lists a pre-computed spectrogram: {f} "
                                 "(use front_end='host' for .npy / .pt spectrograms)")
        if bool(getattr(audio_conf, "speed_volume_perturb", False)) and not perturb:     # perturb=True: the loader's front-end applies it
            warnings.warn("asr_amd.data (front_end='gpu'): speed_volume_perturb is not implemented, ignored — its sox tempo time-stretch "
                          "needs a resampling kernel of its own and is a separate issue; noise_dir and spec_augment are applied on the GPU")

    def parse_audio(self, path):
        sr, y = _read_wav(path)
        if sr != self.audio_conf.sample_rate:
            if not self.resample:
                raise ValueError(f"{path}: {sr} Hz, expected {self.audio_conf.sample_rate} Hz audio")
            y = resample_waveform(y, sr, self.audio_conf.sample_rate)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def parse_audio_raw(self, path):
        """`parse_audio` for the packed feed: a numpy array, int16 for a 16-bit mono file (its raw samples), float32 otherwise; with
        resample=True `(array, rate of the file header)`, the samples untouched."""
        sr, y = _read_wav_raw(path)
        if self.resample:
            from .. import ops
            ops.resample_ratio(sr, self.audio_conf.sample_rate)        # ValueError for a pair the resampler does not support
            return np.ascontiguousarray(y), int(sr)
        if sr != self.audio_conf.sample_rate:
            raise ValueError(f"{path}: {sr} Hz, expected {self.audio_conf.sample_rate} Hz audio")
        return np.ascontiguousarray(y)

    def get_raw(self, index):
        """Item `index` as `(parse_audio_raw's array, transcript ids)`, with resample=True `(samples, rate, transcript ids)`; `caching=True`
        keeps these arrays (a cache of their own)."""
        def make(row):
            audio = self.parse_audio_raw(row.audio_filepath)
            return (*audio, self.parse_transcript(row.text)) if self.resample else (audio, self.parse_transcript(row.text))
        return self._cached(self._raw_cache, index, make)

    def raw_items(self):
        """A Dataset over the same manifest whose items are `get_raw`'s: what the workers of the packed feed read."""
        return _RawWaveforms(self)


class _RawWaveforms(Dataset):
    def __init__(self, dataset):
        self.dataset = dataset

    def __getitem__(self, index):
        return self.dataset.get_raw(index)

    def __len__(self):
        return len(self.dataset)


def _waveform_batch(batch):
    return batch


def packed_layout(lengths, limit=WAVE_MAX_ELEMS):
    """(offsets (B,) int64, total) of a packed batch: utterance b occupies [offsets[b], offsets[b] + lengths[b]), every offset a multiple
    of WAVE_ALIGN elements, total = the 8-aligned end of the last one.  ValueError when the total does not fit the device's int32."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if (lengths < 0).any():
        raise ValueError(f"packed_layout: negative length in {lengths.tolist()}")
    padded = (lengths + WAVE_ALIGN - 1) // WAVE_ALIGN * WAVE_ALIGN
    ends = np.cumsum(padded)
    total = int(ends[-1]) if len(ends) else 0
    if total > limit:
        raise ValueError(f"a packed batch of {total} elements does not fit int32 device offsets (at most {limit}): use a smaller batch")
    return (ends - padded).astype(np.int64), total


def pack_waveforms(batch):
    """Worker-side collate_fn of the packed feed (a pure host function): a list of `(samples, transcript)` items, samples a 1-D int16 or
    float32 array, -> `(buffer, offsets, lengths, transcripts)`: ONE ragged 1-D tensor per batch, laid out by `packed_layout` (gaps are
    zero), int16 when EVERY item is int16 (raw 16-bit mono PCM), else float32 with the int16 items scaled like `_read_wav` does
    (/ 32768) — so both buffers unpack to the bits of the per-item float32 path; offsets, lengths: (B,) int64 numpy arrays.
    Items that carry their sample rate, `(samples, rate, transcript)` (WaveformDataset(resample=True)), give a fifth field: rates, (B,)
    int64.  All items of a batch have the same form."""
    if len({len(item) for item in batch}) > 1:
        raise ValueError("pack_waveforms: items with and without a sample rate in one batch")
    rates = np.array([item[1] for item in batch], dtype=np.int64) if batch and len(batch[0]) == 3 else None
    batch = [(item[0], item[-1]) for item in batch]
    waves = [np.asarray(w) for w, _ in batch]
    for w in waves:
        if w.ndim != 1 or w.dtype not in (np.int16, np.float32):
            raise ValueError(f"pack_waveforms: expected 1-D int16 or float32 samples, got {w.dtype} with shape {w.shape}")
    dtype = np.int16 if all(w.dtype == np.int16 for w in waves) else np.float32
    lengths = np.array([len(w) for w in waves], dtype=np.int64)
    offsets, total = packed_layout(lengths)
    buf = np.zeros(total, dtype=dtype)
    for w, o in zip(waves, offsets.tolist()):
        buf[o:o + len(w)] = w if w.dtype == dtype else w.astype(np.float32) / 32768.0
    packed = (torch.from_numpy(buf), offsets, lengths, [t for _, t in batch])
    return packed if rates is None else packed + (rates,)


class _FeedEnd:
    """Last item of a feeder's queue: the epoch is over (exc None) or the feeder / a worker failed (exc is raised in the consumer)."""

    def __init__(self, exc=None):
        self.exc = exc


def _feed_batches(batches, device, depth, put, stop):
    torch.cuda.set_device(device)
    stream = torch.cuda.Stream(device)
    ring = [None] * (depth + 1)                         # [pinned uint8 buffer, event of the last copy out of it]
    k = 0
    while not stop.is_set():
        try:
            buf, *fields = next(batches)                # (offsets, lengths, transcripts[, rates])
        except StopIteration:
            return
        nbytes = buf.numel() * buf.element_size()
        slot = ring[k % len(ring)]
        if slot is not None:
            slot[1].synchronize()
        if slot is None or slot[0].numel() < nbytes:
            slot = ring[k % len(ring)] = [torch.empty(max(nbytes, 16), dtype=torch.uint8, pin_memory=True), None]
        host = slot[0][:nbytes].view(buf.dtype)
        host.copy_(buf)
        copied = torch.cuda.Event()
        with torch.cuda.stream(stream):
            dev = torch.empty(buf.numel(), dtype=buf.dtype, device=device)
            dev.copy_(host, non_blocking=True)
            copied.record(stream)
        slot[1] = copied
        if not put((dev, copied, *fields)):
            return
        del buf, dev
        k += 1


def _feed(batches, device, depth, out, stop):
    """Body of the feeder thread: packed host batches -> a ring of depth + 1 pinned buffers (grown on demand, a slot reused only after
    its copy event) -> asynchronous copies on a copy stream of its own -> `out`, a queue of (device buffer, copy event, offsets, lengths,
    transcripts[, rates]).  No random draw and no kernel here: only host copies and host-to-device copies."""
    import queue
    import traceback

    def put(item):
        while not stop.is_set():
            try:
                out.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False
    try:
        _feed_batches(batches, device, depth, put, stop)
        put(_FeedEnd())
    except BaseException as e:                          # noqa: BLE001 — a worker's or this thread's failure is the consumer's to raise
        # the frames below hold pinned and device buffers, events and the DataLoader iterator: an exception that outlives this thread must
        # not keep them alive (garbage with GPU resources that a later fork hands to worker processes, which must never free it)
        traceback.clear_frames(e.__traceback__)
        put(_FeedEnd(e))
    finally:
        batches = None                                  # the DataLoader iterator goes here: its workers are shut down


class _WaveformFeeder:
    """One background thread per iterator of a prefetching GpuAudioDataLoader (`_feed`), and the consumer's end of its queue."""

    def __init__(self, batches, device, depth):
        import queue
        import threading
        self.queue, self.stop = queue.Queue(maxsize=depth), threading.Event()
        self.thread = threading.Thread(target=_feed, args=(batches, device, depth, self.queue, self.stop), name="asr_amd-waveform-feeder",
                                       daemon=True)
        self.thread.start()

    def get(self):
        """The next queued batch, None at the end of the epoch; raises what the feeder or a worker raised, or RuntimeError when the thread
        is gone without a word."""
        import queue
        while True:
            try:
                item = self.queue.get(timeout=0.2)
            except queue.Empty:
                if not self.thread.is_alive() and self.queue.empty():
                    raise RuntimeError("asr_amd.data: the waveform feeder thread ended without finishing the epoch")
                continue
            if isinstance(item, _FeedEnd):
                exc, item = item.exc, None
                if exc is not None:
                    try:
                        raise exc
                    finally:
                        exc = None                      # (no cycle exception -> traceback -> this frame -> exception)
                return None
            return item

    def close(self):
        import queue
        self.stop.set()
        while self.thread.is_alive():
            try:
                self.queue.get_nowait()
            except queue.Empty:
                pass
            self.thread.join(0.05)


class GpuAudioDataLoader:
    """Iterates a DataLoader of (waveform, transcript) items and turns each batch into the `_collate_fn` 4-tuple in the MAIN process:
    `(inputs (B,1,161,T) on the GPU, targets, input_percentages, target_sizes)`.  Items are sorted like _collate_fn (frame count 1 + n // hop,
    descending, stable), then GpuSpectrogramFrontEnd makes the spectrograms (and draws the augmentation, in that sorted order).  With a
    perturbing front-end the tempo / gain draws come first, in arrival order, and n is the perturbed length floor(n / tempo + 0.5).

    `prefetch=N >= 1` is the pipelined feed, batch for batch bit-identical to `prefetch=0`: the workers pack every batch into ONE ragged
    buffer (`pack_waveforms`: raw int16 PCM when every file is 16-bit mono), a feeder thread per iterator copies it through a ring of
    N + 1 pinned buffers to the device on a copy stream of its own, up to N batches ahead, and the consumer — `next()`, on the caller's
    current stream — makes ALL the draws, waits for the copy event, unpacks (ops.wave_unpack: scale, sort, zero padding) and runs the same
    front-end kernels, in order between the train steps; only host work and the host-to-device copy overlap a step.

    A dataset with `resample=True` hands over files at their own rates.  The lengths at the front-end's rate, ceil(n L / M), are computed
    on the host first — tempo draws, the sort and input_percentages all use them — and the batch is converted where it is unpacked
    (ops.wave_resample in place of ops.wave_unpack; a batch whose files are all at the target rate still takes ops.wave_unpack, so it is
    bit-identical to the resample=False batch).  `prefetch=0` then packs on the host too (`pack_waveforms`) and takes the same route."""

    def __init__(self, dataset, batch_sampler, num_workers, front_end, prefetch=0):
        self.dataset, self.batch_sampler, self.front_end, self.prefetch = dataset, batch_sampler, front_end, int(prefetch)
        self.resample = bool(getattr(dataset, "resample", False))
        if self.prefetch or self.resample:
            self.loader = DataLoader(dataset.raw_items(), num_workers=num_workers, batch_sampler=batch_sampler, collate_fn=pack_waveforms)
        else:
            self.loader = DataLoader(dataset, num_workers=num_workers, batch_sampler=batch_sampler, collate_fn=_waveform_batch)

    def __len__(self):
        return len(self.loader)

    def _sort(self, lengths):
        """The draws that precede the front-end's and the batch order: (order, lengths in that order — perturbed ones with a perturbing
        front-end —, perturb)."""
        hop = self.front_end.hop
        perturb = None
        if self.front_end.perturb:                       # drawn in arrival order; the batch is then sorted by its PERTURBED lengths
            tempo, gain = self.front_end.draw_perturbation(len(lengths))
            lengths = self.front_end.perturbed_lengths(lengths, tempo)
        frames = [1 + n // hop if n > 0 else 0 for n in lengths]
        order = sorted(range(len(lengths)), key=lambda i: frames[i], reverse=True)
        if self.front_end.perturb:
            perturb = (tempo[order], gain[order])
        return order, [lengths[i] for i in order], perturb

    def _batch(self, inputs, lengths, transcripts):
        hop, max_len = self.front_end.hop, inputs.size(3)
        input_percentages = torch.zeros(len(lengths), dtype=torch.float32)
        target_sizes = torch.zeros(len(lengths), dtype=torch.int32)
        targets = []
        for i, target in enumerate(transcripts):
            input_percentages[i] = min(1 + lengths[i] // hop, max_len) / float(max_len)
            target_sizes[i] = len(target)
            targets.extend(target)
        return inputs, torch.tensor(targets, dtype=torch.int32), input_percentages, target_sizes

    def collate(self, batch):
        order, lengths, perturb = self._sort([len(w) for w, _ in batch])
        batch = [batch[i] for i in order]
        inputs, _ = self.front_end([w for w, _ in batch], perturb=perturb)
        return self._batch(inputs, lengths, [t for _, t in batch])

    def collate_packed(self, packed, offsets, lengths, transcripts, rates=None):
        """`collate` for a packed batch whose buffer is on the device: the same draws in the same order, the sort as the unpack
        kernel's row index.  `rates`: the files' sample rates when the dataset resamples (None: all at the front-end's rate)."""
        from .. import ops
        raw = [int(v) for v in lengths]
        target = self.front_end.sample_rate
        convert = rates is not None and any(int(r) != target for r in rates)
        at_target = [ops.resample_out_samples(n, r, target) for n, r in zip(raw, rates)] if convert else raw
        order, lengths, perturb = self._sort(at_target)
        n_in = [at_target[i] for i in order]
        if convert:
            waves, _ = ops.wave_resample(packed, offsets, raw, [int(r) for r in rates], order, target, max(n_in), n_out=at_target)
        else:
            waves = ops.wave_unpack(packed, offsets, raw, order, max(n_in))
        inputs, _ = self.front_end.from_device_batch(waves, n_in, perturb=perturb)
        return self._batch(inputs, lengths, [transcripts[i] for i in order])

    def __iter__(self):
        if not self.prefetch and self.resample:          # synchronous, but packed on the host and converted by the same kernel
            dev = self.front_end._dev()
            for buf, *fields in self.loader:
                yield self.collate_packed(buf.to(dev), *fields)
            return
        if not self.prefetch:
            for batch in self.loader:
                yield self.collate(batch)
            return
        dev = self.front_end._dev()
        if dev.type != "cuda":
            raise RuntimeError(f"prefetch={self.prefetch} needs the GPU front-end's device, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())          # the feeder thread sets it: threads do not inherit it
        feeder = _WaveformFeeder(iter(self.loader), dev, self.prefetch)       # (the workers start here, in the caller's thread)
        try:
            while True:
                item = feeder.get()
                if item is None:
                    return
                packed, copied, *fields = item
                stream = torch.cuda.current_stream(dev)
                stream.wait_event(copied)
                out = self.collate_packed(packed, *fields)
                packed.record_stream(stream)             # allocated on the copy stream, read by the unpack kernel on this one
                del item, packed
                yield out
        finally:
            feeder.close()


def _durations_of(data_source, durations=None):
    """Per-item lengths for bucketing: explicit sequence, else the manifest's `duration` column (etl/jsut_dataset.py:36-42,
    etl/librispeech_dataset.py:100-103 write it), else the text length as a proxy."""
    if durations is not None:
        d = np.asarray(list(durations), dtype=np.float64)
    else:
        df = getattr(data_source, "df", None)
        if df is not None and "duration" in df.columns:
            d = df["duration"].to_numpy(dtype=np.float64)
        elif df is not None and "text_size" in df.columns:
            d = df["text_size"].to_numpy(dtype=np.float64)
        else:
            raise ValueError("length bucketing needs per-item durations: pass `durations=` or a manifest with a `duration` column")
    if len(d) != len(data_source):
        raise ValueError(f"{len(d)} durations for {len(data_source)} items")
    return d


def _item_order(self, data_source, durations, descending, order):
    """Item ids in binning order: by duration (stable; ties by manifest index) or as the manifest lists them."""
    if order == "manifest":
        self.durations = None
        return list(range(len(data_source)))
    if order != "duration":
        raise ValueError(f"order={order!r}: expected duration or manifest")
    self.durations = _durations_of(data_source, durations)
    return np.argsort(-self.durations if descending else self.durations, kind="stable").tolist()


def _full_bins(order, batch_size, partial):
    """Consecutive runs of `batch_size` ids of a length-sorted order.  A short last run is kept as it is ("keep": the reference's
    BucketingSampler behaviour, bucketing_sampler.py:13-14), dropped ("drop") or topped up with its nearest-in-length neighbours — the
    ids just before it, which then occur twice in the epoch ("fill")."""
    if partial not in ("keep", "drop", "fill"):
        raise ValueError(f"partial={partial!r}: expected keep, drop or fill")
    bins = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
    if bins and len(bins[-1]) < batch_size and len(order) >= batch_size:
        if partial == "drop":
            bins.pop()
        elif partial == "fill":
            need = batch_size - len(bins[-1])
            bins[-1] = order[len(order) - len(bins[-1]) - need:len(order) - len(bins[-1])] + bins[-1]
    return bins


class LengthBucketingSampler(Sampler):
    """True length bucketing (BASELINE configs[3] "bucketed sampler" / configs[4] "length-sorted batching").

    The reference's BucketingSampler (data/samplers/bucketing_sampler.py:5-25) only ASSUMES a manifest "in order of size" (its ETL merely
    bounds the lengths, etl/__main__.py:48); this one establishes the order: items are sorted by duration (stable, ties by manifest
    index), consecutive runs of `batch_size` form the bins, and the interface is the reference's — `__iter__` yields one bin per batch
    (ids shuffled inside the bin like the reference; `_collate_fn` re-sorts a batch by length anyway), `__len__` = number of bins,
    `shuffle()` permutes the bin ORDER (batches stay homogeneous in length, epochs see them in a different order)."""

    def __init__(self, data_source, batch_size=1, durations=None, descending=False, partial="keep", order="duration"):
        super().__init__()
        self.data_source = data_source
        self.batch_size = int(batch_size)
        self.bins = _full_bins(_item_order(self, data_source, durations, descending, order), self.batch_size, partial)

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch=None):
        if epoch is None:
            np.random.shuffle(self.bins)                 # the reference's call (bucketing_sampler.py:24-25)
        else:
            g = torch.Generator()
            g.manual_seed(int(epoch))
            self.bins = [self.bins[i] for i in torch.randperm(len(self.bins), generator=g).tolist()]

    def bin_spread(self):
        """max - min duration inside each bin (what bucketing minimises; used by the tests and the bench)."""
        return [float(self.durations[b].max() - self.durations[b].min()) for b in self.bins]


class BucketingSampler(LengthBucketingSampler):
    """The reference's sampler of this name (data/samplers/bucketing_sampler.py:5-25: bins of consecutive manifest rows, "assuming they are
    in order of size") = the length-bucketing sampler with the manifest order taken as given.  Bins, in-bin shuffle and `shuffle()` are
    held to the reference's own output in tests/golden/data_formats.json."""

    def __init__(self, data_source, batch_size=1):
        super().__init__(data_source, batch_size=batch_size, order="manifest")


class DistributedLengthBucketingSampler(Sampler):
    """Length bucketing for one-process-per-GPU data parallelism: the partition rule is the reference's (rank r takes every
    `num_replicas`-th bin starting at r, distributed_bucketing_sampler.py:22-34), applied to LENGTH-SORTED bins, and the epoch shuffle
    moves whole ROUNDS (the `num_replicas` bins that the ranks process concurrently) instead of single bins — so at every step all ranks
    hold batches that are neighbours in length, and the gradient all-reduce does not wait for a straggler with a much longer T
    ("for C5 sort by length first so concurrent ranks get similar T").  The tail is padded to a whole round with the
    bins just before it (nearest in length), where the reference wraps around to the first bins (which here would put the SHORTEST
    batches next to the LONGEST ones in the last round).

    `order="manifest"`, `pad="wrap"`, `shuffle_unit="bin"` select the reference's own behaviour instead (DistributedBucketingSampler below):
    manifest order, wrap-around padding applied AFTER the shuffle, single bins permuted."""

    _fill_logged = False

    def __init__(self, data_source, batch_size=1, num_replicas=None, rank=None, durations=None, descending=False, partial="keep",
                 order="duration", pad="nearest", shuffle_unit="round"):
        super().__init__()
        if num_replicas is None:
            num_replicas = torch.distributed.get_world_size()
        if rank is None:
            rank = torch.distributed.get_rank()
        if pad not in ("nearest", "wrap") or shuffle_unit not in ("round", "bin"):
            raise ValueError(f"pad={pad!r} / shuffle_unit={shuffle_unit!r}: expected nearest | wrap and round | bin")
        self.data_source, self.batch_size = data_source, int(batch_size)
        self.num_replicas, self.rank = int(num_replicas), int(rank)
        self.pad, self.shuffle_unit = pad, shuffle_unit
        self.ids = _item_order(self, data_source, durations, descending, order)
        # partial="keep" (default, the reference sampler's behaviour: the short last bin stays short, epochs are composed exactly as with
        # data/samplers/distributed_bucketing_sampler.py).  partial="fill" tops the short bin up with the ids just before it, so that every
        # rank of every round runs the SAME batch size — gradients are averaged unweighted, and a rank whose B is not a multiple of 8 leaves
        # the packed bf16 fast path and straggles in the all-reduce; it duplicates samples within an epoch (logged once), so it is opt-in.
        self.bins = _full_bins(self.ids, self.batch_size, partial)
        if partial == "fill" and len(self.ids) % self.batch_size and not DistributedLengthBucketingSampler._fill_logged:
            DistributedLengthBucketingSampler._fill_logged = True
            print(f"[asr_amd] DistributedLengthBucketingSampler(partial='fill'): the last bin is topped up with "
                  f"{self.batch_size - len(self.ids) % self.batch_size} duplicate sample(s) per epoch", flush=True)
        self.num_samples = int(math.ceil(len(self.bins) / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas
        self._round_order = None                                   # shuffle_unit="round": permutation of the rounds, set by shuffle()

    def _padded(self):
        """The bins of one epoch, padded to a whole number of rounds."""
        pad = self.total_size - len(self.bins)
        if self.pad == "wrap":                                     # the reference: the epoch's first bins again
            bins = self.bins + self.bins[:pad]
            assert len(bins) == self.total_size                    # (its own assertion: fails when there are fewer bins than padding)
            return bins
        if not pad:
            return self.bins
        src = self.bins[-(pad + 1):-1] if len(self.bins) > pad else (self.bins * (pad // max(len(self.bins), 1) + 1))[:pad]
        return self.bins + [list(b) for b in src]

    @property
    def rounds(self):
        bins = self._padded()
        rounds = [bins[i:i + self.num_replicas] for i in range(0, self.total_size, self.num_replicas)]
        return rounds if self._round_order is None else [rounds[i] for i in self._round_order]

    def __iter__(self):
        return iter([r[self.rank] for r in self.rounds])

    def __len__(self):
        return self.num_samples

    def shuffle(self, epoch):
        g = torch.Generator()
        g.manual_seed(int(epoch))
        if self.shuffle_unit == "bin":
            self.bins = [self.bins[i] for i in torch.randperm(len(self.bins), generator=g).tolist()]
        else:
            prev = self._round_order if self._round_order is not None else list(range(self.num_samples))
            self._round_order = [prev[i] for i in torch.randperm(self.num_samples, generator=g).tolist()]


class DistributedBucketingSampler(DistributedLengthBucketingSampler):
    """The reference's sampler of this name (data/samplers/distributed_bucketing_sampler.py:8-44; dead code there, the SURVEY §8(e) partition
    rule here): bins of consecutive manifest rows, rank r takes bins[r::world] of the bin list wrap-padded to a multiple of world, `shuffle(epoch)`
    permutes the bins with a generator seeded by the epoch.  Same attributes (`ids`, `bins`, `num_replicas`, `rank`, `num_samples`,
    `total_size`); per-rank bins for world 1 / 2 / 4 / 8 and the shuffles are held to the reference's own output (tests/golden/data_formats.json)."""

    def __init__(self, data_source, batch_size=1, num_replicas=None, rank=None):
        super().__init__(data_source, batch_size=batch_size, num_replicas=num_replicas, rank=rank, order="manifest", pad="wrap",
                         shuffle_unit="bin")


def write_manifest(records, path):
    """Manifest CSV in the layout the reference's ETL writes (etl/jsut_dataset.py:36-42 + etl/__main__.py:55: DataFrame.to_csv(index=False)
    with the columns audio_filepath, duration, fq, text, text_size).  `records`: iterable of (audio_filepath, duration, fq, text)."""
    import pandas as pd
    rows = [(str(f), float(d), int(fq), str(t), len(str(t))) for f, d, fq, t in records]
    pd.DataFrame.from_records(rows, columns=["audio_filepath", "duration", "fq", "text", "text_size"]).to_csv(path, index=False)


def export_labels(texts, path):
    """labels.csv as the reference writes it (etl/jsut_dataset.py:56-60): one `label` column holding every character of the corpus; the
    reference emits the set in hash order, this writes it sorted (index 0 = CTC blank is whatever row comes first, as there)."""
    import pandas as pd
    chars = set()
    for t in texts:
        chars |= set(t)
    pd.DataFrame.from_records([(c,) for c in sorted(chars)], columns=["label"]).to_csv(path, index=False)


def clean_jsut_text(line):
    """`key:text` line of a JSUT transcript_utf8.txt -> (key, text) with spaces, newlines and the two Japanese punctuation marks removed
    (etl/jsut_dataset.py:46-50)."""
    k, v = line.split(":")
    for ch in (" ", "\n", "\u3001", "\u3002"):
        v = v.replace(ch, "")
    return k, v


class AudioDataLoader(DataLoader):
    """data/loaders/audio_data_loader.py:7-13."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.collate_fn = _collate_fn


def get_loader(audio_conf, labels, manifest, batch_size, num_workers, caching=False, length_bucketing=False, front_end="host",
               perturb=False, prefetch=0, resample=False, star=None):
    """data/loaders/functional.py:6-24.  `length_bucketing=True` (not in the reference) sorts the manifest by its `duration` column
    before binning (LengthBucketingSampler; the distributed variant when torch.distributed is initialised).

    front_end="host" (default): SpectrogramDataset + AudioDataLoader, spectrograms per item in the workers, no augmentation.
    front_end="gpu": WaveformDataset + GpuAudioDataLoader — workers read WAV files and transcripts only; per batch, in the main process,
    GpuSpectrogramFrontEnd(normalize=True, augment=True) makes the spectrograms on the GPU with the noise injection (audio_conf.noise_dir,
    noise_prob, noise_levels or noise_min / noise_max) and SpecAugment (audio_conf.spec_augment) that audio_conf asks for.  Batches are the
    same 4-tuple, `inputs` already on the GPU.  With caching=True the waveforms are cached and the augmentation is redrawn every epoch.
    `perturb=True` (front_end="gpu" only) also applies audio_conf.speed_volume_perturb there: tempo ~ U(0.85, 1.15) and gain ~ U(-6, 8) dB per
    utterance, first of all, the batch sorted by its perturbed lengths (ops.tempo_gain; modelled on sox's effects, parity with sox unpinned).
    With the default perturb=False the switch is ignored with a warning, as on the host path.
    `prefetch=N` (front_end="gpu" only; an integer >= 0, default 0 = the synchronous loader): the pipelined feed.  The workers return
    one packed buffer per batch (raw int16 for 16-bit mono files, float32 otherwise), a feeder thread stages it in pinned memory and
    copies it to the GPU on a copy stream up to N batches ahead of the consumer, and `next()` unpacks it on the GPU (ops.wave_unpack)
    and runs the same front-end kernels on the caller's stream.  Every batch is bit-identical to the `prefetch=0` batch for the same
    seeds; the sampler's draws from numpy's global state are made up to N batches early, so code that draws from that state inside the
    loop sees them interleaved differently.  Leaving the loop early stops the thread and the workers; a worker's error is raised by
    `next()`.
    `resample=True` (default False: a file at another rate is an error) accepts WAV files at any supported rate — the rate of the file
    header, a ratio to audio_conf.sample_rate in [1/8, 8] with a small enough polyphase table (ops.resample_ratio; 48, 44.1, 22.05 and
    8 kHz against 16 kHz are) — and converts each to audio_conf.sample_rate by Kaiser-windowed sinc interpolation: with front_end="gpu"
    per batch on the GPU, fused into the unpack pass (ops.wave_resample), ahead of the unchanged tempo, noise, STFT and SpecAugment
    kernels, for `prefetch=0` too; the noise bank converts its off-rate files once; with front_end="host" per item in the workers
    (`resample_waveform`).  Parity with sox / ffmpeg is unpinned.
    `audio_conf.rir_dir` (front_end="gpu"; needs no parameter here, works with `prefetch` too): a directory of room impulse responses —
    with probability `audio_conf.reverb_prob` (default 0.5, a starting point: which value serves real recordings is unmeasured) an
    utterance is reverberated on the GPU (ImpulseResponses, ops.reverb) after tempo / gain and before the noise; `resample` is passed on to
    the bank.  With front_end="host" a set `rir_dir` is ignored with a warning, like the other augmentations.
    `star="*"` (default None: the ids are exactly the ones above): that character, any single one that is not a label, in a manifest's
    transcript becomes the wildcard id len(labels) for `asr_amd.CTCLoss(star=True)` — "this part was not transcribed"; characters that
    are neither a label nor the star are dropped first, then runs of wildcards collapse to one."""
    if front_end not in ("host", "gpu"):
        raise ValueError(f"front_end={front_end!r}: expected host or gpu")
    if perturb and front_end != "gpu":
        raise ValueError("perturb=True needs front_end='gpu' (the host front-end has no tempo / gain perturbation)")
    if isinstance(prefetch, bool) or not isinstance(prefetch, (int, np.integer)) or prefetch < 0:
        raise ValueError(f"prefetch={prefetch!r}: expected an integer >= 0 (batches staged ahead of the consumer)")
    if prefetch and front_end != "gpu":
        raise ValueError("prefetch needs front_end='gpu' (the host front-end's batches are made in the workers already)")
    if front_end == "gpu":
        dataset = WaveformDataset(audio_conf=audio_conf, manifest_filepath=manifest, labels=labels, caching=caching, perturb=perturb,
                                  resample=bool(resample), star=star)
        fe = GpuSpectrogramFrontEnd(audio_conf, normalize=True, augment=True, speed_volume_perturb=perturb, resample=bool(resample))
        make = lambda sampler: GpuAudioDataLoader(dataset, sampler, num_workers, fe, prefetch=int(prefetch))      # noqa: E731
    else:
        dataset = SpectrogramDataset(audio_conf=audio_conf, manifest_filepath=manifest, labels=labels, normalize=True,
                                     spec_augment=getattr(audio_conf, "spec_augment", False), caching=caching, resample=bool(resample),
                                     star=star)
        make = lambda sampler: AudioDataLoader(dataset, num_workers=num_workers, batch_sampler=sampler)   # noqa: E731
    if length_bucketing and torch.distributed.is_available() and torch.distributed.is_initialized():
        sampler = DistributedLengthBucketingSampler(dataset, batch_size=batch_size)
        loader = make(sampler)
        sampler.shuffle(0)
        return loader, sampler
    sampler = (LengthBucketingSampler if length_bucketing else BucketingSampler)(dataset, batch_size=batch_size)
    loader = make(sampler)
    sampler.shuffle()
    return loader, sampler
