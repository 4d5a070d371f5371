"""Host side of the tempo / gain perturbation (no GPU needed): properties of the fp64 oracle the kernels are held to, the draws and
their order, the host entry points of the C ABI, and the `perturb` switch of get_loader."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import tempo_oracle as T


def conf(**kw):
    c = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def signal(n, seed=0, grid=True):
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 733 * t + 1) + 0.05 * np.random.default_rng(seed).standard_normal(n)
    return (np.rint(x * 32768) / 32768 if grid else x).astype(np.float32)


def test_oracle_sizes_and_identity():
    assert T.sizes(16000) == (1312, 235, 192)
    for n in (0, 1, 191, 1312, 4321, 160000):
        x = signal(n)
        y, d = T.tempo_gain(x, 1.0)
        assert np.array_equal(y.astype(np.float32), x) and y.dtype == np.float64 and (d == 0).all()


@pytest.mark.parametrize("f", [0.85, 0.93, 1.07, 1.15])
def test_oracle_length_and_offsets(f):
    R = T.sizes(16000)[1]
    for n in (0, 1, 191, 1312, 4321, 160000):
        y, d = T.tempo_gain(signal(n), f)
        assert len(y) == int(np.floor(n / f + 0.5)) == T.out_samples(n, f)
        assert len(d) == -(-len(y) // 1120) and (d >= 0).all() and (d < R).all() and (len(d) == 0 or d[0] == 0)


@pytest.mark.parametrize("f", [0.85, 1.15])
def test_oracle_keeps_the_pitch(f):
    """A two-tone signal, stretched: the spectral peak stays within one FFT bin of 220 Hz (a resampler would move it to 220 / f),
    and the gain is applied and clipped last."""
    x = signal(160000)
    y, _ = T.tempo_gain(x, f)
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    assert abs(int(np.argmax(spec)) - 220.0 * len(y) / 16000.0) <= 1.0
    G = np.float32(10 ** (8 / 20.0))
    loud, _ = T.tempo_gain(x, f, G)
    assert np.array_equal(loud, np.clip(float(G) * y, -1, 1)) and (np.abs(loud) == 1.0).any() and np.abs(loud).max() == 1.0


def test_draw_perturbation_order_and_ranges():
    from asr_amd.data import draw_perturbation
    tempo, gain = draw_perturbation(np.random.default_rng(5), 7)
    rng = np.random.default_rng(5)
    for b in range(7):
        assert tempo[b] == rng.uniform(0.85, 1.15) and gain[b] == rng.uniform(-6, 8)
    assert tempo.dtype == gain.dtype == np.float64
    tempo, gain = draw_perturbation(np.random.default_rng(6), 500, tempo_range=(0.9, 1.1), gain_range=(-3, 0))
    assert tempo.min() >= 0.9 and tempo.max() < 1.1 and gain.min() >= -3 and gain.max() < 0 and tempo.std() > 0.03
    assert len(draw_perturbation(np.random.default_rng(0), 0)[0]) == 0


def test_front_end_draws_are_unchanged_with_the_feature_off():
    """Off (the default, or audio_conf without the switch): draw() is draw_augmentation on a fresh Generator — not one extra number.
    On: one block of 2 B numbers first, then draw_augmentation fed the perturbed lengths."""
    from asr_amd.data import GpuSpectrogramFrontEnd, draw_augmentation, draw_perturbation
    lens = [16000, 8000, 4321]
    want = draw_augmentation(np.random.default_rng(11), lens, 160, 161, None, 0.0, True, 27.0, 70.0, 1, 1)
    for kw in (dict(), dict(speed_volume_perturb=True)):                       # the second: audio_conf does not ask for it
        fe = GpuSpectrogramFrontEnd(conf(spec_augment=True), augment=True, seed=11, **kw)
        assert not fe.perturb
        got = fe.draw(lens)
        assert all(np.array_equal(got[k], want[k]) for k in want)
    assert not GpuSpectrogramFrontEnd(conf(spec_augment=True, speed_volume_perturb=True), augment=True, seed=11).perturb
    assert not GpuSpectrogramFrontEnd(conf(speed_volume_perturb=True), speed_volume_perturb=True).perturb      # augment=False
    fe = GpuSpectrogramFrontEnd(conf(spec_augment=True, speed_volume_perturb=True), augment=True, seed=11, speed_volume_perturb=True)
    assert fe.perturb
    tempo, gain = fe.draw_perturbation(3)
    n_out = fe.perturbed_lengths(lens, tempo)
    got = fe.draw(n_out)
    rng = np.random.default_rng(11)
    t2, g2 = draw_perturbation(rng, 3)
    want = draw_augmentation(rng, [T.out_samples(n, f) for n, f in zip(lens, t2)], 160, 161, None, 0.0, True, 27.0, 70.0, 1, 1)
    assert np.array_equal(tempo, t2) and np.array_equal(gain, g2) and all(np.array_equal(got[k], want[k]) for k in want)
    assert (got["time"][:, 0, 1] <= [1 + n // 160 for n in n_out]).all()
    with pytest.raises(ValueError):
        GpuSpectrogramFrontEnd(conf(speed_volume_perturb=True), augment=True, speed_volume_perturb=True, tempo_range=(0.4, 1.0))


def test_host_entry_points_match_the_oracle():
    from asr_amd import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for f in [0.5, 0.85, 0.93, 1.0, 1.07, 1.15, 2.0] + rng.uniform(0.5, 2.0, 200).tolist():
        for n in [0, 1, 2, 191, 1312, 4321, 160000, 2 ** 29] + rng.integers(0, 2 ** 29, 20).tolist():
            assert lib.ds2_tempo_out_samples(int(n), float(f)) == T.out_samples(int(n), float(f)) == ops.tempo_out_samples(n, f)
    for n, f in ((-1, 1.0), (2 ** 29 + 1, 1.0), (100, 0.49), (100, 2.01), (100, float("nan"))):
        assert lib.ds2_tempo_out_samples(n, f) == -1
        with pytest.raises(_lib.DS2LibraryError):
            ops.tempo_out_samples(n, f)
    for sr in (8000, 11025, 16000, 22050, 44100, 48000):
        assert ops.tempo_sizes(sr) == T.sizes(sr)
    assert ops.tempo_sizes(16000) == (1312, 235, 192)
    for bad in (dict(segment_ms=20.0), dict(search_ms=0.01), dict(search_ms=200.0), dict(overlap_ms=0.0)):    # S <= 2 O, R = 0, R + O > 2048
        with pytest.raises(_lib.DS2LibraryError):
            ops.tempo_sizes(16000, **bad)
    assert lib.ds2_tempo_workspace_bytes(64) >= 64 * 24


def test_tempo_gain_has_no_cpu_path():
    import torch
    from asr_amd import _lib, ops
    with pytest.raises(_lib.DS2LibraryError):
        ops.tempo_gain(torch.zeros(2, 100), [100, 50], [1.0, 1.1], [0.0, 0.0], 16000)


def _wav_corpus(tmp_path, lengths, sr=16000):
    import pandas as pd
    from scipy.io import wavfile
    rng = np.random.default_rng(2)
    rows = []
    for i, n in enumerate(lengths):
        wavfile.write(str(tmp_path / f"u{i}.wav"), sr, (rng.standard_normal(n) * 3000).astype(np.int16))
        rows.append((str(tmp_path / f"u{i}.wav"), n / sr, sr, "ab c"[: 1 + i % 4]))
    pd.DataFrame({"audio_filepath": [r[0] for r in rows], "duration": [r[1] for r in rows], "fq": [sr] * len(rows),
                  "text": [r[3] for r in rows], "text_size": [len(r[3]) for r in rows]}).to_csv(tmp_path / "manifest.csv", index=False)
    pd.DataFrame({"label": ["_", "a", "b", "c"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def test_get_loader_perturb_switch(tmp_path):
    """perturb=True with the switch on builds without a warning and a perturbing front-end (no GPU touched before the first batch);
    the default still warns with today's text; perturb=True is refused on the host path and is inert without the switch."""
    from asr_amd.data import GpuAudioDataLoader, get_loader
    manifest, labels = _wav_corpus(tmp_path, [8000, 4000, 12000])
    c = conf(speed_volume_perturb=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader, _ = get_loader(c, labels, manifest, batch_size=2, num_workers=0, front_end="gpu", perturb=True)
    assert isinstance(loader, GpuAudioDataLoader) and loader.front_end.perturb
    assert loader.front_end.tempo_range == (0.85, 1.15) and loader.front_end.gain_range == (-6.0, 8.0)
    with pytest.warns(UserWarning, match="speed_volume_perturb is not implemented.*separate issue"):
        loader, _ = get_loader(c, labels, manifest, batch_size=2, num_workers=0, front_end="gpu", perturb=False)
    assert not loader.front_end.perturb
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader, _ = get_loader(conf(), labels, manifest, batch_size=2, num_workers=0, front_end="gpu", perturb=True)
    assert not loader.front_end.perturb
    with pytest.raises(ValueError, match="front_end='gpu'"):
        get_loader(c, labels, manifest, batch_size=2, num_workers=0, front_end="host", perturb=True)
