"""Host side of the augmented GPU front-end (no GPU needed): the noise bank, the reference's inject_noise, the per-utterance draws
and their order, mask bounds, the front_end switch of get_loader."""
import math
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_oracle as A


def conf(**kw):
    c = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def write_noise(tmp_path, sr=16000):
    """Three int16 noise files (one in a subdirectory), a float32 one, a stereo one and two files that are not WAV."""
    from scipy.io import wavfile
    rng = np.random.default_rng(1)
    d = tmp_path / "noise"
    (d / "sub").mkdir(parents=True)
    files = {}
    files["b.wav"] = (rng.standard_normal(3000) * 3000).astype(np.int16)
    files["a.wav"] = (rng.standard_normal(5000) * 1000).astype(np.int16)
    files["sub/c.wav"] = (rng.standard_normal(700) * 8000).astype(np.int16)
    files["d.wav"] = (rng.standard_normal(1200) * 0.1).astype(np.float32)
    files["e.wav"] = (rng.standard_normal((900, 2)) * 2000).astype(np.int16)
    for k, v in files.items():
        wavfile.write(str(d / k), sr, v)
    (d / "x.mp3").write_bytes(b"\x00" * 16)
    (d / "notes.txt").write_text("not audio")
    return d, files


def test_noise_bank_loads_every_wav_once_sorted_and_scaled(tmp_path):
    from asr_amd.data import NoiseInjection
    d, files = write_noise(tmp_path)
    with pytest.warns(UserWarning, match="non-WAV"):
        ni = NoiseInjection(str(d), 16000, (0.1, 0.3))
    names = [p[len(str(d)) + 1:].replace("\\", "/") for p in ni.paths]
    assert names == sorted(names) == ["a.wav", "b.wav", "d.wav", "e.wav", "sub/c.wav"]
    assert ni.samples.dtype == np.float32 and len(ni) == 5
    assert ni.starts.tolist() == [0, 5000, 8000, 9200, 10100] and ni.lengths.tolist() == [5000, 3000, 1200, 900, 700]
    np.testing.assert_array_equal(ni.samples[:5000], files["a.wav"].astype(np.float32) / 32768.0)
    np.testing.assert_array_equal(ni.samples[8000:9200], files["d.wav"])
    np.testing.assert_array_equal(ni.samples[9200:10100], (files["e.wav"].astype(np.float32) / 32768.0).mean(axis=1))
    np.testing.assert_array_equal(ni.samples[10100:], files["sub/c.wav"].astype(np.float32) / 32768.0)
    assert ni.noise_levels == (0.1, 0.3)


def test_noise_bank_errors(tmp_path):
    from scipy.io import wavfile
    from asr_amd.data import NoiseInjection
    with pytest.raises(IOError):
        NoiseInjection(str(tmp_path / "missing"))
    with pytest.raises(IOError):
        NoiseInjection(None)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .wav"):
        NoiseInjection(str(tmp_path / "empty"))
    (tmp_path / "sr").mkdir()
    wavfile.write(str(tmp_path / "sr" / "n.wav"), 8000, np.zeros(100, np.int16))
    with pytest.raises(ValueError, match="8000 Hz"):
        NoiseInjection(str(tmp_path / "sr"), 16000)


def test_noise_levels_fall_back_to_noise_min_max():
    from asr_amd.data import noise_levels_of
    assert noise_levels_of(conf(noise_levels=(0.2, 0.7))) == (0.2, 0.7)
    c = conf(noise_min=0.0, noise_max=0.25)
    del c.noise_levels
    assert noise_levels_of(c) == (0.0, 0.25)                     # the reference's config.yml keys
    c = conf()
    del c.noise_levels
    assert noise_levels_of(c) == (0.0, 0.5)                      # NoiseInjection's default


def test_inject_noise_matches_the_reference_formula(tmp_path):
    """inject_noise_sample == noise_injection.py:33-38 given the same segment; inject_noise draws file, level, u from numpy's global
    state in the reference's order; a noise file shorter than the utterance wraps; a silent segment leaves the data unmixed."""
    from scipy.io import wavfile
    from asr_amd.data import NoiseInjection
    d, _ = write_noise(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ni = NoiseInjection(str(d), 16000, (0.0, 0.5))
    x = (np.sin(np.arange(2000) * 0.01) * 0.3).astype(np.float32)
    for idx, u in ((0, 0.37), (1, 0.99), (4, 0.5)):                  # file 4 (700 samples) is shorter than x: wraps
        seg = A.segment(ni.samples[ni.starts[idx]:ni.starts[idx] + ni.lengths[idx]], len(x), u)
        np.testing.assert_array_equal(ni.segment(idx, len(x), u), seg.astype(np.float32))
        got = ni.inject_noise_sample(x.copy(), idx, 0.3, u)
        want = A.reference_inject_noise_sample(x.astype(np.float64), seg, 0.3)
        assert np.abs(got - want).max() < 1e-6
        assert np.abs(got - A.mix(x, ni.samples[ni.starts[idx]:ni.starts[idx] + ni.lengths[idx]], 0.3, u)).max() < 1e-6
    np.random.seed(7)
    got = ni.inject_noise(x.copy())
    np.random.seed(7)
    idx, lv, u = np.random.choice(len(ni.paths)), np.random.uniform(0.0, 0.5), np.random.rand()
    assert np.abs(got - A.mix(x, ni.samples[ni.starts[idx]:ni.starts[idx] + ni.lengths[idx]], lv, u)).max() < 1e-6
    (tmp_path / "silent").mkdir()
    wavfile.write(str(tmp_path / "silent" / "z.wav"), 16000, np.zeros(4000, np.int16))
    z = NoiseInjection(str(tmp_path / "silent"))
    np.testing.assert_array_equal(z.inject_noise_sample(x.copy(), 0, 0.4, 0.2), x)


def test_draw_order_and_determinism(tmp_path):
    """draw_augmentation consumes the Generator in the documented order (the oracle's restatement gives the same values) and a fixed
    seed gives the same parameters; start = floor(u (L - n)) or floor(u L) for short noise."""
    from asr_amd.data import NoiseInjection, draw_augmentation
    d, _ = write_noise(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ni = NoiseInjection(str(d), 16000, (0.1, 0.6))
    lengths = [16000, 8000, 4321, 777, 250, 160, 3000]
    for spec in (False, True):
        p = draw_augmentation(np.random.default_rng(3), lengths, 160, 161, ni, 0.6, spec, 27, 70, 2, 3)
        want = A.draws(np.random.default_rng(3), lengths, 160, 161, len(ni), 0.6, (0.1, 0.6), spec, 27, 70, 2, 3)
        for b, w in enumerate(want):
            assert (p["file"][b] if p["file"][b] >= 0 else None) == w["file"]
            if w["file"] is not None:
                L = int(ni.lengths[w["file"]])
                assert p["level"][b] == np.float32(w["level"]) and p["u"][b] == w["u"]
                assert p["base"][b] == ni.starts[w["file"]] and p["period"][b] == L
                assert p["start"][b] == (math.floor(w["u"] * (L - lengths[b])) if L >= lengths[b] else math.floor(w["u"] * L))
                assert 0 <= p["start"][b] < L
            else:
                assert p["level"][b] == 0.0
            assert [tuple(r) for r in p["freq"][b].tolist()] == w["freq"] and [tuple(r) for r in p["time"][b].tolist()] == w["time"]
        assert p["freq"].shape == ((7, 2, 2) if spec else (7, 0, 2))
        assert any(f >= 0 for f in p["file"]) and any(f < 0 for f in p["file"])
        q = draw_augmentation(np.random.default_rng(3), lengths, 160, 161, ni, 0.6, spec, 27, 70, 2, 3)
        assert all(np.array_equal(p[k], q[k]) for k in p)


def test_mask_bounds_and_clamping():
    from asr_amd.data import draw_augmentation
    rng = np.random.default_rng(11)
    lengths = [160000, 16000, 4000, 800, 250, 100]                 # tau = 1001, 101, 26, 6, 2, 1: the last four are below T_param = 70
    seen_clamp = False
    for _ in range(200):
        p = draw_augmentation(rng, lengths, 160, 161, spec_augment=True, freq_masks=2, time_masks=2)
        assert (p["file"] < 0).all() and (p["level"] == 0).all()
        for b, n in enumerate(lengths):
            tau = 1 + n // 160
            for lo, hi in p["freq"][b]:
                assert 0 <= lo <= hi <= 161 and hi - lo < 27
            for lo, hi in p["time"][b]:
                assert 0 <= lo <= hi <= tau and hi - lo <= min(69, tau)
                seen_clamp |= (tau < 70 and hi - lo == tau)
    assert seen_clamp


def test_front_end_settings_and_seed():
    """Construction (no GPU): augment reads spec_augment / noise_prob from audio_conf; seed=None draws from numpy's global state."""
    from asr_amd.data import GpuSpectrogramFrontEnd
    fe = GpuSpectrogramFrontEnd(conf(spec_augment=True), normalize=True, augment=True, seed=5)
    assert fe.spec_augment and fe.noise is None and fe.noise_prob == 0.0 and fe.seed == 5
    a = fe.draw([16000, 8000])
    b = GpuSpectrogramFrontEnd(conf(spec_augment=True), normalize=True, augment=True, seed=5).draw([16000, 8000])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    np.random.seed(123)
    s1 = GpuSpectrogramFrontEnd(conf(spec_augment=True), augment=True).seed
    np.random.seed(123)
    assert GpuSpectrogramFrontEnd(conf(spec_augment=True), augment=True).seed == s1 == np.random.RandomState(123).randint(0, 2 ** 31 - 1)
    st = np.random.get_state()[1].copy()
    GpuSpectrogramFrontEnd(conf(), augment=True)                                # nothing to draw: the global state is not consumed
    assert np.array_equal(np.random.get_state()[1], st)
    assert not GpuSpectrogramFrontEnd(conf(spec_augment=True)).augment            # default: the plain front-end
    with pytest.raises(ValueError):
        GpuSpectrogramFrontEnd(conf(), augment=True, freq_masks=9)


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


def test_front_end_host_is_unchanged_and_still_warns(tmp_path):
    from asr_amd.data import AudioDataLoader, SpectrogramDataset, get_loader
    manifest, labels = _wav_corpus(tmp_path, [8000, 4000])
    c = conf(noise_dir=str(tmp_path), speed_volume_perturb=True, spec_augment=True)
    with pytest.warns(UserWarning) as rec:
        loader, _ = get_loader(c, labels, manifest, batch_size=2, num_workers=0, front_end="host")
    msgs = [str(w.message) for w in rec]
    assert ("asr_amd.data.SpectrogramDataset: augmentation(s) requested by audio_conf but not implemented here, ignored: "
            "noise_dir, speed_volume_perturb, spec_augment") in msgs
    assert isinstance(loader, AudioDataLoader) and isinstance(loader.dataset, SpectrogramDataset)
    with pytest.raises(ValueError):
        get_loader(conf(), labels, manifest, batch_size=2, num_workers=0, front_end="cpu")


def test_front_end_gpu_dataset_reads_waveforms(tmp_path):
    """front_end="gpu" builds the waveform dataset (no GPU touched before the first batch): items are (waveform, ids); .npy / .pt
    manifest entries are refused naming the file; speed_volume_perturb still warns, with the GPU path's text."""
    import pandas as pd
    from asr_amd.data import GpuAudioDataLoader, LengthBucketingSampler, WaveformDataset, get_loader
    manifest, labels = _wav_corpus(tmp_path, [8000, 4000, 12000])
    loader, sampler = get_loader(conf(), labels, manifest, batch_size=2, num_workers=0, front_end="gpu", length_bucketing=True)
    assert isinstance(loader, GpuAudioDataLoader) and isinstance(loader.dataset, WaveformDataset)
    assert isinstance(sampler, LengthBucketingSampler) and len(loader) == 2
    w, ids = loader.dataset[0]
    assert w.dtype == torch.float32 and w.shape == (8000,) and ids == [1]
    with pytest.warns(UserWarning, match="speed_volume_perturb is not implemented.*separate issue"):
        get_loader(conf(speed_volume_perturb=True), labels, manifest, batch_size=2, num_workers=0, front_end="gpu")
    df = pd.read_csv(manifest)
    df.loc[1, "audio_filepath"] = str(tmp_path / "spec.npy")
    df.to_csv(tmp_path / "m2.csv", index=False)
    with pytest.raises(ValueError, match="spec.npy"):
        get_loader(conf(), labels, str(tmp_path / "m2.csv"), batch_size=2, num_workers=0, front_end="gpu")
