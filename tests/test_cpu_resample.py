"""Sample-rate conversion, host side (no GPU needed): the oracle (tests/resample_oracle.py) against scipy.signal.resample_poly, the quality
of the default filter, asr_amd.data.resample_waveform and ops.resample_taps against the oracle, ds2_resample_out_samples, the rates through
pack_waveforms, `resample=True` through WaveformDataset / NoiseInjection / SpectrogramDataset / get_loader, and the C ABI declarations."""
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resample_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000)]


def conf(**kw):
    c = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def pcm(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 9000).clip(-32768, 32767).astype(np.int16)


def test_default_filter_sizes():
    assert [2 * R.ratio(fs, ft)[3] for fs, ft in PAIRS] == [204, 188, 94, 68]
    assert [R.ratio(fs, ft)[:2] for fs, ft in PAIRS] == [(1, 3), (160, 441), (320, 441), (2, 1)]
    assert max(R.taps(fs, ft).size for fs, ft in PAIRS) == 320 * 94


@pytest.mark.parametrize("fs,ft", [(48000, 16000), (8000, 16000), (44100, 16000)], ids=["L1", "L2", "L160"])
def test_oracle_vs_scipy_resample_poly(fs, ft):
    """resample_poly(x, L, M, window=h) with the same full filter: scipy multiplies the filter it is given by `up`, so it is handed h / L;
    it centres an odd-length filter on its middle tap, which is tau = 0 of `full_filter`.  With the fp32-rounded taps the two are the same
    sum in another order (fp64 rounding only); with the unrounded filter they differ by the rounding of the taps, at most 2^-24 A[m]."""
    from scipy.signal import resample_poly
    L, M, _, J = R.ratio(fs, ft)
    x = np.random.default_rng(3).standard_normal(1500)
    y, A = R.resample(x, fs, ft)
    assert len(y) == -(-1500 * L // M)
    ref = resample_poly(x, L, M, window=R.full_filter(fs, ft) / L)
    assert ref.shape == y.shape
    print("oracle vs scipy, rounded taps:", np.abs(ref - y).max())
    assert np.abs(ref - y).max() <= 1e-13 * A.max()
    exact = resample_poly(x, L, M, window=R.full_filter(fs, ft, rounded=False) / L)
    print("oracle vs scipy, fp64 taps:", np.abs(exact - y).max())
    assert (np.abs(exact - y) <= 2.0 ** -24 * A + 1e-13 * A.max()).all()
    assert np.abs(exact - y).max() > 0                   # (the rounding of the taps is there)


def _tone(fs, f, n=3000):
    return np.sin(2 * np.pi * f * np.arange(n) / fs)


@pytest.mark.parametrize("fs,ft", PAIRS)
def test_default_filter_quality(fs, ft):
    """On the oracle, the middle half of a 3000-sample tone.  Pass band: 1 kHz and 0.85 x the lower Nyquist frequency come out as the
    same tone at the new rate, error <= 2e-5.  Stop band: 1.06 x and 1.3 x the lower Nyquist frequency come out at <= -95 dB — going down,
    the whole output (the tone has no place at the new rate); going up, the samples ARE those of the tone's alias below the source
    Nyquist frequency, and what must be gone is its image at the tone's own frequency, whose amplitude a joint least-squares fit of the
    two sinusoids gives."""
    nyq = min(fs, ft) / 2.0
    floor = 10.0 ** (-95.0 / 20.0)
    for f in (1000.0, 0.85 * nyq):
        y, _ = R.resample(_tone(fs, f), fs, ft)
        m = np.arange(len(y))[len(y) // 4: len(y) - len(y) // 4]
        err = np.abs(y[m] - np.sin(2 * np.pi * f * m / ft)).max()
        print(fs, ft, "pass", f, err)
        assert err <= 2e-5
    for f in (1.06 * nyq, 1.3 * nyq):
        y, _ = R.resample(_tone(fs, f), fs, ft)
        m = np.arange(len(y))[len(y) // 4: len(y) - len(y) // 4]
        if fs > ft:
            level = np.abs(y[m]).max()
        else:
            basis = np.stack([np.sin(2 * np.pi * f * m / ft), np.cos(2 * np.pi * f * m / ft),
                              np.sin(2 * np.pi * (fs - f) * m / ft), np.cos(2 * np.pi * (fs - f) * m / ft)], axis=1)
            c = np.linalg.lstsq(basis, y[m], rcond=None)[0]
            level = float(np.hypot(c[0], c[1]))
            assert np.hypot(c[2], c[3]) > 0.1            # (the alias itself, a tone inside the pass or transition band, is there)
        print(fs, ft, "stop", f, 20 * np.log10(max(level, 1e-300)))
        assert level <= floor


def test_resample_taps_match_the_oracle():
    from asr_amd import ops
    for fs, ft in PAIRS + [(32000, 16000), (16000, 8000), (16000, 48000)]:
        tab = ops.resample_taps(fs, ft)
        L, M, _, J = R.ratio(fs, ft)
        assert tab.dtype == np.float32 and tab.shape == (L, 2 * J) and ops.resample_ratio(fs, ft) == (L, M, J)
        assert np.array_equal(tab.astype(np.float64), R.taps(fs, ft))
        assert ops.resample_taps(fs, ft) is tab          # cached
    assert ops.resample_ratio(16000, 16000) == (1, 1, 0)
    for fs, ft in ((16001, 16000), (16000, 1999), (2000, 16001), (0, 16000), (16000, -1)):
        with pytest.raises(ValueError):
            ops.resample_ratio(fs, ft)
    with pytest.raises(ValueError):
        ops.resample_taps(16000, 16000)


@pytest.mark.parametrize("fs,ft", PAIRS + [(16000, 16000)])
def test_resample_waveform_vs_oracle(fs, ft):
    from asr_amd.data import resample_waveform
    rng = np.random.default_rng(fs)
    for n in (4801, 777, 5, 1, 0):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        got = resample_waveform(x, fs, ft)
        y, A = R.resample(x, fs, ft)
        assert got.dtype == np.float32 and got.shape == y.shape == (R.out_samples(n, fs, ft),)
        if fs == ft:
            assert np.array_equal(got.view(np.int32), x.view(np.int32))
        else:
            assert (np.abs(got.astype(np.float64) - y) <= 2.0 ** -23 * np.maximum(np.abs(y), A)).all()
    if fs != ft:
        assert np.abs(resample_waveform(rng.uniform(-1, 1, 500).astype(np.float32), fs, ft)).max() > 0.1
    with pytest.raises(ValueError):
        resample_waveform(np.zeros(10, np.float32), 16001, 16000)


def test_out_samples_host_function():
    from asr_amd import _lib, ops
    lib = _lib.load()
    for n in (0, 1, 2, 7, 441, 48000, 2 ** 29):
        for fs, ft in PAIRS + [(16000, 16000), (16000, 48000)]:
            L, M, _, _ = R.ratio(fs, ft)
            want = -(-n * L // M)                        # ceil(n L / M) in Python's integers
            assert lib.ds2_resample_out_samples(n, L, M) == want == ops.resample_out_samples(n, fs, ft) == R.out_samples(n, fs, ft)
    assert lib.ds2_resample_out_samples(-1, 1, 3) == -1 and lib.ds2_resample_out_samples(5, 0, 3) == -1
    assert lib.ds2_resample_out_samples(5, 1, 0) == -1 and lib.ds2_resample_out_samples(2 ** 31 + 1, 1, 1) == -1
    assert lib.ds2_resample_tile_samples() >= 64


def test_pack_waveforms_carries_the_rates():
    from asr_amd.data import pack_waveforms
    items = [(pcm(13, 0), [1]), (pcm(0, 1), []), (pcm(250, 2), [2, 3])]
    plain = pack_waveforms(items)
    assert len(plain) == 4                               # unchanged for items without a rate
    rated = pack_waveforms([(w, r, t) for (w, t), r in zip(items, (48000, 16000, 44100))])
    assert len(rated) == 5 and rated[4].dtype == np.int64 and rated[4].tolist() == [48000, 16000, 44100]
    assert torch.equal(rated[0], plain[0]) and rated[1].tolist() == plain[1].tolist() and rated[2].tolist() == plain[2].tolist()
    assert rated[3] == plain[3] == [[1], [], [2, 3]]
    with pytest.raises(ValueError):
        pack_waveforms([items[0], (pcm(5, 3), 16000, [])])


RATES = (48000, 44100, 22050, 8000, 16000, 48000)
LENS = (9000, 7001, 3000, 2500, 4000, 1234)


def _mixed_rate_corpus(tmp_path, rates=RATES):
    import pandas as pd
    from scipy.io import wavfile
    rows = []
    for i, (sr, n) in enumerate(zip(rates, LENS)):
        y = np.stack([pcm(n, i), pcm(n, 50 + i)], axis=1) if i == 2 else pcm(n, i)          # one stereo file: the float32 path
        wavfile.write(str(tmp_path / f"u{i}.wav"), sr, y)
        rows.append((str(tmp_path / f"u{i}.wav"), n / sr, 16000, "abc"[: 1 + i % 3]))         # (the fq column lies: it is not trusted)
    pd.DataFrame.from_records(rows, columns=["audio_filepath", "duration", "fq", "text"]).to_csv(tmp_path / "manifest.csv", index=False)
    pd.DataFrame({"label": ["_", "a", "b", "c"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def test_waveform_dataset_with_resample(tmp_path):
    from asr_amd.data import WaveformDataset, _read_wav, pack_waveforms
    manifest, labels = _mixed_rate_corpus(tmp_path)
    ds = WaveformDataset(conf(), manifest, labels, resample=True)
    raw = ds.raw_items()
    for i, (sr, n) in enumerate(zip(RATES, LENS)):
        samples, rate, ids = raw[i]
        assert rate == sr and len(samples) == n and samples.dtype == (np.float32 if i == 2 else np.int16) and ids == ds[i][1]
        w = ds[i][0].numpy()                             # the float32 item: converted on the host
        y, A = R.resample(_read_wav(str(tmp_path / f"u{i}.wav"))[1], sr, 16000)
        assert len(w) == R.out_samples(n, sr, 16000)
        assert (np.abs(w.astype(np.float64) - y) <= 2.0 ** -23 * np.maximum(np.abs(y), A)).all()
    buf, off, ln, tr, rates = pack_waveforms([raw[i] for i in range(6)])
    assert rates.tolist() == list(RATES) and ln.tolist() == list(LENS) and buf.dtype == torch.float32
    # the default still raises the old message
    with pytest.raises(ValueError, match="48000 Hz, expected 16000 Hz audio"):
        WaveformDataset(conf(), manifest, labels).raw_items()[0]
    with pytest.raises(ValueError, match="48000 Hz, expected 16000 Hz audio"):
        WaveformDataset(conf(), manifest, labels)[0]
    # an unsupported pair
    manifest2, labels2 = _mixed_rate_corpus(tmp_path, rates=(16001,) + RATES[1:])
    bad = WaveformDataset(conf(), manifest2, labels2, resample=True)
    with pytest.raises(ValueError, match="16001"):
        bad.raw_items()[0]
    with pytest.raises(ValueError, match="16001"):
        bad[0]


def test_noise_injection_with_resample(tmp_path):
    from scipy.io import wavfile
    from asr_amd.data import NoiseInjection, resample_waveform
    d = tmp_path / "noise"
    d.mkdir()
    files = [("a.wav", 44100, 5000), ("b.wav", 16000, 3000), ("c.wav", 8000, 1001)]
    for name, sr, n in files:
        wavfile.write(str(d / name), sr, pcm(n, len(name) + n))
    with pytest.raises(ValueError, match=r"44100 Hz, expected 16000 Hz \(no resampling here\)"):
        NoiseInjection(str(d), 16000)
    ni = NoiseInjection(str(d), 16000, resample=True)
    want = [R.out_samples(n, sr, 16000) for _, sr, n in files]
    assert ni.lengths.tolist() == want == [1815, 3000, 2002]
    assert ni.starts.tolist() == [0, 1815, 4815] and ni.samples.dtype == np.float32 and len(ni.samples) == sum(want)
    for (name, sr, n), b, m in zip(files, ni.starts, ni.lengths):
        x = wavfile.read(str(d / name))[1].astype(np.float32) / 32768.0
        assert np.array_equal(ni.samples[b:b + m], resample_waveform(x, sr, 16000))
    wavfile.write(str(d / "d.wav"), 16001, pcm(100, 9))
    with pytest.raises(ValueError, match="16001"):
        NoiseInjection(str(d), 16000, resample=True)


def test_get_loader_with_resample(tmp_path):
    """resample=True builds both loaders without touching the GPU; the GPU one packs on the host for prefetch=0 too and its batches carry
    the rates; the host one yields spectrograms of the converted waveforms."""
    import inspect
    from asr_amd import DeepSpeech
    from asr_amd.data import GpuAudioDataLoader, _stft_spectrogram, get_loader, pack_waveforms, resample_waveform, _read_wav
    manifest, labels = _mixed_rate_corpus(tmp_path)
    assert inspect.signature(get_loader).parameters["resample"].default is False
    assert inspect.signature(DeepSpeech.get_loader).parameters["resample"].default is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for prefetch in (0, 2):
            loader, _ = get_loader(conf(), labels, manifest, batch_size=3, num_workers=0, front_end="gpu", prefetch=prefetch, resample=True)
            assert isinstance(loader, GpuAudioDataLoader) and loader.resample and loader.dataset.resample
            assert loader.loader.collate_fn is pack_waveforms
            packed = list(loader.loader)
            assert len(packed) == 2 and all(len(p) == 5 for p in packed)
            assert sorted(int(r) for p in packed for r in p[4]) == sorted(RATES)
        host, _ = get_loader(conf(), labels, manifest, batch_size=6, num_workers=0, front_end="host", resample=True)
    assert get_loader(conf(), labels, manifest, batch_size=3, num_workers=0, front_end="gpu")[0].resample is False
    # the host front-end: item 0 is the spectrogram of the converted file
    spect, _ = host.dataset[0]
    y = resample_waveform(_read_wav(str(tmp_path / "u0.wav"))[1], 48000, 16000)
    ref = torch.from_numpy(_stft_spectrogram(y, 16000, 0.02, 0.01, "hamming"))
    ref = (ref - ref.mean()) / ref.std()
    assert spect.shape == ref.shape == (161, 1 + len(y) // 160) and torch.equal(spect, ref)
    (x, _, pct, _), = list(host)
    assert tuple(x.shape) == (6, 1, 161, 1 + R.out_samples(2500, 8000, 16000) // 160) and float(pct.max()) == 1.0     # the 8 kHz file is the longest
    # without the flag the host dataset still refuses the file
    plain, _ = get_loader(conf(), labels, manifest, batch_size=6, num_workers=0, front_end="host")
    with pytest.raises(AssertionError, match="expected 16000 Hz audio"):
        plain.dataset[0]


def test_resample_entry_points_are_declared_and_exported():
    from asr_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    assert re.search(r"\bint ds2_wave_resample_f32\s*\(", header) and re.search(r"\blong long ds2_resample_out_samples\s*\(", header)
    assert "UNPINNED" in header[header.index("sample-rate conversion"):header.index("ds2_wave_resample_f32(")]
    lib = _lib.load()
    for name in ("ds2_wave_resample_f32", "ds2_resample_out_samples", "ds2_resample_tile_samples"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "wave_resample_kernel" in open(os.path.join(ROOT, "asr_amd", "csrc", "resample.h")).read()
    # the C entry point refuses what it can see on the host (nothing is launched: no GPU needed)
    assert lib.ds2_wave_resample_f32(None, 0, 0, None, None, None, None, None, None, None, None, 0, 1, 8, None, 8, None) != 0
    assert b"null pointer" in lib.ds2_last_error()
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.wave_resample(torch.zeros(8, dtype=torch.int16), [0], [8], [48000])
