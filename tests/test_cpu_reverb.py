"""Reverberation, host side (no GPU needed): the oracle (tests/reverb_oracle.py) against numpy / scipy convolution, the rules of the
impulse-response bank (asr_amd.data.ImpulseResponses) on WAV files, the synthetic bank, draw_reverb and the front-end's draw order, the
host loader's warning and the C ABI declarations."""
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import reverb_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conf(**kw):
    c = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def write_wav(path, samples, sr=16000):
    from scipy.io import wavfile
    wavfile.write(str(path), sr, np.asarray(samples))


def test_oracle_vs_numpy_and_scipy():
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(1)
    for n, P in [(1, 1), (5, 9), (300, 1), (300, 17), (1000, 257), (64, 200)]:
        x, h = rng.standard_normal(n), rng.standard_normal(P)
        y, A = V.reverb(x, h)
        assert y.shape == A.shape == (n,)
        assert np.abs(y - V.reverb_direct(x, h)).max() <= 1e-13 * A.max()
        assert np.abs(y - np.convolve(x, h)[:n]).max() <= 1e-13 * A.max()
        assert np.abs(y - fftconvolve(x, h)[:n]).max() <= 1e-12 * A.max()
        assert (np.abs(y) <= A * (1 + 1e-12)).all()
        assert y[0] == h[0] * x[0] and A[0] == abs(h[0]) * abs(x[0])
    y, A = V.reverb(np.arange(4.0), [])                  # no taps: the utterance itself
    assert np.array_equal(y, np.arange(4.0)) and np.array_equal(A, np.arange(4.0))
    assert V.reverb([], [1.0])[0].shape == (0,)


def test_bank_peak_tail_cut_cap_and_unit_energy(tmp_path):
    """The peak rule with a tie, the tail cut at exactly the sample where the energy rule flips (energies that are powers of two, and a
    threshold a hair on either side of one of them), the max_seconds cap, and unit energy."""
    from asr_amd.data import ImpulseResponses
    # a: |h| peaks at 2 and 4 (a tie, opposite signs): the samples before index 2 go.  Kept: [-0.5, 0.25, 0.5, 2^-3, 2^-6, 2^-7, 0, 0]
    a = np.array([0.125, 0.25, -0.5, 0.25, 0.5, 2.0 ** -3, 2.0 ** -6, 2.0 ** -7, 0.0, 0.0])
    # b: energies 1, 2^-2, 2^-10, 2^-10: with tail_db = 10 log10(2^-10 / total') the rule flips exactly at a cut
    b = np.array([1.0, 0.5, 2.0 ** -5, 2.0 ** -5])
    c = np.concatenate([[0.0, 1.0], 0.5 * np.ones(30)])    # no decay: only the cap cuts it
    for name, h in (("a", a), ("b", b), ("c", c)):
        write_wav(tmp_path / f"{name}.wav", h.astype(np.float32))
    bank = ImpulseResponses(str(tmp_path), max_seconds=10 / 16000)
    assert len(bank) == 3 and [os.path.basename(p) for p in bank.paths] == ["a.wav", "b.wav", "c.wav"]
    assert bank.taps.dtype == np.float32 and bank.starts.tolist() == [0] + np.cumsum(bank.lengths)[:-1].tolist()
    got = [bank.taps[s:s + n].astype(np.float64) for s, n in zip(bank.starts, bank.lengths)]
    for h, g in zip((a, b, c), got):
        want = V.prepare(h, max_seconds=10 / 16000)
        assert np.array_equal(g, want)
        exact = V.prepare(h, max_seconds=10 / 16000, rounded=False)
        assert abs((exact * exact).sum() - 1.0) <= 1e-12                           # unit energy before the fp32 rounding
    assert bank.lengths[0] == 6 and got[0][0] < 0 and abs(got[0][0]) == abs(got[0][2])      # starts at the FIRST peak; -60 dB drops the zeros only
    assert bank.lengths[2] == 10                                                        # the cap: int(max_seconds * sample_rate)
    # the flip: total = 1 + 2^-2 + 2^-9; the tail after 3 taps holds 2^-10, after 2 taps 2^-9
    total = 1.0 + 0.25 + 2.0 ** -9
    at = 10.0 * np.log10(2.0 ** -10 / total)
    for tail_db, P in ((at + 1e-9, 3), (at - 1e-6, 4), (10.0 * np.log10(2.0 ** -9 / total) + 1e-9, 2)):
        only_b = tmp_path / f"b{P}"
        only_b.mkdir()
        write_wav(only_b / "b.wav", b.astype(np.float32))
        assert ImpulseResponses(str(only_b), tail_db=tail_db).lengths.tolist() == [P] == [len(V.prepare(b, tail_db=tail_db))]


def test_bank_channels_rates_and_errors(tmp_path):
    from asr_amd.data import ImpulseResponses, resample_waveform
    rng = np.random.default_rng(4)
    h0 = (rng.standard_normal(40) * np.exp(-np.arange(40) / 6.0) * 8000).astype(np.int16)
    h0[0] = 20000
    h1 = (rng.standard_normal(40) * 3000).astype(np.int16)
    stereo = tmp_path / "stereo"
    stereo.mkdir()
    write_wav(stereo / "s.wav", np.stack([h0, h1], axis=1))
    bank = ImpulseResponses(str(stereo))
    assert np.array_equal(bank.taps.astype(np.float64), V.prepare(h0.astype(np.float64) / 32768.0))      # channel 0, not the mean
    off = tmp_path / "off"
    (off / "deep").mkdir(parents=True)
    write_wav(off / "deep" / "h.wav", h0, sr=48000)
    with pytest.raises(ValueError, match="48000 Hz"):
        ImpulseResponses(str(off))
    bank = ImpulseResponses(str(off), resample=True)                                  # found recursively, converted once
    want = V.prepare(resample_waveform(h0.astype(np.float32) / 32768.0, 48000, 16000))
    assert np.array_equal(bank.taps.astype(np.float64), want) and bank.sample_rate == 16000
    zero = tmp_path / "zero"
    zero.mkdir()
    write_wav(zero / "z.wav", np.zeros(16, np.int16))
    with pytest.raises(ValueError, match="non-zero"):
        ImpulseResponses(str(zero))
    with pytest.raises(IOError):
        ImpulseResponses(str(tmp_path / "missing"))
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no .wav"):
        ImpulseResponses(str(empty))


def test_synthetic_bank():
    from asr_amd.data import ImpulseResponses
    kw = dict(t60_range=(0.05, 0.1), max_seconds=0.05)
    a = ImpulseResponses.synthetic(3, seed=7, **kw)
    b = ImpulseResponses.synthetic(3, seed=7, **kw)
    c = ImpulseResponses.synthetic(3, seed=8, **kw)
    assert len(a) == 3 and np.array_equal(a.taps, b.taps) and np.array_equal(a.lengths, b.lengths)
    assert not (a.taps.shape == c.taps.shape and np.array_equal(a.taps, c.taps))
    want = V.synthetic(3, seed=7, **kw)
    assert a.lengths.tolist() == [len(h) for h in want] and (a.lengths <= 800).all() and (a.lengths > 100).all()
    assert np.array_equal(a.taps.astype(np.float64), np.concatenate(want))
    for s, n in zip(a.starts, a.lengths):
        h = a.taps[s:s + n].astype(np.float64)
        assert abs((h * h).sum() - 1.0) < 1e-6 and np.argmax(np.abs(h)) == 0          # unit energy, the direct path at lag 0
    assert a.device_taps("cpu") is a.device_taps("cpu") and a.device_taps("cpu").dtype == torch.float32
    with pytest.raises(TypeError):
        ImpulseResponses.synthetic(1, bogus=1)


def test_draw_reverb_matches_the_oracle():
    from asr_amd.data import ImpulseResponses, draw_reverb
    bank = ImpulseResponses.synthetic(4, t60_range=(0.02, 0.05), max_seconds=0.02)
    for prob in (0.0, 0.3, 1.0):
        r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
        file, base, taps = draw_reverb(r1, 40, bank, prob)
        wf, wb, wt = V.draw_reverb(r2, 40, bank.starts, bank.lengths, prob)
        assert np.array_equal(file, wf) and np.array_equal(base, wb) and np.array_equal(taps, wt)
        assert base.dtype == np.int64 and taps.dtype == np.int32
        assert r1.random() == r2.random()                                             # the same number of draws
        on = file >= 0
        assert (taps[~on] == 0).all() and np.array_equal(taps[on], bank.lengths[file[on]]) and np.array_equal(base[on], bank.starts[file[on]])
    # prob 0 consumes the coins and nothing else
    r1, r2 = np.random.default_rng(2), np.random.default_rng(2)
    file, _, taps = draw_reverb(r1, 7, bank, 0.0)
    for _ in range(7):
        r2.binomial(1, 0.0)
    assert (file == -1).all() and (taps == 0).all() and r1.random() == r2.random()


def test_front_end_draw_order_and_unchanged_stream_without_a_bank():
    """Per batch: the perturbation block, the reverb block, then draw_augmentation's — a seeded Generator's stream checked at each block
    boundary.  Without a bank the parameters are those of a front-end built without the feature."""
    from asr_amd.data import GpuSpectrogramFrontEnd, ImpulseResponses, draw_augmentation, draw_perturbation, draw_reverb
    bank = ImpulseResponses.synthetic(3, t60_range=(0.02, 0.05), max_seconds=0.02)
    lens = [16000, 8000, 4321]
    c = conf(spec_augment=True, speed_volume_perturb=True, reverb_prob=0.7)
    fe = GpuSpectrogramFrontEnd(c, augment=True, seed=11, speed_volume_perturb=True, reverb=bank)
    assert fe.reverb is bank and fe.reverb_prob == 0.7 and fe.perturb
    rng = np.random.default_rng(11)
    tempo, gain = fe.draw_perturbation(3)
    t2, g2 = draw_perturbation(rng, 3)
    assert np.array_equal(tempo, t2) and np.array_equal(gain, g2)
    assert fe.rng.bit_generator.state == rng.bit_generator.state                      # boundary 1
    got = fe.draw_reverb(3)
    want = draw_reverb(rng, 3, bank, 0.7)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert fe.rng.bit_generator.state == rng.bit_generator.state                      # boundary 2
    n_out = fe.perturbed_lengths(lens, tempo)
    p, q = fe.draw(n_out), draw_augmentation(rng, n_out, 160, 161, None, 0.0, True, 27.0, 70.0, 1, 1)
    assert all(np.array_equal(p[k], q[k]) for k in q)
    assert fe.rng.bit_generator.state == rng.bit_generator.state                      # boundary 3
    assert GpuSpectrogramFrontEnd(conf(), augment=True, reverb=bank).reverb_prob == 0.5       # the default
    # no bank: nothing of the feature is drawn
    want = draw_augmentation(np.random.default_rng(11), lens, 160, 161, None, 0.0, True, 27.0, 70.0, 1, 1)
    for cc in (conf(spec_augment=True), conf(spec_augment=True, rir_dir=None, reverb_prob=1.0)):
        fe = GpuSpectrogramFrontEnd(cc, augment=True, seed=11)
        assert fe.reverb is None and fe.reverb_prob == 0.0
        got = fe.draw(lens)
        assert all(np.array_equal(got[k], want[k]) for k in want)
    assert GpuSpectrogramFrontEnd(conf(), reverb=bank).reverb is None                  # augment=False: the plain front-end
    # a bank is something to draw: seed=None takes the seed from numpy's global state
    np.random.seed(123)
    assert GpuSpectrogramFrontEnd(conf(), augment=True, reverb=bank).seed == np.random.RandomState(123).randint(0, 2 ** 31 - 1)
    st = np.random.get_state()[1].copy()
    GpuSpectrogramFrontEnd(conf(), augment=True)
    assert np.array_equal(np.random.get_state()[1], st)
    with pytest.raises(ValueError, match="Hz"):
        GpuSpectrogramFrontEnd(conf(sample_rate=8000), augment=True, reverb=bank)


def test_front_end_builds_the_bank_from_rir_dir(tmp_path):
    from asr_amd.data import GpuSpectrogramFrontEnd
    h = np.zeros(50, np.int16)
    h[3], h[10] = 16000, -4000
    write_wav(tmp_path / "r.wav", h)
    fe = GpuSpectrogramFrontEnd(conf(rir_dir=str(tmp_path), reverb_prob=0.25), augment=True, seed=1)
    assert len(fe.reverb) == 1 and fe.reverb_prob == 0.25 and fe.reverb.lengths.tolist() == [8]
    assert GpuSpectrogramFrontEnd(conf(rir_dir=str(tmp_path))).reverb is None         # augment=False
    write_wav(tmp_path / "r48.wav", h, sr=48000)
    with pytest.raises(ValueError, match="48000 Hz"):
        GpuSpectrogramFrontEnd(conf(rir_dir=str(tmp_path)), augment=True, seed=1)
    assert len(GpuSpectrogramFrontEnd(conf(rir_dir=str(tmp_path)), augment=True, seed=1, resample=True).reverb) == 2


def test_host_loader_warns_about_rir_dir(tmp_path):
    import pandas as pd
    from asr_amd.data import get_loader
    write_wav(tmp_path / "u.wav", (np.random.default_rng(0).standard_normal(2000) * 3000).astype(np.int16))
    write_wav(tmp_path / "rir.wav", np.array([16000, 0, 4000], np.int16))
    pd.DataFrame.from_records([(str(tmp_path / "u.wav"), 0.125, 16000, "ab")],
                              columns=["audio_filepath", "duration", "fq", "text"]).to_csv(tmp_path / "manifest.csv", index=False)
    pd.DataFrame({"label": ["_", "a", "b"]}).to_csv(tmp_path / "labels.csv", index=False)
    with pytest.warns(UserWarning, match="rir_dir"):
        get_loader(conf(rir_dir=str(tmp_path)), str(tmp_path / "labels.csv"), str(tmp_path / "manifest.csv"), batch_size=1, num_workers=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        get_loader(conf(), str(tmp_path / "labels.csv"), str(tmp_path / "manifest.csv"), batch_size=1, num_workers=0)


def test_reference_route_of_the_loader_test_is_inside_its_bar(tmp_path):
    """tests/test_gpu_reverb.py holds the loader's batch to 2e-4 against oracle-reverberated waveforms.  The reference route alone must be
    well inside that: the same corpus and responses convolved once in fp64 and once in fp32 numpy, through the host spectrogram with the
    loader's normalisation, differ by less than 2e-5 (observed: 8.4e-7)."""
    import test_gpu_reverb as G
    from asr_amd.data import ImpulseResponses, _stft_spectrogram
    G._corpus(tmp_path)
    bank = ImpulseResponses(G._rirs(tmp_path))
    assert bank.lengths.max() <= 256
    print("prepared lengths:", bank.lengths.tolist())
    worst = 0.0
    for f in range(len(bank)):
        file = np.full(6, f)
        a = G.reference_waves(tmp_path, bank, file, G.ORDER, np.float64)
        b = G.reference_waves(tmp_path, bank, file, G.ORDER, np.float32)
        for u, v in zip(a, b):
            su, sv = (torch.from_numpy(_stft_spectrogram(w, 16000, 0.02, 0.01)) for w in (u, v))
            su, sv = (su - su.mean()) / su.std(), (sv - sv.mean()) / sv.std()
            worst = max(worst, float((su - sv).abs().max()))
    print("fp64 vs fp32 reference route:", worst)
    assert worst < 2e-5


def test_reverb_entry_points_are_declared_and_exported():
    from asr_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ds2hip.h")).read()
    names = sorted(set(re.findall(r"\b(ds2_reverb_\w+)\s*\(", header)))
    assert names == ["ds2_reverb_f32", "ds2_reverb_max_taps", "ds2_reverb_tap_chunk", "ds2_reverb_tile_samples"]
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    section = header[header.index("reverberation of the waveform batch"):header.index("int ds2_reverb_f32(")]
    assert "DENORMALS" in section and "must not alias" in section
    assert "reverb_kernel" in open(os.path.join(ROOT, "asr_amd", "csrc", "reverb.h")).read()
    tile, chunk = lib.ds2_reverb_tile_samples(), lib.ds2_reverb_tap_chunk()
    assert lib.ds2_reverb_max_taps() >= 16384 and ops.reverb_max_taps() == lib.ds2_reverb_max_taps() and tile >= 16 and chunk >= 16
    assert V.MAX_TAPS == lib.ds2_reverb_max_taps()
    # the C entry point refuses what it can see on the host (nothing is launched: no GPU needed)
    assert lib.ds2_reverb_f32(None, 8, None, None, 0, None, None, 1, 8, None, 8, None) != 0
    assert b"null pointer" in lib.ds2_last_error()
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.reverb(torch.zeros(1, 8), [8], None, [0], [0])
