"""-m gpu: the tempo / gain perturbation (ds2_tempo_gain_f32: a chain kernel for the WSOLA searches, a synthesis kernel for cross-fade,
gain and clip) against the fp64 / integer contract of tests/tempo_oracle.py — every search offset to the integer —, its exact properties,
the front-end with all three augmentations against the chained oracles, and get_loader(front_end="gpu", perturb=True) end to end.
Parity with sox's `tempo` effect itself is unpinned (no sox here); the contract in include/ds2hip.h is what is held."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_oracle as A
import det
import tempo_oracle as T

pytestmark = pytest.mark.gpu

LENS = [16000, 8000, 4321, 777, 250, 0]
TEMPO = [0.85, 1.15, 0.93, 1.07, 1.0, 1.1]
GAIN_DB = [-6.0, 8.0, 0.0, 3.0, -2.0, 5.0]                   # utterance 1 (peaks near 0.47) clips at +8 dB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def conf(**kw):
    c = dict(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def linear_gain(db):
    return np.float32(10.0 ** (np.asarray(db, dtype=np.float64) / 20.0))


def ragged_batch(grid, garbage=7.5):
    """The ragged batch of the spectrogram tests plus an empty utterance: garbage beyond each length, odd row pitch.  `grid`: samples on
    the 16-bit grid (what a WAV file gives) or plain fp32 values between its levels."""
    t = np.arange(16000) / 16000.0
    waves = [(0.3 * np.sin(2 * np.pi * (200.0 + 150 * i) * t[:n]) + 0.1 * det.unitvar((n,), 70 + i)).astype(np.float32)
             for i, n in enumerate(LENS)]
    if grid:
        waves = [(np.rint(w * 32768) / 32768).astype(np.float32) for w in waves]
    batch = np.full((len(LENS), 16000 + 37), garbage, dtype=np.float32)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = w
    return waves, batch


def check_against_oracle(waves, tempo, gain_db, out, n_out, offsets):
    """Offsets equal to the integer — all of them —, lengths equal, samples within 1e-6 G max|x| (at most six fp32 roundings of 2^-24
    relative on magnitudes up to 2 max|x|: 7.2e-7), exact zeros beyond n_out, clipped samples exactly +-1."""
    out, n_out, offsets = out.cpu().numpy(), n_out.cpu().numpy(), offsets.cpu().numpy()
    G = linear_gain(gain_db)
    clipped = 0
    for b, w in enumerate(waves):
        y, d = T.tempo_gain(w, tempo[b], G[b])
        assert n_out[b] == len(y) == T.out_samples(len(w), tempo[b])
        mism = np.flatnonzero(offsets[b, :len(d)] != d)
        print(f"utt {b}: n {len(w)} f {tempo[b]:.4f} K {len(d)} offset mismatches {len(mism)}")
        assert len(mism) == 0, (b, mism[:8], offsets[b, mism[:8]], d[mism[:8]])
        assert (offsets[b, len(d):] == 0).all()
        assert (out[b, len(y):] == 0).all()
        if len(y):
            err = np.abs(out[b, :len(y)] - y).max()
            bound = 1e-6 * float(G[b]) * float(np.abs(w).max())
            print(f"        max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (b, err, bound)
            sat = np.abs(y) == 1.0
            assert (out[b, :len(y)][sat] == y[sat]).all()
            clipped += int(sat.sum())
    return clipped


@pytest.mark.parametrize("grid", [True, False], ids=["wav_grid", "fp32_between_levels"])
def test_tempo_gain_vs_oracle(dev, grid):
    from asr_amd import ops
    waves, batch = ragged_batch(grid)
    out, n_out, offsets = ops.tempo_gain(torch.from_numpy(batch).to(dev), LENS, TEMPO, GAIN_DB, 16000)
    assert out.shape == (6, max(T.out_samples(n, f) for n, f in zip(LENS, TEMPO))) and n_out.dtype == offsets.dtype == torch.int32
    assert offsets.shape == (6, -(-out.size(1) // 1120))
    assert check_against_oracle(waves, TEMPO, GAIN_DB, out, n_out, offsets) > 0            # something did clip
    assert bool((offsets > 0).any())


def test_tempo_gain_exact_properties(dev):
    from asr_amd import ops
    waves, batch = ragged_batch(True)
    x = torch.from_numpy(batch).to(dev)
    # tempo 1, 0 dB: the input, bit for bit
    same, n_out, offsets = ops.tempo_gain(x, LENS, [1.0] * 6, [0.0] * 6, 16000)
    assert n_out.tolist() == LENS and int(offsets.abs().max()) == 0
    got = same.cpu().numpy()
    for b, w in enumerate(waves):
        assert np.array_equal(got[b, :len(w)].view(np.int32), w.view(np.int32)) and (got[b, len(w):] == 0).all()
    # reruns are bit-identical; garbage beyond n has no effect
    a = ops.tempo_gain(x, LENS, TEMPO, GAIN_DB, 16000)
    b = ops.tempo_gain(x, LENS, TEMPO, GAIN_DB, 16000)
    c = ops.tempo_gain(torch.from_numpy(ragged_batch(True, garbage=-0.123)[1]).to(dev), LENS, TEMPO, GAIN_DB, 16000)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    # a wider row pitch changes nothing but the zero padding
    wide = torch.full((6, 20011), 3.0, device=dev)
    wide[:, :batch.shape[1]] = x
    for u, v in zip(a, ops.tempo_gain(wide, LENS, TEMPO, GAIN_DB, 16000)):
        assert torch.equal(u, v)


def test_tempo_gain_rejects_arguments_outside_the_contract(dev):
    from asr_amd import _lib, ops
    x = torch.zeros(2, 1000, device=dev)
    for kw in (dict(tempo=[0.4, 1.0]), dict(tempo=[1.0, 2.5]), dict(tempo=[float("nan"), 1.0])):
        with pytest.raises(_lib.DS2LibraryError):
            ops.tempo_gain(x, [1000, 500], kw["tempo"], [0.0, 0.0], 16000)
    with pytest.raises(_lib.DS2LibraryError):
        ops.tempo_gain(x, [1000, 500], [1.0, 1.0], [0.0, 0.0], 16000, segment_ms=20.0)        # S <= 2 O
    with pytest.raises(AssertionError):
        ops.tempo_gain(x, [1001, 500], [1.0, 1.0], [0.0, 0.0], 16000)


def test_tempo_gain_full_size_offsets(dev):
    """B = 64 x 10 s of 16-bit-grid waveforms at mixed tempos, the full-size shape of the chain (K = 125 .. 169): every offset equal."""
    from asr_amd import ops
    B, n = 64, 160000
    t = np.arange(n) / 16000.0
    waves = []
    for i in range(B):
        w = 0.25 * np.sin(2 * np.pi * (110.0 + 13 * i) * t) + 0.15 * np.sin(2 * np.pi * (700.0 + 31 * i) * t + i) + 0.05 * det.unitvar((n,), 500 + i)
        waves.append((np.rint(w[:n - 160 * (i % 5)] * 32768) / 32768).astype(np.float32))
    tempo = np.linspace(0.85, 1.15, B)[np.argsort(det.unitvar((B,), 9))]
    gain = np.linspace(-6, 8, B)
    batch = torch.from_numpy(np.stack([np.pad(w, (0, n - len(w))) for w in waves])).to(dev)
    out, n_out, offsets = ops.tempo_gain(batch, [len(w) for w in waves], tempo, gain, 16000)
    assert offsets.size(1) == max(-(-T.out_samples(len(w), f) // 1120) for w, f in zip(waves, tempo)) >= 168
    check_against_oracle(waves, tempo, gain, out, n_out, offsets)


def _noise_dir(tmp_path):
    from scipy.io import wavfile
    (tmp_path / "noise").mkdir()
    for i, m in enumerate((20000, 3000)):
        wavfile.write(str(tmp_path / "noise" / f"n{i}.wav"), 16000, (det.unitvar((m,), 300 + i) * 6000).astype(np.int16))
    return str(tmp_path / "noise")


@pytest.mark.parametrize("normalize", [False, True])
def test_front_end_with_all_three_augmentations_vs_oracles(dev, tmp_path, normalize):
    """GpuSpectrogramFrontEnd(augment=True, speed_volume_perturb=True) = tempo oracle -> augmented-spectrogram oracle fed the same draws
    (one block of tempo / gain draws, then the noise and mask draws on the PERTURBED lengths), at the augmented front-end's tolerance."""
    from asr_amd.data import GpuSpectrogramFrontEnd, NoiseInjection
    waves = ragged_batch(True)[0][:5]
    lens = LENS[:5]
    ni = NoiseInjection(_noise_dir(tmp_path), 16000, (0.1, 0.5))
    c = conf(noise_dir="unused", noise_prob=0.7, noise_levels=(0.1, 0.5), spec_augment=True, speed_volume_perturb=True)
    fe = GpuSpectrogramFrontEnd(c, normalize=normalize, device=dev, augment=True, seed=21, noise=ni, speed_volume_perturb=True)
    assert fe.perturb
    spect, pct = fe(waves)
    rng = np.random.default_rng(21)
    tempo, gain = np.zeros(5), np.zeros(5)
    for b in range(5):
        tempo[b], gain[b] = rng.uniform(0.85, 1.15), rng.uniform(-6, 8)
    ys = [T.tempo_gain(w, f, g)[0] for w, f, g in zip(waves, tempo, linear_gain(gain))]
    n_out = [len(y) for y in ys]
    assert n_out != lens
    dr = A.draws(rng, n_out, 160, 161, n_files=len(ni), noise_prob=0.7, levels=(0.1, 0.5), spec_augment=True)
    assert any(d["file"] is not None for d in dr)
    files = [ni.samples[int(s):int(s) + int(L)] for s, L in zip(ni.starts, ni.lengths)]
    ref, frames = A.augmented_spectrogram(ys, files, [float(np.float32(d["level"])) for d in dr], [d["u"] for d in dr],
                                          [d["file"] for d in dr], [d["freq"] for d in dr], [d["time"] for d in dr], 320, 160, "hamming",
                                          "constant", normalize)
    assert frames == [1 + n // 160 for n in n_out] and spect.shape == ref.shape
    assert torch.equal(pct, torch.tensor(frames, dtype=torch.float32) / float(ref.shape[3]))
    err = np.abs(spect.cpu().numpy() - ref).max()
    print(f"normalize {normalize}: max abs err {err:.3e}")
    assert err < 2e-5 * (10.0 if normalize else 1.0), err
    # an already drawn pair gives the same batch as drawing it here
    fe2 = GpuSpectrogramFrontEnd(c, normalize=normalize, device=dev, augment=True, seed=21, noise=ni, speed_volume_perturb=True)
    again, pct2 = fe2(waves, perturb=fe2.draw_perturbation(5))
    assert torch.equal(again, spect) and torch.equal(pct, pct2)
    with pytest.raises(ValueError):
        GpuSpectrogramFrontEnd(c, normalize=normalize, device=dev, augment=True, seed=21, noise=ni)(waves, perturb=(tempo, gain))


def _corpus(tmp_path, n=11, sr=16000):
    import pandas as pd
    from scipy.io import wavfile
    from asr_amd.data import write_manifest
    rng = np.random.default_rng(9)
    rows = []
    for i in range(n):
        m = int(rng.integers(6000, 24000))
        wavfile.write(str(tmp_path / f"u{i:02d}.wav"), sr, (np.sin(np.arange(m) * (0.01 + 0.003 * i)) * 8000 + rng.standard_normal(m) * 500).astype(np.int16))
        rows.append((str(tmp_path / f"u{i:02d}.wav"), m / sr, sr, "".join(rng.choice(list("abcd"), size=int(rng.integers(2, 6))))))
    write_manifest(rows, str(tmp_path / "manifest.csv"))
    pd.DataFrame({"label": ["_", "a", "b", "c", "d"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def test_loader_with_perturbation(dev, tmp_path):
    """get_loader(front_end="gpu", perturb=True): no warning, batches sorted by the PERTURBED frame count with input_percentages from
    n_out, targets following the sort, two epochs differ, a fixed seed repeats, and one DeepSpeechTrainer.fit step gives a finite loss."""
    from test_gpu_model import make_model
    from asr_amd import CTCLoss
    from asr_amd.data import get_loader
    from asr_amd.trainers import DeepSpeechTrainer
    manifest, labels = _corpus(tmp_path)
    c = conf(speed_volume_perturb=True, spec_augment=True)

    def make():
        np.random.seed(4)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            return get_loader(c, labels, manifest, batch_size=4, num_workers=0, front_end="gpu", perturb=True, caching=True)[0]
    loader = make()
    assert loader.front_end.perturb and loader.front_end.seed is not None
    raw = list(loader.loader)
    e1 = [loader.collate(r) for r in raw]
    e2 = [loader.collate(r) for r in raw]                                          # the same items again: drawn anew
    rng = np.random.default_rng(loader.front_end.seed)
    for r, (x, tg, pct, tsz) in zip(raw, e1):
        tempo = np.array([(rng.uniform(0.85, 1.15), rng.uniform(-6, 8)) for _ in r])[:, 0]
        n_out = [T.out_samples(len(w), f) for (w, _), f in zip(r, tempo)]
        order = sorted(range(len(r)), key=lambda i: 1 + n_out[i] // 160, reverse=True)
        frames = [1 + n_out[i] // 160 for i in order]
        A.draws(rng, [n_out[i] for i in order], 160, 161, spec_augment=True)       # the mask draws that follow, on the perturbed lengths
        assert x.is_cuda and x.shape == (len(r), 1, 161, frames[0]) and bool(torch.isfinite(x).all())
        assert torch.equal(pct, torch.tensor(frames, dtype=torch.float32) / float(frames[0]))
        assert torch.equal(tg, torch.tensor([ch for i in order for ch in r[i][1]], dtype=torch.int32))
        assert tsz.tolist() == [len(r[i][1]) for i in order]
    assert any(a[0].shape != b[0].shape or not torch.equal(a[0], b[0]) for a, b in zip(e1, e2))
    assert any(a[0].shape != b[0].shape for a, b in zip(e1, e2))                     # the lengths themselves are redrawn
    again = make()
    for a, r in zip(e1, raw):                                                      # the same seed: the same batches, bit for bit
        b = again.collate(r)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    torch.manual_seed(0)
    model = make_model(dict(rnn="gru", hidden=32, layers=2, classes=5))
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, torch.optim.AdamW(model.parameters(), lr=1e-3), None, None, "cuda",
                           "cuda", False, None)
    valid, loss, loss_value = tr.fit(e1[0])
    assert valid and np.isfinite(loss_value) and bool(torch.isfinite(loss))
