"""-m gpu: the augmented spectrogram front-end (ds2_spectrogram_aug_f32: noise injection fused into the pad pass, SpecAugment masks into
the last pass) against the fp64 contract of tests/augment_oracle.py, its exact properties, and get_loader(front_end="gpu") end to end."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_oracle as A
import det

pytestmark = pytest.mark.gpu

LENS = [16000, 8000, 4321, 777, 250]


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


def ragged_batch():
    """The spectrogram test's ragged batch: garbage (7.5) beyond each length, odd row pitch."""
    t = np.arange(16000) / 16000.0
    waves = [(0.3 * np.sin(2 * np.pi * (200.0 + 150 * i) * t[:n]) + 0.1 * det.unitvar((n,), 70 + i)).astype(np.float32)
             for i, n in enumerate(LENS)]
    batch = np.full((len(LENS), 16000 + 37), 7.5, dtype=np.float32)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = w
    return waves, batch


def bank():
    """Noise files: 20000 samples, 3000 (shorter than three utterances: the segment wraps), 5000 zeros (silent: unmixed)."""
    files = [(0.5 * det.unitvar((20000,), 301) - 0.25).astype(np.float32), (0.8 * det.unitvar((3000,), 302) - 0.4).astype(np.float32),
             np.zeros(5000, np.float32)]
    starts = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.int64)
    return files, starts, np.concatenate(files)


# utterance -> (file, level, u): wrap case, long file, silent file, level 0, long file near its end
PLAN = [(1, 0.4, 0.63), (0, 0.3, 0.25), (2, 0.5, 0.5), (0, 0.0, 0.1), (0, 0.2, 0.999)]
FREQ = [[(3, 20), (150, 161)], [(0, 0), (40, 41)], [(100, 127), (0, 0)], [(0, 5), (5, 9)], [(160, 161), (0, 0)]]
TIME = [[(10, 60)], [(0, 0)], [(27, 28)], [(0, 5)], [(1, 70)]]         # the last one reaches beyond the utterance's 2 frames


def call(dev, batch, pad_mode, normalize, noise=True, masks=True, levels=None):
    from asr_amd import ops
    files, starts, flat = bank()
    kw = {}
    if noise:
        lv = [p[1] for p in PLAN] if levels is None else levels
        kw = dict(noise=torch.from_numpy(flat).to(dev), noise_base=[int(starts[f]) for f, _, _ in PLAN],
                  noise_period=[len(files[f]) for f, _, _ in PLAN],
                  noise_start=[A.start_of(len(files[f]), n, u) for (f, _, u), n in zip(PLAN, LENS)], noise_level=np.array(lv, np.float32))
    if masks:
        kw.update(freq_masks=np.array(FREQ, np.int32), time_masks=np.array(TIME, np.int32))
    out, frames = ops.spectrogram_augmented(torch.from_numpy(batch).to(dev), torch.tensor(LENS), 320, 160, "hamming", pad_mode, normalize, **kw)
    return out, frames


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("normalize", [False, True])
def test_augmented_spectrogram_vs_oracle(dev, pad_mode, normalize):
    waves, batch = ragged_batch()
    files, _, _ = bank()
    out, frames = call(dev, batch, pad_mode, normalize)
    ref, frames_ref = A.augmented_spectrogram(waves, files, [float(np.float32(p[1])) for p in PLAN], [p[2] for p in PLAN],
                                              [p[0] for p in PLAN], FREQ, TIME, 320, 160, "hamming", pad_mode, normalize)
    assert frames.tolist() == frames_ref and out.shape == ref.shape
    got = out.cpu().numpy()
    tol = 2e-5 * (10.0 if normalize else 1.0)
    assert np.abs(got - ref).max() < tol, np.abs(got - ref).max()
    # the noise really went in: utterances 0 and 1 differ from the clean spectrogram far beyond the tolerance
    from oracle import stft_oracle as S
    clean, _ = S.batch_spectrogram(waves, 320, 160, "hamming", pad_mode, normalize)
    for b in (0, 1):
        assert np.abs(A.apply_masks(clean.copy(), frames_ref, FREQ, TIME)[b] - got[b]).max() > 10 * tol


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("normalize", [False, True])
def test_augmented_spectrogram_exact_properties(dev, pad_mode, normalize):
    from asr_amd import ops
    _, batch = ragged_batch()
    plain, frames = ops.spectrogram(torch.from_numpy(batch).to(dev), torch.tensor(LENS), 320, 160, "hamming", pad_mode, normalize)
    # level 0 everywhere, no masks: the bits of ds2_spectrogram_f32
    off, _ = call(dev, batch, pad_mode, normalize, masks=False, levels=[0.0] * 5)
    assert torch.equal(off, plain)
    nomask, _ = call(dev, batch, pad_mode, normalize, masks=False)
    # level 0 (utterance 3) and a silent noise file (utterance 2): those utterances keep the plain bits
    assert torch.equal(nomask[2:4], plain[2:4])
    out, _ = call(dev, batch, pad_mode, normalize)
    again, _ = call(dev, batch, pad_mode, normalize)
    assert torch.equal(out, again)                                                   # reruns are bit-identical
    o, n = out.cpu().numpy(), nomask.cpu().numpy()
    masked = np.zeros(o.shape, bool)
    for b, f in enumerate(frames.tolist()):
        for lo, hi in FREQ[b]:
            masked[b, 0, lo:hi, :f] = True
        for lo, hi in TIME[b]:
            masked[b, 0, :, lo:min(hi, f)] = True
        assert (o[b, 0, :, f:] == 0).all()                                           # padding exactly 0
    assert (o[masked] == 0).all() and masked.any()                                   # masked rectangles exactly 0
    assert np.array_equal(o[~masked], n[~masked])                                    # masks come after the statistics


def test_augmented_front_end_full_size(dev, tmp_path):
    """B = 64 x 10 s with a noise bank of three minutes (noise on every utterance): finite, (64,1,161,1001), ~0 mean / unit std per
    utterance before masking, the masked call equal to it outside its masks."""
    from scipy.io import wavfile
    from asr_amd import ops
    from asr_amd.data import GpuSpectrogramFrontEnd, NoiseInjection
    (tmp_path / "noise").mkdir()
    for i, secs in enumerate((80, 60, 40)):
        wavfile.write(str(tmp_path / "noise" / f"n{i}.wav"), 16000, (det.unitvar((16000 * secs,), 400 + i) * 8000).astype(np.int16))
    ni = NoiseInjection(str(tmp_path / "noise"), 16000, (0.1, 0.5))
    assert len(ni.samples) == 16000 * 180
    waves = [det.unitvar((160000 - 160 * (i % 5),), 90 + i) for i in range(64)]
    c = conf(noise_dir=str(tmp_path / "noise"), noise_prob=1.0, spec_augment=True, noise_levels=(0.1, 0.5))
    fe = GpuSpectrogramFrontEnd(c, normalize=True, device=dev, augment=True, seed=1)
    assert fe.noise is not None and len(fe.noise) == 3
    p = fe.draw([len(w) for w in waves])
    assert (p["level"] > 0).all()
    batch = torch.from_numpy(np.stack([np.pad(w, (0, 160000 - len(w))) for w in waves])).to(dev)
    nz = dict(noise=fe.noise.device_samples(dev), noise_base=p["base"], noise_period=p["period"], noise_start=p["start"], noise_level=p["level"])
    x, frames = ops.spectrogram_augmented(batch, torch.tensor([len(w) for w in waves]), 320, 160, "hamming", "constant", True, **nz)
    xm, _ = ops.spectrogram_augmented(batch, torch.tensor([len(w) for w in waves]), 320, 160, "hamming", "constant", True,
                                      freq_masks=p["freq"], time_masks=p["time"], **nz)
    assert x.shape == (64, 1, 161, 1001) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(xm).all())
    plain, _ = ops.spectrogram(batch, torch.tensor([len(w) for w in waves]), 320, 160, "hamming", "constant", True)
    for i in (0, 3, 63):
        f = int(frames[i])
        assert f == 1 + len(waves[i]) // 160
        v = x[i, 0, :, :f]
        assert abs(float(v.mean())) < 1e-3 and abs(float(v.std()) - 1.0) < 1e-3
        assert not torch.equal(v, plain[i, 0, :, :f])
        keep = xm[i, 0, :, :f] != 0
        assert torch.equal(xm[i, 0, :, :f][keep], v[keep]) and float(keep.float().mean()) < 1.0
    # the front-end itself: same seed, same batch -> same bits; a different seed -> different draws
    y1, _ = GpuSpectrogramFrontEnd(c, normalize=True, device=dev, augment=True, seed=1, noise=ni)(waves)
    y2, _ = GpuSpectrogramFrontEnd(c, normalize=True, device=dev, augment=True, seed=1, noise=ni)(waves)
    y3, _ = GpuSpectrogramFrontEnd(c, normalize=True, device=dev, augment=True, seed=2, noise=ni)(waves)
    assert torch.equal(y1, y2) and torch.equal(y1, xm) and not torch.equal(y1, y3)


def _corpus(tmp_path, n=11, sr=16000):
    import pandas as pd
    from scipy.io import wavfile
    from asr_amd.data import write_manifest
    rng = np.random.default_rng(9)
    rows = []
    for i in range(n):
        m = {4: 9637, 7: 9600}.get(i, int(rng.integers(4000, 24000)) + (37 if i % 3 == 0 else 0))   # 4 and 7: equal frame counts (stable sort)
        wavfile.write(str(tmp_path / f"u{i:02d}.wav"), sr, (np.sin(np.arange(m) * (0.01 + 0.003 * i)) * 8000 + rng.standard_normal(m) * 500).astype(np.int16))
        rows.append((str(tmp_path / f"u{i:02d}.wav"), m / sr, sr, "".join(rng.choice(list("abcd"), size=int(rng.integers(2, 6))))))
    write_manifest(rows, str(tmp_path / "manifest.csv"))
    pd.DataFrame({"label": ["_", "a", "b", "c", "d"]}).to_csv(tmp_path / "labels.csv", index=False)
    (tmp_path / "noise").mkdir()
    wavfile.write(str(tmp_path / "noise" / "n.wav"), sr, (rng.standard_normal(30000) * 3000).astype(np.int16))
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def test_loader_front_end_gpu_matches_host_without_augmentation(dev, tmp_path):
    from asr_amd.data import DistributedLengthBucketingSampler, GpuAudioDataLoader, get_loader
    manifest, labels = _corpus(tmp_path)
    runs = {}
    for fe in ("host", "gpu"):
        np.random.seed(4)
        loader, _ = get_loader(conf(), labels, manifest, batch_size=4, num_workers=0, front_end=fe)
        runs[fe] = list(loader)
    assert len(runs["host"]) == len(runs["gpu"]) == 3
    for (xh, th, ph, sh), (xg, tg, pg, sg) in zip(runs["host"], runs["gpu"]):
        assert xg.is_cuda and xg.shape == xh.shape
        assert torch.equal(th, tg) and torch.equal(ph, pg) and torch.equal(sh, sg) and th.dtype == tg.dtype and ph.dtype == pg.dtype
        assert float((xg.cpu() - xh).abs().max()) < 2e-4                           # normalised spectrograms (the 2e-5 x 10 bar)
    # the distributed length-bucketing sampler behind the GPU loader: rank 1 of 2 gets its bins, sorted like _collate_fn
    np.random.seed(4)
    loader, _ = get_loader(conf(), labels, manifest, batch_size=2, num_workers=0, front_end="gpu")
    ds = loader.dataset
    sampler = DistributedLengthBucketingSampler(ds, batch_size=2, num_replicas=2, rank=1)
    gl = GpuAudioDataLoader(ds, sampler, 0, loader.front_end)
    seen = 0
    for (x, t, pct, tsz), ids in zip(gl, list(sampler)):
        want = sorted(ids, key=lambda i: 1 + len(ds[i][0]) // 160, reverse=True)
        assert torch.equal(t, torch.tensor([c for i in want for c in ds[i][1]], dtype=torch.int32))
        assert x.size(3) == 1 + len(ds[want[0]][0]) // 160 and float(pct[0]) == 1.0
        seen += 1
    assert seen == len(sampler)


def test_loader_front_end_gpu_with_augmentation_trains(dev, tmp_path):
    """Noise on every utterance and SpecAugment, through get_loader(front_end="gpu") and one DeepSpeechTrainer.fit step: finite loss;
    the batches differ from un-augmented ones of the same items, and with caching=True the augmentation is redrawn for cached waveforms."""
    from test_gpu_model import make_model
    from asr_amd import CTCLoss
    from asr_amd.data import GpuAudioDataLoader, GpuSpectrogramFrontEnd, get_loader
    from asr_amd.trainers import DeepSpeechTrainer
    manifest, labels = _corpus(tmp_path)
    c = conf(noise_dir=str(tmp_path / "noise"), noise_prob=1.0, spec_augment=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                            # nothing requested is ignored on this path
        loader, _ = get_loader(c, labels, manifest, batch_size=4, num_workers=0, front_end="gpu", caching=True)
    assert loader.front_end.noise is not None and loader.front_end.spec_augment
    raw = list(loader.loader)                                                     # (waveform, ids) items as the workers deliver them
    assert len(loader.dataset._cache) == 11
    plain = GpuAudioDataLoader(loader.dataset, None, 0, GpuSpectrogramFrontEnd(conf(), normalize=True))
    e1 = [loader.collate(r) for r in raw]
    for a, b in zip(e1, [plain.collate(r) for r in raw]):
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[0].shape == b[0].shape
        assert not torch.equal(a[0], b[0]) and bool(torch.isfinite(a[0]).all())
    assert any(bool((a[0][0, 0] == 0).all(dim=1).any()) for a in e1)               # a frequency mask on an utterance without padding
    e2 = [x for x in loader]                                                      # the next epoch, from the cache: drawn anew
    assert len(e2) == len(e1)
    assert not torch.equal(loader.collate(raw[0])[0], e1[0][0])
    torch.manual_seed(0)
    model = make_model(dict(rnn="gru", hidden=32, layers=2, classes=5))
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, torch.optim.AdamW(model.parameters(), lr=1e-3), None, None, "cuda",
                           "cuda", False, None)
    valid, loss, loss_value = tr.fit(e1[0])
    assert valid and np.isfinite(loss_value) and bool(torch.isfinite(loss))
