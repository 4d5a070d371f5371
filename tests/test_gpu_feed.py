"""-m gpu: the pipelined waveform feed — the unpack kernel (ds2_wave_unpack_f32) against numpy, exactly; get_loader(front_end="gpu",
prefetch=N) batch for batch bit-identical to the synchronous loader, with every augmentation and with none, with and without workers; the
iterator's lifecycle (early exit, a failing worker); and three train steps fed through it against the same steps fed synchronously."""
import copy
import threading
import time
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import det

pytestmark = pytest.mark.gpu

FEEDER = "asr_amd-waveform-feeder"


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


def pcm(n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 9000).clip(-32768, 32767).astype(np.int16)
    if n >= 2:
        x[0], x[-1] = -32768, 32767
    return x


def unpack_reference(waves, src_index, n_max):
    """numpy: row b = utterance src_index[b] as float32 (int16 / 32768, the arithmetic of asr_amd.data._read_wav), zeros beyond its length."""
    ref = np.zeros((len(src_index), n_max), np.float32)
    for b, u in enumerate(src_index):
        w = waves[u]
        ref[b, :len(w)] = w.astype(np.float32) / 32768.0 if w.dtype == np.int16 else w
    return ref


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("kind", ["int16", "fp32"])
def test_unpack_vs_numpy(dev, kind):
    """Exact equality (bit patterns), for: the extreme samples -32768 and 32767, a permuted src_index, a zero-length row, n_max not a
    multiple of the vector width (8) and larger than every length, row pitches of every alignment, B = 1."""
    from asr_amd import ops
    from asr_amd.data import pack_waveforms
    lens = [4001, 0, 8, 1, 2555, 13, 16000, 7]
    if kind == "int16":
        waves = [pcm(n, 10 + i) for i, n in enumerate(lens)]
        assert waves[0][0] == -32768 and waves[0][-1] == 32767
    else:
        waves = [det.unitvar((n,), 20 + i).astype(np.float32) * np.float32(0.37) for i, n in enumerate(lens)]
    buf, off, ln, _ = pack_waveforms([(w, []) for w in waves])
    assert buf.dtype == (torch.int16 if kind == "int16" else torch.float32)
    packed = buf.to(dev)
    order = [6, 0, 4, 5, 2, 7, 3, 1]
    for src, n_max in ((None, None), (order, None), (order, 16003), (order, 16009), (order, 16010), (order[::-1], 16001), ([3, 3, 1, 0, 0, 6, 6, 2], 16000)):
        got = ops.wave_unpack(packed, off, ln, src, n_max)
        idx = list(range(len(lens))) if src is None else src
        ref = unpack_reference(waves, idx, max(lens) if n_max is None else n_max)
        assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_contiguous()
        assert np.array_equal(bits(got.cpu().numpy()), bits(ref)), (kind, src, n_max)
    # the unpacked int16 batch equals the float32 batch of the same files, bit for bit
    if kind == "int16":
        fbuf, foff, fln, _ = pack_waveforms([(w.astype(np.float32) / 32768.0, []) for w in waves])
        assert fbuf.dtype == torch.float32
        assert torch.equal(ops.wave_unpack(fbuf.to(dev), foff, fln, order), ops.wave_unpack(packed, off, ln, order))
    # B = 1, and a batch of empty utterances
    one, o1, l1, _ = pack_waveforms([(waves[4], [])])
    got = ops.wave_unpack(one.to(dev), o1, l1)
    assert np.array_equal(bits(got.cpu().numpy()), bits(unpack_reference(waves, [4], lens[4])))
    none, o0, l0, _ = pack_waveforms([(waves[1], []), (waves[1], [])])
    assert ops.wave_unpack(none.to(dev), o0, l0).shape == (2, 0)
    assert bool((ops.wave_unpack(none.to(dev), o0, l0, n_max=11) == 0).all())
    # reruns are bit-identical
    assert torch.equal(ops.wave_unpack(packed, off, ln, order), ops.wave_unpack(packed, off, ln, order))


def test_unpack_rejects_descriptions_outside_the_contract(dev):
    from asr_amd import _lib, ops
    packed = torch.zeros(64, dtype=torch.int16, device=dev)
    assert ops.wave_unpack(packed, [0, 16], [10, 48]).shape == (2, 48)
    for off, ln, src, n_max in (([0, 12], [10, 20], None, None),        # a misaligned offset
                                ([0, -8], [10, 20], None, None),
                                ([0, 16], [10, 49], None, None),        # ends beyond the buffer
                                ([0, 56], [10, 9], None, None),         # its 8-aligned end does
                                ([0, 16], [10, -1], None, None),
                                ([0, 16], [10, 20], [0, 2], None),      # an index outside [0, B)
                                ([0, 16], [10, 20], [0], None),
                                ([0, 16], [10, 20], None, 19)):         # a length above n_max
        with pytest.raises(ValueError):
            ops.wave_unpack(packed, off, ln, src, n_max)
    with pytest.raises(ValueError):
        ops.wave_unpack(torch.zeros(60, dtype=torch.int16, device=dev), [0], [10])          # not a multiple of 8 elements
    with pytest.raises(ValueError):
        ops.wave_unpack(torch.zeros(64, dtype=torch.int32, device=dev), [0], [10])
    # the C entry point's own checks
    lib, meta, out = _lib.load(), torch.zeros(3, 2, dtype=torch.int32, device=dev), torch.zeros(2, 48, device=dev)
    ok = (packed.data_ptr(), 64, 0, meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), 2, 48, out.data_ptr(), 48, None)
    assert lib.ds2_wave_unpack_f32(*ok) == 0
    for i, v in ((1, 60), (1, -8), (2, 2), (6, 0), (6, 65536), (7, -1), (9, 47), (0, packed.data_ptr() + 2)):
        bad = list(ok)
        bad[i] = v
        assert lib.ds2_wave_unpack_f32(*bad) != 0, (i, v)
    torch.cuda.synchronize()


def _noise_dir(tmp_path):
    from scipy.io import wavfile
    (tmp_path / "noise").mkdir()
    for i, m in enumerate((20000, 3000)):
        wavfile.write(str(tmp_path / "noise" / f"n{i}.wav"), 16000, (det.unitvar((m,), 300 + i) * 6000).astype(np.int16))
    return str(tmp_path / "noise")


def _corpus(tmp_path, n=14, sr=16000, stereo=(5,), missing=()):
    """Ragged 16-bit WAVs; the files in `stereo` have two channels (their batch takes the float32 path), those in `missing` do not exist."""
    import pandas as pd
    from scipy.io import wavfile
    from asr_amd.data import write_manifest
    rng = np.random.default_rng(9)
    rows = []
    for i in range(n):
        m = int(rng.integers(6000, 24000))
        y = (np.sin(np.arange(m) * (0.01 + 0.003 * i)) * 8000 + rng.standard_normal(m) * 500).astype(np.int16)
        if i in stereo:
            y = np.stack([y, y[::-1]], axis=1)
        if i not in missing:
            wavfile.write(str(tmp_path / f"u{i:02d}.wav"), sr, y)
        rows.append((str(tmp_path / f"u{i:02d}.wav"), m / sr, sr, "".join(rng.choice(list("abcd"), size=int(rng.integers(2, 6))))))
    write_manifest(rows, str(tmp_path / "manifest.csv"))
    pd.DataFrame({"label": ["_", "a", "b", "c", "d"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def _make(c, labels, manifest, perturb, prefetch, num_workers, batch_size=4):
    """A loader with fixed seeds: the front-end's seed and the sampler's bin shuffle come from numpy's global state."""
    from asr_amd.data import get_loader
    np.random.seed(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader, sampler = get_loader(c, labels, manifest, batch_size=batch_size, num_workers=num_workers, front_end="gpu", perturb=perturb,
                                     prefetch=prefetch)
    return loader, sampler, copy.deepcopy(sampler.bins)


def _epoch(loader, sampler, bins, stop_after=None):
    """One epoch from the same sampler state (the sampler shuffles its bins in place, from numpy's global state, as it goes)."""
    sampler.bins = copy.deepcopy(bins)
    np.random.seed(11)
    out = []
    for data in loader:
        out.append(data)
        if stop_after is not None and len(out) == stop_after:
            break
    return out


def _same(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))


def _feeders():
    return [t for t in threading.enumerate() if t.name == FEEDER and t.is_alive()]


@pytest.mark.parametrize("augment", [True, False], ids=["all_augmentations", "plain"])
def test_loader_equivalence(dev, tmp_path, augment):
    """prefetch in {1, 3} x num_workers in {0, 2}: every batch of an epoch — inputs, targets, percentages, target sizes — is torch.equal
    to the prefetch=0 loader's, same seeds; one batch holds a stereo file (the float32 buffer), the others are raw int16."""
    manifest, labels = _corpus(tmp_path)
    c = conf(noise_dir=_noise_dir(tmp_path), noise_prob=0.7, noise_levels=(0.1, 0.5), spec_augment=True, speed_volume_perturb=True) if augment else conf()
    kinds = {p[0].dtype for p in _make(c, labels, manifest, augment, 1, 0)[0].loader}
    assert kinds == {torch.int16, torch.float32}
    for workers in (0, 2):
        base = _epoch(*_make(c, labels, manifest, augment, 0, workers))
        assert len(base) == 4 and all(b[0].is_cuda for b in base)
        for prefetch in (1, 3):
            loader, sampler, bins = _make(c, labels, manifest, augment, prefetch, workers)
            assert len(loader) == 4 and loader.front_end.perturb == augment
            got = _epoch(loader, sampler, bins)
            assert len(got) == len(base)
            for k, (a, b) in enumerate(zip(got, base)):
                assert a[0].is_cuda and _same(a, b), (workers, prefetch, k)
            assert not _feeders()
    if augment:                                                    # (the draws do something: a second epoch differs)
        loader, sampler, bins = _make(c, labels, manifest, augment, 1, 0)
        e1, e2 = _epoch(loader, sampler, bins), _epoch(loader, sampler, bins)
        assert any(a[0].shape != b[0].shape or not torch.equal(a[0], b[0]) for a, b in zip(e1, e2))


@pytest.mark.parametrize("workers", [0, 2])
def test_early_exit_and_restart(dev, tmp_path, workers):
    """break after one batch: the feeder thread is gone and no worker process is left; a fresh iteration gives the full epoch, equal to
    the synchronous loader's second epoch from the same state."""
    import multiprocessing
    manifest, labels = _corpus(tmp_path)
    c = conf(spec_augment=True, speed_volume_perturb=True)
    before = set(p.pid for p in multiprocessing.active_children())
    ref_loader, ref_sampler, ref_bins = _make(c, labels, manifest, True, 0, workers)
    first = _epoch(ref_loader, ref_sampler, ref_bins, stop_after=1)
    ref = _epoch(ref_loader, ref_sampler, ref_bins)
    loader, sampler, bins = _make(c, labels, manifest, True, 2, workers)
    got1 = _epoch(loader, sampler, bins, stop_after=1)
    assert len(got1) == 1 and _same(got1[0], first[0])
    assert not _feeders()
    t0 = time.time()
    while set(p.pid for p in multiprocessing.active_children()) - before and time.time() - t0 < 30:
        time.sleep(0.1)
    assert not set(p.pid for p in multiprocessing.active_children()) - before
    got = _epoch(loader, sampler, bins)
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert _same(a, b)
    assert not _feeders()


@pytest.mark.parametrize("workers", [0, 2])
def test_missing_file_raises_in_the_consumer(dev, tmp_path, workers):
    """A manifest row that points at a missing file: the worker's (or the feeder's) error is raised by next(), not a hang."""
    manifest, labels = _corpus(tmp_path, missing=(6,))
    loader, sampler, bins = _make(conf(), labels, manifest, False, 2, workers)
    t0 = time.time()
    with pytest.raises((FileNotFoundError, RuntimeError), match="u06.wav"):
        _epoch(loader, sampler, bins)
    assert time.time() - t0 < 60
    t0 = time.time()
    while _feeders() and time.time() - t0 < 30:
        time.sleep(0.1)
    assert not _feeders()


def test_training_through_the_feed(dev, tmp_path):
    """Three DeepSpeechTrainer.step calls on a small bidirectional GRU fed by prefetch=2: the weights are bit-identical to the same three
    steps fed by prefetch=0, and no persistent recurrence launch starved."""
    from test_gpu_model import make_model
    from asr_amd import CTCLoss, FusedAdamW
    from asr_amd.trainers import DeepSpeechTrainer
    manifest, labels = _corpus(tmp_path, stereo=())
    c = conf(noise_dir=_noise_dir(tmp_path), noise_prob=0.7, noise_levels=(0.1, 0.5), spec_augment=True, speed_volume_perturb=True)
    starved = DeepSpeechTrainer.starved_steps

    def train(prefetch):
        torch.manual_seed(0)
        model = make_model(dict(rnn="gru", hidden=32, layers=2, classes=5))
        tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, FusedAdamW(model, lr=1e-3), None, None, "cuda", "cuda", False, None)
        loader, sampler, bins = _make(c, labels, manifest, True, prefetch, 0)
        losses = []
        for k, data in enumerate(_iterate(loader, sampler, bins)):
            valid, lv = tr.step(data)
            assert valid and np.isfinite(lv)
            losses.append(lv)
            if k == 2:
                break
        tr.synchronize()
        return model.flat_parameters()[0].detach().clone(), losses

    def _iterate(loader, sampler, bins):
        sampler.bins = copy.deepcopy(bins)
        np.random.seed(11)
        return iter(loader)
    w0, l0 = train(0)
    w2, l2 = train(2)
    assert len(l0) == 3 and l0 == l2
    assert torch.equal(w0, w2)
    assert DeepSpeechTrainer.starved_steps == starved
    assert not _feeders()
