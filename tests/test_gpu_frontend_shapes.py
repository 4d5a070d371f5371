"""-m gpu: the spectrogram front-end (ds2_spectrogram_f32 / ds2_spectrogram_aug_f32, csrc/stft.hip) away from 320 / 160 / hamming: the
shape grid of tests/frontend_cases.py against oracle.stft_oracle in fp64 — the GEMM's vectorised B loads (n_fft % 4 == 2), A rows that
overlap 1, 3 and 4 times, bin counts of exactly one 32-bin block and one past eight, 64 and 65 frames, utterances of n_fft/2 samples and
fewer under reflect padding (np.pad reflects as often as it takes; the kernel used to reflect only once), one-sample and
empty rows —, the frames= argument on both sides of the batch's own width, a silent utterance, the augmented entry's exact properties,
the front-end class at an 8 kHz / 25 ms / hann config, and the refusals.

Tolerances are not taken from the kernel: frontend_cases.E32 holds, per case, the error of an fp32 CPU restatement against the fp64 oracle
(at most 4.5e-6), and tol = max(2e-5, 4 * e32) = 2e-5 un-normalised in every case, x 2 / std_b for a normalised utterance.

Teeth (checked on the CPU, tests/test_oracle_golden.py::test_frontend_case_table_and_teeth): frames shifted by one sample and a symmetric
(fftbins=False) window miss the tolerance in all 15 cases, normalised or not; the one-reflection pad rule misses it in all 8 reflect
cases (the rows of n_fft/2 samples and fewer); statistics with biased variance miss it in all 15 normalised cases."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import augment_oracle as A
import det
import frontend_cases as F

pytestmark = pytest.mark.gpu

PADS = ["constant", "reflect"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def g(a, dev):
    return torch.as_tensor(np.asarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def reference(shape, pad_mode, normalize, frames=0):
    """Computed once per case and shared; the arrays are read-only."""
    n_fft, hop, window = shape
    ref, fr, std = F.oracle_batch(F.grid_waves(n_fft, hop), n_fft, hop, window, pad_mode, normalize, frames)
    ref.setflags(write=False)
    return ref, tuple(fr), tuple(std)


def check_values(got, waves, shape, pad_mode, normalize, frames=0):
    """Every comparable row within the case's tolerance; the empty row and all padding exactly 0."""
    n_fft, hop, window = shape
    ref, fr, std = reference(shape, pad_mode, normalize, frames)
    ref_un, _, _ = reference(shape, pad_mode, False, frames)
    tol = F.tolerance(n_fft, hop, window, pad_mode)
    assert got.shape == ref.shape
    for b, (y, f) in enumerate(zip(waves, fr)):
        assert float(np.abs(got[b, 0, :, f:]).max(initial=0.0)) == 0.0, b         # exact zero padding; an empty utterance: all of it
        if F.comparable(y, ref_un[b, 0, :, :f], normalize):
            t = tol * 2.0 / std[b] if normalize else tol
            err = float(np.abs(got[b, 0, :, :f] - ref[b, 0, :, :f]).max())
            print(f"{F.shape_id(shape)} {pad_mode} normalize={normalize} frames={frames} row {b} n={len(y)}: err {err:.3e} tol {t:.3e}")
            assert err < t, (b, len(y), err, t)
        assert np.isfinite(got[b]).all(), b


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("shape", F.GRID, ids=F.shape_id)
def test_shape_grid_vs_oracle(dev, shape, pad_mode, normalize):
    from asr_amd import ops
    n_fft, hop, window = shape
    waves = F.grid_waves(n_fft, hop)
    lens = [len(w) for w in waves]
    ref, frames_ref, _ = reference(shape, pad_mode, normalize)
    # the oracle does not define the empty row (np.pad cannot reflect nothing; zero padding would make one frame): frontend_cases.oracle_batch
    # puts the kernel's contract there — 0 frames, a spectrogram of exact zeros
    assert lens[F.EMPTY_ROW] == 0 and frames_ref[F.EMPTY_ROW] == 0 and max(frames_ref) == 65 and 64 in frames_ref
    batch = g(F.garbage_batch(waves), dev)
    out, frames = ops.spectrogram(batch, torch.tensor(lens), n_fft, hop, window, pad_mode, normalize)
    assert frames.tolist() == list(frames_ref)
    assert tuple(out.shape) == (len(waves), 1, n_fft // 2 + 1, 65)
    check_values(out.cpu().numpy(), waves, shape, pad_mode, normalize)
    again, _ = ops.spectrogram(batch, torch.tensor(lens), n_fft, hop, window, pad_mode, normalize)
    assert torch.equal(out, again)                                                 # reruns give the same bits


@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("shape", [F.GRID[0], F.GRID[3]], ids=F.shape_id)
def test_frames_argument(dev, shape, pad_mode):
    """frames= wider than the batch: the kernel writes the zeros (the buffer comes back dirty from the allocator) and everything else keeps
    the default call's bits.  frames= narrower: every utterance is cut to its first T frames, un-normalised values keep their bits, and the
    statistics of a normalised utterance are those of the nb * min(T, frames) elements that are left (unbiased)."""
    from asr_amd import ops
    n_fft, hop, window = shape
    nb = n_fft // 2 + 1
    waves = F.grid_waves(n_fft, hop)
    lens = torch.tensor([len(w) for w in waves])
    batch = g(F.garbage_batch(waves), dev)
    for normalize in (False, True):
        base, fr = ops.spectrogram(batch, lens, n_fft, hop, window, pad_mode, normalize)
        wide_T = 65 + 70
        torch.full((len(waves), 1, nb, wide_T), float("nan"), device=dev)          # leave NaNs for the allocator to hand back
        wide, fr_w = ops.spectrogram(batch, lens, n_fft, hop, window, pad_mode, normalize, frames=wide_T)
        assert tuple(wide.shape) == (len(waves), 1, nb, wide_T) and fr_w.tolist() == fr.tolist()
        assert torch.equal(wide[..., :65], base)
        for b, f in enumerate(fr.tolist()):
            assert float(wide[b, 0, :, f:].abs().max()) == 0.0 and bool(torch.isfinite(wide[b]).all()), b
        T = 65 - 3
        cut, fr_c = ops.spectrogram(batch, lens, n_fft, hop, window, pad_mode, normalize, frames=T)
        assert tuple(cut.shape) == (len(waves), 1, nb, T) and fr_c.tolist() == [min(f, T) for f in fr.tolist()]
        assert fr_c.tolist() == list(reference(shape, pad_mode, normalize, T)[1])
        if not normalize:
            assert torch.equal(cut, base[..., :T])
        check_values(cut.cpu().numpy(), waves, shape, pad_mode, normalize, frames=T)


@pytest.mark.parametrize("pad_mode", PADS)
def test_silent_utterance_normalises_to_zero(dev, pad_mode):
    """An all-zero waveform with normalize=True: the kernel's contract is rstd = 0 for zero variance (stft_stats_kernel), so the output is
    exactly 0 and finite.  This DIVERGES from the reference arithmetic, (spect - mean) / std = 0 / 0 = NaN, which the oracle reproduces."""
    from asr_amd import ops
    from oracle import stft_oracle as S
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(S.stft_log_spectrogram(np.zeros(800, np.float32), 400, 160, "hamming", pad_mode, normalize=True)).all()
    out, frames = ops.spectrogram(torch.zeros(1, 800, device=dev), torch.tensor([800]), 400, 160, "hamming", pad_mode, True)
    assert frames.tolist() == [6] and tuple(out.shape) == (1, 1, 201, 6)
    assert float(out.abs().max()) == 0.0 and bool(torch.isfinite(out).all())


# ---- the augmented entry --------------------------------------------------------------------------------------------------------
def aug_case(shape):
    """Five utterances: 65 frames (a time mask across frame 64), a middle one, the short reflected one (n_fft/2 - 1 samples, with noise:
    the noise is read at the reflected index too), one on a silent noise file, one at level 0."""
    n_fft, hop, window = shape
    nb = n_fft // 2 + 1
    lens = [64 * hop + 5, 7 * hop + 3, n_fft // 2 - 1, 3 * hop, hop]
    waves = [F.wave(i, n, 1300 + n_fft) for i, n in enumerate(lens)]
    files = [(0.5 * det.unitvar((2 * lens[0],), 311) - 0.25).astype(np.float32), (0.8 * det.unitvar((lens[0] // 3,), 312) - 0.4).astype(np.float32),
             np.zeros(500, np.float32)]                                            # long; shorter than utterance 0 (wraps); silent
    plan = [(1, 0.3, 0.63), (0, 0.25, 0.25), (0, 0.3, 0.5), (2, 0.5, 0.5), (0, 0.0, 0.1)]        # utterance -> (file, level, u)
    freq = [[(nb - 3, nb), (1, 4)], [(0, 0), (nb // 2, nb // 2 + 1)], [(0, 2), (0, 0)], [(2, 3), (3, 5)], [(nb - 1, nb), (0, 0)]]
    time = [[(60, 70)], [(0, 1)], [(0, 0)], [(1, 3)], [(1, 70)]]                   # the last reaches beyond its utterance's 2 frames; the short
    #                                                                                reflected row (1 or 2 frames) keeps its frames unmasked
    return lens, waves, files, plan, freq, time


def aug_call(dev, shape, batch, pad_mode, normalize, noise=True, masks=True, levels=None):
    from asr_amd import ops
    n_fft, hop, window = shape
    lens, _, files, plan, freq, time = aug_case(shape)
    starts = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.int64)
    kw = {}
    if noise:
        kw = dict(noise=g(np.concatenate(files), dev), noise_base=[int(starts[f]) for f, _, _ in plan],
                  noise_period=[len(files[f]) for f, _, _ in plan],
                  noise_start=[A.start_of(len(files[f]), n, u) for (f, _, u), n in zip(plan, lens)],
                  noise_level=np.array([p[1] for p in plan] if levels is None else levels, np.float32))
    if masks:
        kw.update(freq_masks=np.array(freq, np.int32), time_masks=np.array(time, np.int32))
    return ops.spectrogram_augmented(batch, torch.tensor(lens), n_fft, hop, window, pad_mode, normalize, **kw)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("pad_mode", PADS)
@pytest.mark.parametrize("shape", [F.GRID[0], F.GRID[3]], ids=F.shape_id)
def test_augmented_entry_exact_properties(dev, shape, pad_mode, normalize):
    from asr_amd import ops
    n_fft, hop, window = shape
    lens, waves, files, plan, freq, time = aug_case(shape)
    batch = g(F.garbage_batch(waves), dev)
    plain, frames = ops.spectrogram(batch, torch.tensor(lens), n_fft, hop, window, pad_mode, normalize)
    assert frames.tolist() == [65, 8, 1 + (n_fft // 2 - 1) // hop, 4, 2]
    # no noise (absent, or level 0 everywhere) and no masks: the bits of ds2_spectrogram_f32
    for kw in (dict(noise=False), dict(levels=[0.0] * 5)):
        off, fr = aug_call(dev, shape, batch, pad_mode, normalize, masks=False, **kw)
        assert torch.equal(off, plain) and fr.tolist() == frames.tolist()
    # masks only: masked elements exactly 0, all others the plain bits (the statistics are those of the unmasked spectrogram)
    only, _ = aug_call(dev, shape, batch, pad_mode, normalize, noise=False)
    o, p = only.cpu().numpy(), plain.cpu().numpy()
    masked = np.zeros(o.shape, bool)
    for b, f in enumerate(frames.tolist()):
        for lo, hi in freq[b]:
            masked[b, 0, lo:hi, :f] = True
        for lo, hi in time[b]:
            masked[b, 0, :, lo:min(hi, f)] = True
        assert (o[b, 0, :, f:] == 0).all()
    assert masked[0, 0, -1, 0] and masked[0, 0, 0, 64] and not masked[0, 0, 0, 59]  # the last bin; a time mask across the 64-frame block edge
    assert (o[masked] == 0).all() and np.array_equal(o[~masked], p[~masked])
    # noise and masks against the fp64 contract, at the case's tolerance (x 2 / std_b of the mixed utterance when normalised)
    out, fr = aug_call(dev, shape, batch, pad_mode, normalize)
    again, _ = aug_call(dev, shape, batch, pad_mode, normalize)
    assert torch.equal(out, again)
    args = ([float(np.float32(q[1])) for q in plan], [q[2] for q in plan], [q[0] for q in plan])
    ref, frames_ref = A.augmented_spectrogram(waves, files, *args, freq, time, n_fft, hop, window, pad_mode, normalize)
    mixed, _ = A.augmented_spectrogram(waves, files, *args, [[]] * 5, [[]] * 5, n_fft, hop, window, pad_mode, False)
    assert fr.tolist() == frames_ref and tuple(out.shape) == ref.shape
    got = out.cpu().numpy()
    tol = F.tolerance(n_fft, hop, window, pad_mode)
    for b, f in enumerate(frames_ref):
        t = tol * 2.0 / float(mixed[b, 0, :, :f].std(ddof=1)) if normalize else tol
        err = float(np.abs(got[b] - ref[b]).max())
        print(f"aug {F.shape_id(shape)} {pad_mode} normalize={normalize} row {b}: err {err:.3e} tol {t:.3e}")
        assert err < t, (b, err, t)
    nomask, _ = aug_call(dev, shape, batch, pad_mode, normalize, masks=False)
    assert torch.equal(nomask[3:5], plain[3:5])                                    # a silent noise file, level 0: the plain bits
    for b in (0, 1, 2):                                                            # the noise really went in, the short reflected row included
        assert float((nomask[b] - plain[b]).abs().max()) > 100 * tol


# ---- the front-end class ----------------------------------------------------------------------------------------------------------
def test_front_end_class_8khz_hann(dev):
    """GpuSpectrogramFrontEnd derives n_fft = 200, hop = 80 from an 8 kHz / 25 ms / 10 ms config: against the host path item by item
    (_stft_spectrogram, then torch's mean / unbiased std as the dataset does), zero-padded to the longest as _collate_fn pads."""
    from asr_amd.data import GpuSpectrogramFrontEnd, _stft_spectrogram
    from oracle import stft_oracle as S
    conf = SimpleNamespace(sample_rate=8000, window_size=0.025, window_stride=0.01, window="hann")
    fe = GpuSpectrogramFrontEnd(conf, normalize=True, pad_mode="reflect", device=dev)
    assert (fe.n_fft, fe.hop, fe.window) == F.FRONT_END
    waves = F.front_end_waves()                                                    # longest first, as _collate_fn sorts; the last has 60 samples
    x, pct = fe(list(waves))
    frames = [1 + len(w) // 80 for w in waves]
    T = max(frames)
    assert tuple(x.shape) == (3, 1, 101, T)
    assert pct.dtype == torch.float32 and torch.equal(pct.cpu(), torch.tensor(frames, dtype=torch.float32) / float(T))     # frames / T
    got = x.cpu()
    tol = F.tolerance(*F.FRONT_END, "reflect")
    for b, (w, f) in enumerate(zip(waves, frames)):
        s = torch.from_numpy(_stft_spectrogram(w, 8000, 0.025, 0.01, "hann", "reflect"))
        want = torch.zeros(101, T)
        want[:, :f] = (s - s.mean()) / s.std()
        std = float(S.stft_log_spectrogram(w, 200, 80, "hann", "reflect").std(ddof=1))
        err = float((got[b, 0] - want).abs().max())
        print(f"front-end row {b} n={len(w)}: err {err:.3e} tol {tol * 2.0 / std:.3e}")
        assert err < tol * 2.0 / std, (b, err)
        assert float(got[b, 0, :, f:].abs().sum()) == 0.0                           # padded after the normalisation


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", [(441, 160), (320, 6), (64, 128), (2, 4)], ids=["odd-n_fft", "hop-6", "hop-above-n_fft", "n_fft-2"])
def test_entries_refuse_shapes_outside_the_contract(dev, n_fft, hop):
    """Checked on the host before any launch: the library's error with the 'bad dims' message, from both entries."""
    from asr_amd import _lib, ops
    x = torch.zeros(2, 1000, device=dev)
    with pytest.raises(_lib.DS2LibraryError, match="ds2_spectrogram_f32: bad dims"):
        ops.spectrogram(x, torch.tensor([1000, 500]), n_fft, hop, "hamming")
    with pytest.raises(_lib.DS2LibraryError, match="ds2_spectrogram_aug_f32: bad dims"):
        ops.spectrogram_augmented(x, torch.tensor([1000, 500]), n_fft, hop, "hamming")
    torch.cuda.synchronize()
