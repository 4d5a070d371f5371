"""The spectrogram front-end's shape grid, its waveforms and an fp32 CPU restatement of the kernels' arithmetic — TEST INFRASTRUCTURE ONLY,
shared by tests/test_gpu_frontend_shapes.py (the GPU comparisons) and tests/test_oracle_golden.py (which recomputes the error table below
and the teeth of the tolerances on the CPU).

E32[(n_fft, hop, window, pad_mode)] = (e32, tol), e32 = max |fp32 restatement - fp64 oracle| over the case's un-normalised batch (two digits, up):
what fp32 frames x the fp32 basis (`ops.dft_basis_host`, a numpy float32 matmul) and a float32 log1p(sqrt(re^2 + im^2)) lose against
oracle.stft_oracle.  The MFMA chain and the host BLAS are both fp32 dot products of n_fft terms with the same worst-case bound and differ
only in summation order, hence tol = max(2e-5, 4 * e32) un-normalised, and tol * 2 / std_b (the oracle's fp64 unbiased standard deviation
of utterance b; 2 for the fp32 block partials of the statistics) for a normalised utterance.
"""
from __future__ import annotations

import functools

import numpy as np

import det
from oracle import stft_oracle as S

GRID = [(400, 160, "hamming"),      # 25 ms window; row ratio 3; 201 bins
        (512, 128, "hann"),         # power of two; row ratio 4; 257 bins, one past eight 32-bin blocks
        (160, 80, "hamming"),       # 8 kHz config
        (62, 32, "blackman"),       # 32 bins, exactly one block; ldb = 64 takes the vectorised B path of the GEMM
        (64, 64, "hamming"),        # hop == n_fft, no overlap, R == T; 33 bins
        (8, 4, "hann"),             # 5 bins, K = 8
        (4, 4, "hamming")]          # the smallest shape the entry accepts
FRONT_END = (200, 80, "hann")       # audio_conf(sample_rate=8000, window_size=0.025, window_stride=0.01, window="hann")
FRONT_END_LENS = [1234, 800, 60]
FULL_SCALE = {(400, 160), (512, 128)}
EMPTY_ROW = 3                       # where the n = 0 row sits in a grid batch: between two utterances, not at an end

# (e32, un-normalised tolerance) per case: e32 measured once on the CPU by `measure_e32` (fp32 restatement against the fp64 oracle on this
# file's waveforms), rounded up; tolerance = max(2e-5, 4 * e32), which is the 2e-5 floor in every case
E32 = {
    (400, 160, "hamming", "constant"): (2.4e-06, 2e-5), (400, 160, "hamming", "reflect"): (2.8e-06, 2e-5),
    (512, 128, "hann", "constant"): (4.5e-06, 2e-5), (512, 128, "hann", "reflect"): (4.5e-06, 2e-5),
    (160, 80, "hamming", "constant"): (6.9e-07, 2e-5), (160, 80, "hamming", "reflect"): (6.9e-07, 2e-5),
    (62, 32, "blackman", "constant"): (3.1e-07, 2e-5), (62, 32, "blackman", "reflect"): (3.7e-07, 2e-5),
    (64, 64, "hamming", "constant"): (3.8e-07, 2e-5), (64, 64, "hamming", "reflect"): (3.8e-07, 2e-5),
    (8, 4, "hann", "constant"): (8.2e-08, 2e-5), (8, 4, "hann", "reflect"): (8.2e-08, 2e-5),
    (4, 4, "hamming", "constant"): (4.7e-08, 2e-5), (4, 4, "hamming", "reflect"): (4.7e-08, 2e-5),
    (200, 80, "hann", "reflect"): (8.3e-07, 2e-5),
}


def shape_id(shape):
    return f"{shape[0]}-{shape[1]}-{shape[2]}"


def tolerance(n_fft, hop, window, pad_mode):
    return E32[(n_fft, hop, window, pad_mode)][1]


def lengths(n_fft, hop):
    """One row each; the empty row goes in at EMPTY_ROW, the full-scale row (two shapes) at the end."""
    h = n_fft // 2
    lens = [h + 1, h, h - 1, 1, hop - 1, hop, 5 * hop, 5 * hop - 1, 64 * hop, 64 * hop - 1]
    lens.insert(EMPTY_ROW, 0)
    if (n_fft, hop) in FULL_SCALE:
        lens.append(9 * hop + 7)
    return lens


def wave(i, n, seed=700):
    """The existing recipe: a sine plus uniform noise, amplitude about 0.3 + 0.17."""
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * (200.0 + 150 * i) * t) + 0.1 * det.unitvar((n,), seed + i)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid_waves(n_fft, hop):
    lens = lengths(n_fft, hop)
    waves = [wave(i, n, 700 + n_fft) for i, n in enumerate(lens)]
    if (n_fft, hop) in FULL_SCALE:
        w = waves[-1].astype(np.float64)
        waves[-1] = (w / np.abs(w).max()).astype(np.float32)          # peak exactly 1.0
        assert float(np.abs(waves[-1]).max()) == 1.0
    for w in waves:
        w.setflags(write=False)
    return tuple(waves)


@functools.lru_cache(maxsize=None)
def front_end_waves():
    waves = [wave(i, n, 1900) for i, n in enumerate(FRONT_END_LENS)]
    for w in waves:
        w.setflags(write=False)
    return tuple(waves)


def garbage_batch(waves, fill=7.5):
    """(B, max n + 37): an odd row pitch, garbage beyond each length that must not leak in."""
    batch = np.full((len(waves), max(len(w) for w in waves) + 37), fill, dtype=np.float32)
    for i, w in enumerate(waves):
        batch[i, :len(w)] = w
    return batch


def oracle_batch(waves, n_fft, hop, window, pad_mode, normalize, frames=0):
    """oracle.stft_oracle.batch_spectrogram plus the two things it does not define: an empty utterance (np.pad refuses to reflect an
    empty array, and zero padding would give one frame) is a row of zeros with 0 frames — the kernel's contract —, and `frames` > 0
    truncates every utterance to its first `frames` frames BEFORE the statistics and pads the batch to that width.
    Returns (ref (B,1,bins,T) fp64, frames list, std list: the fp64 unbiased standard deviation of each un-normalised utterance)."""
    nb = n_fft // 2 + 1
    specs = []
    for y in waves:
        if len(y) == 0:
            specs.append(np.zeros((nb, 0)))
            continue
        s = S.batch_spectrogram([y], n_fft, hop, window, pad_mode, False)[0][0, 0]
        specs.append(s[:, :frames] if frames else s)
    T = frames or max(max(s.shape[1] for s in specs), 1)
    out = np.zeros((len(specs), 1, nb, T))
    std = []
    for i, (y, s) in enumerate(zip(waves, specs)):
        std.append(float(s.std(ddof=1)) if s.size > 1 else 0.0)
        if normalize and s.size:
            with np.errstate(invalid="ignore", divide="ignore"):     # a constant utterance: 0 / 0, excluded by `comparable`
                if frames:                                           # statistics over nb * min(T, frames) elements, unbiased
                    s = (s - s.mean()) / s.std(ddof=1) if s.size > 1 else s * np.nan
                else:
                    s = S.batch_spectrogram([y], n_fft, hop, window, pad_mode, True)[0][0, 0]
        out[i, 0, :, :s.shape[1]] = s
    return out, [s.shape[1] for s in specs], std


def comparable(y, spect, normalize):
    """The normalisation rule: a normalised row is compared only if its spectrogram holds at least two distinct values; a one-sample row
    is compared un-normalised only under either padding (zeros: one constant frame; reflect: the frame is y[0] times the window)."""
    if len(y) == 0:
        return False                                              # checked exactly instead
    if not normalize:
        return True
    return len(y) > 1 and has_two_values(spect)


def has_two_values(spect):
    """Distinct beyond the round-off of the fp64 FFT (a one-sample utterance under zero padding has |y0 w[n_fft/2]| in every bin, give
    or take 1e-17): the spread exceeds 1e-6, far below anything a real utterance's bins differ by."""
    return float(np.ptp(spect)) > 1e-6


# ---- numpy restatements of the kernels' rules -------------------------------------------------------------------------------------
def reflect_index(j, n):
    """stft_pad_kernel's index rule for reflect padding: fold j into [0, 2(n-1)), mirror the upper half; n == 1: every index is 0."""
    j = np.asarray(j, dtype=np.int64)
    P = 2 * (n - 1)
    if P == 0:
        return np.zeros_like(j)
    j = j % P                                                      # (numpy's % is already non-negative)
    return np.where(j >= n, P - j, j)


def one_reflection_index(j, n):
    """The rule the kernel had before: one reflection, anything still outside [0, n) reads as zero (returned as -1)."""
    j = np.asarray(j, dtype=np.int64)
    r = np.where(j < 0, -j, np.where(j >= n, 2 * (n - 1) - j, j))
    return np.where((r >= 0) & (r < n), r, -1)


def padded_fp32(y, half, pad_mode, pad_rule=reflect_index):
    y = np.asarray(y, dtype=np.float32)
    n = len(y)
    j = np.arange(-half, n + half)
    if pad_mode == "constant":
        idx = np.where((j >= 0) & (j < n), j, -1)
    else:
        idx = pad_rule(j, n)
    return np.where(idx >= 0, y[np.clip(idx, 0, n - 1)], np.float32(0)).astype(np.float32)


def restate_fp32(y, n_fft, hop, window, pad_mode, normalize=False, shift=0, fftbins=True, pad_rule=reflect_index, ddof=1):
    """What the four kernels compute, in float32 on the host: float32 padded frames x the float32 basis (np.float32 matmul), float32
    log1p(sqrt(re^2 + im^2)), statistics combined in float64.  The keyword arguments are the teeth check's mutations: frames shifted by
    `shift` samples, a symmetric window, the one-reflection pad rule, biased variance."""
    from asr_amd import ops
    if fftbins:
        basis = ops.dft_basis_host(n_fft, window)
    else:
        from scipy.signal import get_window
        basis = ops.dft_basis_host(n_fft, "boxcar") * get_window(window, n_fft, fftbins=False).astype(np.float32)[:, None]
    assert basis.dtype == np.float32
    yp = np.concatenate([padded_fp32(y, n_fft // 2, pad_mode, pad_rule), np.zeros(shift, np.float32)])
    T = 1 + len(y) // hop
    frames = np.stack([yp[t * hop + shift: t * hop + shift + n_fft] for t in range(T)]).astype(np.float32)
    C = frames @ basis
    assert C.dtype == np.float32
    re, im = C[:, 0::2], C[:, 1::2]
    spect = np.log1p(np.sqrt(re * re + im * im)).T
    assert spect.dtype == np.float32
    if normalize:
        s64 = spect.astype(np.float64)
        spect = ((s64 - s64.mean()) / s64.std(ddof=ddof)).astype(np.float32)
    return spect


def cases():
    """(n_fft, hop, window, pad_mode, waves) of every row of E32."""
    for n_fft, hop, window in GRID:
        for pad_mode in ("constant", "reflect"):
            yield n_fft, hop, window, pad_mode, grid_waves(n_fft, hop)
    yield FRONT_END + ("reflect", front_end_waves())


def measure_e32(n_fft, hop, window, pad_mode, waves):
    worst = 0.0
    for y in waves:
        if len(y):
            ref = S.stft_log_spectrogram(y, n_fft, hop, window, pad_mode)
            worst = max(worst, float(np.abs(restate_fp32(y, n_fft, hop, window, pad_mode) - ref).max()))
    return worst


def misses(n_fft, hop, window, pad_mode, waves, normalize, **mutation):
    """True if the fp32 restatement with `mutation` misses the case's tolerance on some comparable row."""
    tol = tolerance(n_fft, hop, window, pad_mode)
    for y in waves:
        if len(y) == 0:
            continue
        ref = S.stft_log_spectrogram(y, n_fft, hop, window, pad_mode)
        if not comparable(y, ref, normalize):
            continue
        t = tol
        if normalize:
            t = tol * 2.0 / float(ref.std(ddof=1))
            ref = (ref - ref.mean()) / ref.std(ddof=1)
        if float(np.abs(restate_fp32(y, n_fft, hop, window, pad_mode, normalize, **mutation) - ref).max()) >= t:
            return True
    return False
