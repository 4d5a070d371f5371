"""-m gpu: sample-rate conversion in the waveform feed — the kernel (ds2_wave_resample_f32) against the fp64 oracle
(tests/resample_oracle.py) through the C ABI, its exact properties, rows and arguments outside the contract, and
get_loader(front_end="gpu", resample=True) on a mixed-rate corpus."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resample_oracle as R

pytestmark = pytest.mark.gpu

TARGET = 16000
CANARY = 7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def conf(**kw):
    c = dict(sample_rate=TARGET, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False, spec_augment=False,
             noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    c.update(kw)
    return SimpleNamespace(**c)


def pcm(n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 9000).clip(-32768, 32767).astype(np.int16)
    if n >= 2:
        x[0], x[-1] = -32768, 32767
    return x


_CASE = {}


def case():
    """The batch of the kernel tests, its packed buffers and the oracle's result: computed once, shared, never modified."""
    if not _CASE:
        from asr_amd import _lib
        from asr_amd.data import pack_waveforms
        tile = _lib.load().ds2_resample_tile_samples()
        # every rate; the lengths 4801, 3000, 777, 5, 1, 0 (shorter than the filter, and empty); outputs of one tile - 1, + 0, + 1 at
        # 48 kHz; 9602 outputs on the L = 2 path (tables in LDS) and 1742 on the L = 160 path (tables through L2): several tiles each
        plan = [(48000, 4801), (44100, 3000), (22050, 777), (8000, 5), (48000, 1), (44100, 0), (16000, 3000), (8000, 4801),
                (48000, 3 * tile - 3), (48000, 3 * tile), (48000, 3 * tile + 1), (22050, 4801), (44100, 5), (16000, 0), (44100, 4801),
                (22050, 1)]
        waves = [pcm(n, 40 + i) for i, (_, n) in enumerate(plan)]
        rates = [r for r, _ in plan]
        ref = [R.resample(w.astype(np.float64) / 32768.0, r, TARGET) for w, r in zip(waves, rates)]
        n_out = [len(y) for y, _ in ref]
        assert n_out[8:11] == [tile - 1, tile, tile + 1] and n_out[7] == 9602 and n_out[4] == 1 and n_out[5] == 0
        i16 = pack_waveforms([(w, []) for w in waves])
        f32 = pack_waveforms([(w.astype(np.float32) / 32768.0, []) for w in waves])
        _CASE.update(waves=waves, rates=rates, ref=ref, n_out=n_out, i16=i16, f32=f32, tile=tile)
    return _CASE


def describe(c, dev, packed=None):
    """The arguments of the C entry point for the shared batch, as host arrays plus the device table."""
    from asr_amd import ops
    buf, off, ln, _ = c["i16"] if packed is None else packed
    pairs = tuple((r, TARGET) for r in sorted(set(c["rates"])) if r != TARGET)
    tab, bases = ops._resample_tables(pairs, dev)
    lmj = [ops.resample_ratio(r, TARGET) for r in c["rates"]]
    B = len(c["rates"])
    return dict(buf=buf.to(dev), off=np.array(off), ln=np.array(ln), src=np.arange(B), L=np.array([v[0] for v in lmj]),
                M=np.array([v[1] for v in lmj]), J=np.array([v[2] for v in lmj]),
                base=np.array([bases.get((r, TARGET), 0) for r in c["rates"]]), tab=tab, tab_elems=tab.numel(), B=B,
                n_out_max=max(c["n_out"]))


def launch(d, dev, extra=5, expect_ok=True):
    """One call through the C ABI into the middle of a canary-filled buffer: (rc, out (B, n_out_max + extra) view, the whole buffer)."""
    from asr_amd import _lib
    B, n_max = d["B"], d["n_out_max"]
    ld, guard = n_max + extra, 4096
    whole = torch.full((guard + B * ld + guard,), CANARY, dtype=torch.float32, device=dev)
    out = whole[guard:guard + B * ld].view(B, ld)
    meta = torch.from_numpy(np.stack([d[k] for k in ("off", "ln", "src", "L", "M", "J", "base")]).astype(np.int32)).to(dev)
    buf = d["buf"]
    rc = _lib.load().ds2_wave_resample_f32(buf.data_ptr() if buf.numel() else None, d.get("packed_elems", buf.numel()),
                                           d.get("dtype", 0 if buf.dtype == torch.int16 else 1), *[meta[i].data_ptr() for i in range(7)],
                                           d["tab"].data_ptr(), d["tab_elems"], B, n_max, out.data_ptr(), d.get("ld", ld), None)
    torch.cuda.synchronize()
    assert (rc == 0) == expect_ok, _lib.load().ds2_last_error()
    return rc, out, whole, guard


def guards_intact(whole, guard):
    return bool((whole[:guard] == CANARY).all()) and bool((whole[-guard:] == CANARY).all())


def test_kernel_vs_oracle(dev):
    """Every sample of every row: |y_dev - y_fp64| <= (P + 1) 2^-24 A[m], the bound of a length-P fp32 dot product in any order (the
    fp32 rounding of the int16 samples and of the taps is exact: both are fp32 numbers the oracle is given as they are)."""
    from asr_amd import ops
    c = case()
    d = describe(c, dev)
    _, out, whole, guard = launch(d, dev)
    got = out.cpu().numpy().astype(np.float64)
    n_max = d["n_out_max"]
    worst = 0.0
    for b, ((y, A), r) in enumerate(zip(c["ref"], c["rates"])):
        P = 2 * R.ratio(r, TARGET)[3]
        n = len(y)
        if r == TARGET:
            assert np.array_equal(got[b, :n], y)
        else:
            err, bound = np.abs(got[b, :n] - y), (P + 1) * 2.0 ** -24 * A
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0)
            assert (err <= bound).all(), (b, r, n, float((err - bound).max()))
        assert (got[b, n:n_max] == 0).all(), b                       # exact zeros beyond n_out
        assert n == 0 or np.abs(got[b, :n]).max() > 0
    print("largest |error| / bound:", worst)
    assert bool((out[:, n_max:] == CANARY).all()) and guards_intact(whole, guard)      # columns beyond n_out_max are untouched
    # the 16 kHz row is the unpack pass, bit for bit
    buf, off, ln, _ = c["i16"]
    plain = ops.wave_unpack(buf.to(dev), off, ln)
    assert torch.equal(out[6, :3000], plain[6, :3000]) and bool((out[6, 3000:n_max] == 0).all())
    # and the wrapper gives the same bits as the raw call
    via, n_out = ops.wave_resample(buf.to(dev), off, ln, c["rates"], None, TARGET)
    assert n_out == c["n_out"] and via.shape == (d["B"], n_max) and torch.equal(via, out[:, :n_max])


def test_dtype_order_and_reruns(dev):
    from asr_amd import ops
    c = case()
    buf, off, ln, _ = c["i16"]
    fbuf, foff, fln, _ = c["f32"]
    assert buf.dtype == torch.int16 and fbuf.dtype == torch.float32
    a, n_out = ops.wave_resample(buf.to(dev), off, ln, c["rates"], None, TARGET)
    f, _ = ops.wave_resample(fbuf.to(dev), foff, fln, c["rates"], None, TARGET)
    assert torch.equal(a, f)                                         # int16- and fp32-packed copies of the same audio: identical bits
    B = len(c["rates"])
    order = list(np.random.default_rng(5).permutation(B))
    order[3] = order[9]                                              # a repeat
    p, n_out_p = ops.wave_resample(buf.to(dev), off, ln, c["rates"], order, TARGET)
    assert n_out_p == n_out and torch.equal(p, a[order])
    assert torch.equal(ops.wave_resample(buf.to(dev), off, ln, c["rates"], order, TARGET)[0], p)          # reruns
    # a wider batch: zeros up to n_out_max; all rows at the target rate: the unpack pass
    wide, _ = ops.wave_resample(buf.to(dev), off, ln, c["rates"], None, TARGET, max(n_out) + 100)
    assert torch.equal(wide[:, :max(n_out)], a) and bool((wide[:, max(n_out):] == 0).all())
    same, n_same = ops.wave_resample(buf.to(dev), off, ln, [TARGET] * B, None, TARGET)
    assert n_same == ln.tolist() and torch.equal(same, ops.wave_unpack(buf.to(dev), off, ln))
    for bad in (dict(rates=[16001] + c["rates"][1:]), dict(rates=c["rates"][1:]), dict(n_out_max=max(n_out) - 1),
                dict(rates=[1000] + c["rates"][1:])):
        with pytest.raises(ValueError):
            ops.wave_resample(buf.to(dev), off, ln, bad.get("rates", c["rates"]), None, TARGET, bad.get("n_out_max"))


@pytest.mark.parametrize("what", ["table_slice_past_the_buffer", "misaligned_offset", "length_past_packed_elems", "src_index_out_of_range",
                                  "n_out_above_n_out_max", "ratio_outside_limits"])
def test_bad_rows_become_zero_rows(dev, what):
    """Rows outside the contract that the kernel is specified to survive: each is written as zeros, the other rows are what they were,
    and nothing around `out` is touched."""
    c = case()
    good = describe(c, dev)
    _, ref, _, _ = launch(good, dev)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    n_max = d["n_out_max"]
    if what == "table_slice_past_the_buffer":
        rows = [1, 14]                                               # the 44.1 kHz utterances: their table now ends 10 taps past the buffer
        for r in rows:
            d["base"][r] = d["tab_elems"] - int(d["L"][r]) * 2 * int(d["J"][r]) + 10
    elif what == "misaligned_offset":
        rows = [7]
        d["off"][7] += 4
    elif what == "length_past_packed_elems":
        rows = [15, 0]
        d["ln"][15] = d["buf"].numel() - int(d["off"][15]) + 1      # the last utterance: ends one sample past the buffer
        d["ln"][0] = -3
    elif what == "src_index_out_of_range":
        rows = [2, 9]
        d["src"][2], d["src"][9] = d["B"], -1
    elif what == "n_out_above_n_out_max":
        rows = [7]                                                   # the longest output
        d["n_out_max"] = n_max = sorted(c["n_out"])[-2]
    else:
        rows = [0, 3, 8]
        d["M"][0], d["L"][0] = 9, 1                                  # below 1/8
        d["L"][3] = 0
        d["J"][8] = 513
    _, out, whole, guard = launch(d, dev)
    for b in range(d["B"]):
        if b in rows:
            assert bool((out[b, :n_max] == 0).all()), b
        else:
            assert torch.equal(out[b, :n_max], ref[b, :n_max]), b
    assert bool((out[:, n_max:] == CANARY).all()) and guards_intact(whole, guard)


def test_rejected_arguments(dev):
    """Each returns non-zero, launches nothing and leaves the output as it was."""
    from asr_amd import _lib
    c = case()
    good = describe(c, dev)
    cases = [dict(dtype=2), dict(B=0), dict(B=65536), dict(n_out_max=-1), dict(n_out_max=2 ** 30 + 1), dict(ld=good["n_out_max"] - 1),
             dict(packed_elems=good["buf"].numel() - 4), dict(packed_elems=-8), dict(packed_elems=2 ** 31), dict(tab_elems=2 ** 22 + 1),
             dict(tab_elems=-1)]
    for bad in cases:
        d = dict(good)
        d.update(bad)
        if "n_out_max" in bad or "B" in bad:                         # (the canary buffer is sized from the good values)
            whole = torch.full((1 << 16,), CANARY, dtype=torch.float32, device=dev)
            meta = torch.zeros(7, max(good["B"], 1), dtype=torch.int32, device=dev)
            rc = _lib.load().ds2_wave_resample_f32(good["buf"].data_ptr(), good["buf"].numel(), 0, *[meta[i].data_ptr() for i in range(7)],
                                                   good["tab"].data_ptr(), good["tab_elems"], d["B"], d["n_out_max"], whole.data_ptr(),
                                                   2 ** 31, None)
            torch.cuda.synchronize()
            assert rc != 0, bad
        else:
            rc, out, whole, guard = launch(d, dev, expect_ok=False)
            assert rc != 0, bad
        assert bool((whole == CANARY).all()), bad
    # null and misaligned pointers
    lib = _lib.load()
    meta = torch.zeros(7, good["B"], dtype=torch.int32, device=dev)
    whole = torch.full((good["B"] * good["n_out_max"],), CANARY, dtype=torch.float32, device=dev)
    ok = [good["buf"].data_ptr(), good["buf"].numel(), 0, *[meta[i].data_ptr() for i in range(7)], good["tab"].data_ptr(), good["tab_elems"],
          good["B"], good["n_out_max"], whole.data_ptr(), good["n_out_max"], None]
    for i, v in ((0, None), (0, good["buf"].data_ptr() + 2), (3, None), (6, None), (9, None), (10, None), (10, good["tab"].data_ptr() + 2),
                 (14, None), (14, whole.data_ptr() + 2)):
        bad = list(ok)
        bad[i] = v
        assert lib.ds2_wave_resample_f32(*bad) != 0, (i, v)
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all())
    ok[13] = 0                                                       # n_out_max == 0: accepted, launches nothing
    assert lib.ds2_wave_resample_f32(*ok) == 0
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all())


# ---- the loader --------------------------------------------------------------------------------------------------------------------
RATES = (48000, 44100, 22050, 8000, 16000, 48000)
LENS = (9000, 7001, 3000, 2500, 4000, 1234)             # at 16 kHz: 3000, 2541, 2177, 5000, 4000, 412 samples: the sort differs from the raw one
TEXTS = ("a", "ab", "abc", "b", "bc", "c")


def _corpus(tmp_path, rates=RATES, stereo=()):
    import pandas as pd
    from scipy.io import wavfile
    rows = []
    for i, (sr, n) in enumerate(zip(rates, LENS)):
        y = np.stack([pcm(n, i), pcm(n, 50 + i)], axis=1) if i in stereo else pcm(n, i)
        wavfile.write(str(tmp_path / f"u{i}.wav"), sr, y)
        rows.append((str(tmp_path / f"u{i}.wav"), n / sr, 16000, TEXTS[i]))
    pd.DataFrame.from_records(rows, columns=["audio_filepath", "duration", "fq", "text"]).to_csv(tmp_path / "manifest.csv", index=False)
    pd.DataFrame({"label": ["_", "a", "b", "c"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def _epoch(c, labels, manifest, prefetch, resample, batch_size=6):
    from asr_amd.data import get_loader
    np.random.seed(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader, sampler = get_loader(c, labels, manifest, batch_size=batch_size, num_workers=0, front_end="gpu", prefetch=prefetch,
                                     resample=resample)
    np.random.seed(11)
    return list(loader)


def _same(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("kind", ["int16", "fp32"])
def test_loader_with_resample(dev, tmp_path, kind):
    """Six short WAVs at mixed rates (fp32: one of them stereo, so the batch is packed as float32).  prefetch=2 and prefetch=0 give the
    same bits; the batch is the plain front-end's spectrogram of the oracle-resampled waveforms, sorted by their 16 kHz frame counts,
    within 2e-4: the bar the loader tests of this suite hold normalised spectrograms of one waveform made two ways to (2e-5 x 10) — the
    device waveform differs from the oracle's by fp32 rounding only."""
    from asr_amd import ops
    from asr_amd.data import _read_wav
    manifest, labels = _corpus(tmp_path, stereo=(2,) if kind == "fp32" else ())
    sync = _epoch(conf(), labels, manifest, 0, True)
    ahead = _epoch(conf(), labels, manifest, 2, True)
    assert len(sync) == len(ahead) == 1 and _same(sync[0], ahead[0])
    x, targets, pct, sizes = sync[0]
    waves = []
    for i, sr in enumerate(RATES):
        y, _ = R.resample(_read_wav(str(tmp_path / f"u{i}.wav"))[1], sr, TARGET)
        waves.append(y.astype(np.float32))
    n16 = [len(w) for w in waves]
    assert n16 == [3000, 2541, 2177, 5000, 4000, 412]
    order = sorted(range(6), key=lambda i: 1 + n16[i] // 160, reverse=True)
    assert order == [3, 4, 0, 1, 2, 5]
    batch = torch.zeros(6, max(n16))
    for b, i in enumerate(order):
        batch[b, :n16[i]] = torch.from_numpy(waves[i])
    ref, frames = ops.spectrogram(batch.to(dev), torch.tensor([n16[i] for i in order]), 320, 160, "hamming", "constant", True)
    assert x.is_cuda and x.shape == ref.shape == (6, 1, 161, 32)
    diff = float((x - ref).abs().max())
    print("loader vs oracle-resampled spectrogram:", diff)
    assert diff < 2e-4
    assert pct.tolist() == [float(np.float32(min(1 + n16[i] // 160, 32) / 32.0)) for i in order]
    assert sizes.tolist() == [len(TEXTS[i]) for i in order]
    assert targets.tolist() == [" abc".index(ch) for i in order for ch in TEXTS[i]]
    with pytest.raises(ValueError, match="expected 16000 Hz audio"):                     # the default still refuses the corpus
        _epoch(conf(), labels, manifest, 0, False)


def test_loader_all_at_target_rate_is_unchanged(dev, tmp_path):
    manifest, labels = _corpus(tmp_path, rates=(TARGET,) * 6)
    for prefetch in (0, 2):
        base = _epoch(conf(), labels, manifest, prefetch, False, batch_size=3)
        got = _epoch(conf(), labels, manifest, prefetch, True, batch_size=3)
        assert len(base) == len(got) == 2
        for a, b in zip(got, base):
            assert _same(a, b)
