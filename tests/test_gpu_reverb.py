"""-m gpu: reverberation of the waveform batch — the kernel (ds2_reverb_f32) against the fp64 oracle (tests/reverb_oracle.py) through the
C ABI, its exact properties, rows and arguments outside the contract, and get_loader(front_end="gpu") with audio_conf.rir_dir."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import reverb_oracle as V

pytestmark = pytest.mark.gpu

CANARY = 7.5
U = 2.0 ** -24


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


def taps_of(P, seed):
    """P fp32 taps, each 0 or at least 2^-40 in magnitude (no denormal can arise from int16 PCM x 2^-15 times such taps)."""
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal(P) * np.exp(-np.arange(P) / max(P / 4.0, 1.0)) / np.sqrt(max(P / 4.0, 1.0))).astype(np.float32)
    h[np.abs(h) < 2.0 ** -40] = 0.0
    if P:
        h[0], h[-1] = 0.75, -2.0 ** -7                   # both ends count
    return h


def unit(d):
    h = np.zeros(d + 1, np.float32)
    h[d] = 1.0
    return h


_CASE = {}


def case():
    """The batch of the kernel tests and the oracle's result: computed once, shared, never modified."""
    if not _CASE:
        from asr_amd import _lib
        lib = _lib.load()
        tile, chunk, max_taps = lib.ds2_reverb_tile_samples(), lib.ds2_reverb_tap_chunk(), lib.ds2_reverb_max_taps()
        big = 3 * tile + 1
        # (n, taps): every n of {0, 1, 5, tile - 1, tile, tile + 1, 3 tile + 1}, every P of {0, 1 .. 5, 15, 16, 17, chunk - 1, chunk,
        # chunk + 1, 2 chunk + 1, max_taps}; rows 6, 7, 8, 24 have P > n; max_taps goes with n = tile + 1
        plan = [(big, 0), (big, 1), (tile + 1, 2), (tile, 3), (tile - 1, 4), (5, 5), (5, 15), (1, 16), (0, 17), (tile + 1, 17),
                (big, chunk - 1), (tile, chunk), (tile + 1, chunk + 1), (big, 2 * chunk + 1), (tile + 1, max_taps), (tile - 1, 15),
                (big, 16), (big, unit(0)), (tile + 1, unit(1)), (big, unit(3)), (tile + 1, unit(17)), (big, unit(chunk)),
                (tile + 1, np.array([0.5], np.float32)), (1, 1), (5, 2 * chunk + 1)]
        hs = [taps_of(p, 100 + i) if isinstance(p, int) else p for i, (_, p) in enumerate(plan)]
        xs = [pcm(n, 40 + i).astype(np.float32) / 32768.0 for i, (n, _) in enumerate(plan)]
        ref = [V.reverb(x, h) for x, h in zip(xs, hs)]
        lengths = np.array([len(h) for h in hs], np.int64)
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        _CASE.update(xs=xs, hs=hs, ref=ref, n=np.array([len(x) for x in xs], np.int64), taps=lengths, base=starts,
                     bank=np.concatenate(hs).astype(np.float32), tile=tile, chunk=chunk, max_taps=max_taps, n_max=big, B=len(plan),
                     exact=dict(one=17, d1=18, d3=19, d17=20, dchunk=21, half=22, passthrough=0))
    return _CASE


def describe(c, dev, rows=None, n_max=None):
    """The arguments of the C entry point for (a selection of rows of) the shared batch: audio rows hold NaN from n_b on."""
    rows = list(range(c["B"])) if rows is None else list(rows)
    n_max = c["n_max"] if n_max is None else n_max
    audio = np.full((len(rows), n_max + 3), np.nan, np.float32)
    for b, r in enumerate(rows):
        audio[b, :c["n"][r]] = c["xs"][r]
    return dict(audio=torch.from_numpy(audio).to(dev), n=c["n"][rows].copy(), base=c["base"][rows].copy(), taps=c["taps"][rows].copy(),
                rir=torch.from_numpy(c["bank"]).to(dev), rir_elems=len(c["bank"]), B=len(rows), n_max=n_max)


def launch(d, dev, extra=5, expect_ok=True):
    """One call through the C ABI into the middle of a canary-filled buffer: (rc, out (B, n_max + extra) view, the whole buffer, guard)."""
    from asr_amd import _lib
    B, n_max = d["B"], d["n_max"]
    ld, guard = n_max + extra, 4096
    whole = torch.full((guard + B * ld + guard,), CANARY, dtype=torch.float32, device=dev)
    out = whole[guard:guard + B * ld].view(B, ld)
    n_dev = torch.from_numpy(d["n"].astype(np.int32)).to(dev)
    taps_dev = torch.from_numpy(d["taps"].astype(np.int32)).to(dev)
    base_dev = torch.from_numpy(d["base"].astype(np.int64)).to(dev)
    rc = _lib.load().ds2_reverb_f32(d["audio"].data_ptr(), d.get("ld_audio", d["audio"].stride(0)), n_dev.data_ptr(),
                                    d["rir"].data_ptr() if d["rir"] is not None else None, d["rir_elems"], base_dev.data_ptr(),
                                    taps_dev.data_ptr(), d.get("B_arg", B), d.get("n_max_arg", n_max), out.data_ptr(), d.get("ld", ld), None)
    torch.cuda.synchronize()
    assert (rc == 0) == expect_ok, _lib.load().ds2_last_error()
    return rc, out, whole, guard


def guards_intact(whole, guard):
    return bool((whole[:guard] == CANARY).all()) and bool((whole[-guard:] == CANARY).all())


def test_kernel_vs_oracle(dev):
    """Every sample of every row: |y_dev - y_fp64| <= gamma A[i], gamma = (P + 1) u / (1 - (P + 1) u), u = 2^-24: the bound of a length-P
    fp32 dot product in any order (samples and taps are fp32 numbers the oracle is given as they are).  Exact: h = [1] returns x, a single
    1.0 at lag d returns x delayed by d, h = [0.5] returns x / 2, P = 0 returns x; zeros in [n_b, n_max), the canary beyond n_max and in
    the guards, no NaN anywhere (the audio rows hold NaN from n_b on).  A rerun and ops.reverb give the same bits."""
    from asr_amd import ops
    c = case()
    d = describe(c, dev)
    _, out, whole, guard = launch(d, dev)
    assert not bool(torch.isnan(whole).any())
    got = out.cpu().numpy().astype(np.float64)
    n_max = d["n_max"]
    worst = 0.0
    for b, (y, A) in enumerate(c["ref"]):
        n, P = len(y), int(c["taps"][b])
        if P == 0:
            assert np.array_equal(got[b, :n], y), b
        else:
            g = (P + 1) * U / (1 - (P + 1) * U)
            err, bound = np.abs(got[b, :n] - y), g * A
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0)
            assert (err <= bound).all(), (b, n, P, int(np.argmax(err - bound)), float((err - bound).max()))
        assert (got[b, n:n_max] == 0).all(), b                           # exact zeros beyond n_b
        assert n == 0 or np.abs(got[b, :n]).max() > 0
    print("largest |error| / bound:", worst)
    assert bool((out[:, n_max:] == CANARY).all()) and guards_intact(whole, guard)          # columns beyond n_max are untouched
    e = c["exact"]
    x = lambda r: torch.from_numpy(c["xs"][r]).to(dev)                   # noqa: E731
    for r in (e["one"], e["passthrough"]):
        assert torch.equal(out[r, :c["n"][r]], x(r)), r
    for r, lag in ((e["d1"], 1), (e["d3"], 3), (e["d17"], 17), (e["dchunk"], c["chunk"])):
        n = int(c["n"][r])
        assert bool((out[r, :lag] == 0).all()) and torch.equal(out[r, lag:n], x(r)[:n - lag]), (r, lag)
    assert torch.equal(out[e["half"], :c["n"][e["half"]]], x(e["half"]) / 2)
    _, again, _, _ = launch(d, dev)
    assert torch.equal(again, out)                                      # a rerun
    via = ops.reverb(d["audio"], d["n"], d["rir"], d["base"], d["taps"])
    assert via.shape == (d["B"], n_max) and torch.equal(via, out[:, :n_max])
    wide = ops.reverb(d["audio"], d["n"], d["rir"], d["base"], d["taps"], n_max + 3)
    assert torch.equal(wide[:, :n_max], via) and bool((wide[:, n_max:] == 0).all())
    for bad in (dict(n=d["n"] + n_max), dict(taps=d["taps"] + c["max_taps"]), dict(base=d["base"] + 1), dict(base=d["base"] - 1),
                dict(n=d["n"][1:]), dict(n_max=n_max - 1), dict(n_max=n_max + 4)):
        with pytest.raises(ValueError):
            ops.reverb(d["audio"], bad.get("n", d["n"]), d["rir"], bad.get("base", d["base"]), bad.get("taps", d["taps"]), bad.get("n_max"))


def test_bits_depend_on_the_row_alone(dev):
    """The same (x, h) gives the same bits as another row of a permuted batch, in a batch of one, and under a larger n_max."""
    c = case()
    _, ref, _, _ = launch(describe(c, dev), dev)
    order = list(np.random.default_rng(5).permutation(c["B"]))
    order[3] = order[9]                                                 # a repeat
    _, out, whole, guard = launch(describe(c, dev, rows=order), dev)
    assert torch.equal(out[:, :c["n_max"]], ref[order, :c["n_max"]]) and guards_intact(whole, guard)
    for r in (13, 14, 10, 6):
        _, one, whole, guard = launch(describe(c, dev, rows=[r]), dev)
        assert torch.equal(one[0, :c["n_max"]], ref[r, :c["n_max"]]) and guards_intact(whole, guard), r
    big = c["n_max"] + c["tile"] + 7
    _, out, whole, guard = launch(describe(c, dev, n_max=big), dev)
    assert torch.equal(out[:, :c["n_max"]], ref[:, :c["n_max"]]) and bool((out[:, c["n_max"]:big] == 0).all())
    assert bool((out[:, big:] == CANARY).all()) and guards_intact(whole, guard)


@pytest.mark.parametrize("what", ["taps_past_the_bank", "negative_base", "taps_above_max", "negative_n", "n_above_n_max"])
def test_bad_rows_become_zero_rows(dev, what):
    """Rows outside the contract that the kernel is specified to survive: each is written as zeros, the other rows are what they were,
    and nothing around `out` is touched."""
    c = case()
    good = describe(c, dev)
    _, ref, _, _ = launch(good, dev)
    d = dict(good)
    for k in ("n", "base", "taps"):
        d[k] = good[k].copy()
    n_max = d["n_max"]
    if what == "taps_past_the_bank":
        rows = [24, 13]                                                 # the last response, and one that now ends one tap past the bank
        d["base"][24] += 1
        d["base"][13] = d["rir_elems"] - int(d["taps"][13]) + 1
    elif what == "negative_base":
        rows = [1, 10]
        d["base"][1], d["base"][10] = -1, -(2 ** 40)
    elif what == "taps_above_max":
        rows = [2]
        d["base"][2], d["taps"][2] = 0, c["max_taps"] + 1                # (inside the bank: only the tap limit refuses it)
        assert d["taps"][2] <= d["rir_elems"]
    elif what == "negative_n":
        rows = [3, 0]
        d["n"][3], d["n"][0] = -1, -(2 ** 31)
    else:
        d["n_max"] = n_max = c["n_max"] - 1
        rows = [r for r in range(d["B"]) if d["n"][r] > n_max]          # the longest rows
        assert 2 <= len(rows) < d["B"] // 2
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
    good = describe(c, dev, rows=[5, 6, 7])
    good["n_max"] = 5
    for bad in (dict(B_arg=0), dict(B_arg=65536), dict(n_max_arg=-1), dict(n_max_arg=2 ** 30 + 1), dict(ld=4), dict(ld_audio=4),
                dict(rir_elems=-1), dict(rir_elems=2 ** 31), dict(rir=None)):
        d = dict(good)
        d.update(bad)
        if "n_max_arg" in bad:
            d["ld"] = d["ld_audio"] = 2 ** 31
        rc, out, whole, guard = launch(d, dev, expect_ok=False)
        assert rc != 0 and bool((whole == CANARY).all()), bad
    # null and misaligned pointers
    lib = _lib.load()
    n_dev = torch.from_numpy(good["n"].astype(np.int32)).to(dev)
    taps_dev = torch.from_numpy(good["taps"].astype(np.int32)).to(dev)
    base_dev = torch.from_numpy(good["base"].astype(np.int64)).to(dev)
    whole = torch.full((3 * 5,), CANARY, dtype=torch.float32, device=dev)
    ok = [good["audio"].data_ptr(), good["audio"].stride(0), n_dev.data_ptr(), good["rir"].data_ptr(), good["rir_elems"], base_dev.data_ptr(),
          taps_dev.data_ptr(), 3, 5, whole.data_ptr(), 5, None]
    for i, v in ((0, None), (0, ok[0] + 2), (2, None), (2, ok[2] + 2), (3, None), (3, ok[3] + 2), (5, None), (5, ok[5] + 4), (6, None),
                 (6, ok[6] + 2), (9, None), (9, ok[9] + 2), (9, ok[0])):
        bad = list(ok)
        bad[i] = v
        assert lib.ds2_reverb_f32(*bad) != 0, (i, v)
    torch.cuda.synchronize()
    assert bool((whole == CANARY).all())
    ok[8] = 0                                                           # n_max == 0: accepted, launches nothing
    assert lib.ds2_reverb_f32(*ok) == 0
    ok[8], ok[3], ok[4] = 5, None, 0                                    # no bank at all is fine when no row has taps
    taps_dev.zero_()
    base_dev.zero_()
    assert lib.ds2_reverb_f32(*ok) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole.view(3, 5)[0], good["audio"][0, :5]) and bool((whole.view(3, 5)[2, 1:] == 0).all())


# ---- the loader --------------------------------------------------------------------------------------------------------------------
LENS = (3000, 2541, 400, 5000, 4000, 1234)
TEXTS = ("a", "ab", "abc", "b", "bc", "c")


def _corpus(tmp_path):
    import pandas as pd
    from scipy.io import wavfile
    rows = []
    for i, n in enumerate(LENS):
        wavfile.write(str(tmp_path / f"u{i}.wav"), 16000, pcm(n, i))
        rows.append((str(tmp_path / f"u{i}.wav"), n / 16000, 16000, TEXTS[i]))
    pd.DataFrame.from_records(rows, columns=["audio_filepath", "duration", "fq", "text"]).to_csv(tmp_path / "manifest.csv", index=False)
    pd.DataFrame({"label": ["_", "a", "b", "c"]}).to_csv(tmp_path / "labels.csv", index=False)
    return str(tmp_path / "manifest.csv"), str(tmp_path / "labels.csv")


def _rirs(tmp_path):
    """Three RIR files: a few samples before the direct path, then decaying noise; at most 256 taps after the preparation."""
    from scipy.io import wavfile
    (tmp_path / "rir").mkdir()
    for i, (lead, tau) in enumerate(((0, 12.0), (5, 20.0), (2, 30.0))):
        rng = np.random.default_rng(70 + i)
        h = rng.standard_normal(300) * np.exp(-np.arange(300) / tau) * 6000
        h[0] = 20000
        wavfile.write(str(tmp_path / "rir" / f"r{i}.wav"), 16000, np.concatenate([rng.standard_normal(lead) * 300, h]).astype(np.int16))
    return str(tmp_path / "rir")


def _noise(tmp_path):
    from scipy.io import wavfile
    (tmp_path / "noise").mkdir()
    for i, n in enumerate((7000, 2000)):
        wavfile.write(str(tmp_path / "noise" / f"n{i}.wav"), 16000, pcm(n, 90 + i))
    return str(tmp_path / "noise")


def _epoch(c, labels, manifest, prefetch, batch_size=6):
    from asr_amd.data import get_loader
    np.random.seed(4)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader, sampler = get_loader(c, labels, manifest, batch_size=batch_size, num_workers=0, front_end="gpu", prefetch=prefetch)
    np.random.seed(11)
    return list(loader), loader.front_end


def _same(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(a, b))


def reference_waves(tmp_path, bank, file, order, dtype=np.float64):
    """The corpus in batch order, utterance b convolved (oracle; in `dtype`) with the response `file[b]` names, rounded to fp32."""
    from asr_amd.data import _read_wav
    waves = []
    for b, i in enumerate(order):
        x = _read_wav(str(tmp_path / f"u{i}.wav"))[1]
        if file[b] >= 0:
            h = bank.taps[bank.starts[file[b]]:bank.starts[file[b]] + bank.lengths[file[b]]]
            x = np.convolve(x.astype(dtype), h.astype(dtype))[:len(x)] if dtype != np.float64 else V.reverb(x, h)[0]
        waves.append(x.astype(np.float32))
    return waves


ORDER = sorted(range(6), key=lambda i: 1 + LENS[i] // 160, reverse=True)


def _batch(waves, dev):
    n = [len(w) for w in waves]
    batch = torch.zeros(len(waves), max(n))
    for b, w in enumerate(waves):
        batch[b, :n[b]] = torch.from_numpy(w)
    return batch.to(dev), torch.tensor(n)


def test_loader_with_reverb(dev, tmp_path):
    """Six short WAVs and an rir_dir of three responses (75, 134 and 200 taps after the preparation), reverb_prob = 1, noise and masks off.
    prefetch=2 and prefetch=0 give the same bits; the batch is the plain front-end's spectrogram of the ORACLE-reverberated waveforms —
    the files draw_reverb names for the same seed, in the sorted order — within 2e-4: the bar this suite holds normalised spectrograms of
    one waveform made two ways to (2e-5 x 10).  The reference route alone — fp64 against fp32 numpy convolution through the host
    spectrogram with the loader's normalisation — differs by 8.4e-7 on this corpus (tests/test_cpu_reverb.py checks < 2e-5)."""
    from asr_amd import ops
    from asr_amd.data import draw_reverb
    manifest, labels = _corpus(tmp_path)
    c = conf(rir_dir=_rirs(tmp_path), reverb_prob=1.0)
    sync, fe = _epoch(c, labels, manifest, 0)
    ahead, _ = _epoch(c, labels, manifest, 2)
    assert len(sync) == len(ahead) == 1 and _same(sync[0], ahead[0])
    bank = fe.reverb
    assert len(bank) == 3 and bank.lengths.max() <= 256 and bank.lengths.min() >= 16
    file, _, _ = draw_reverb(np.random.default_rng(fe.seed), 6, bank, 1.0)
    assert (file >= 0).all() and ORDER == [3, 4, 0, 1, 5, 2]
    x, targets, pct, sizes = sync[0]
    batch, n = _batch(reference_waves(tmp_path, bank, file, ORDER), dev)
    ref, _ = ops.spectrogram(batch, n, 320, 160, "hamming", "constant", True)
    assert x.is_cuda and x.shape == ref.shape == (6, 1, 161, 32)
    diff = float((x - ref).abs().max())
    print("loader vs oracle-reverberated spectrogram:", diff)
    assert diff < 2e-4
    plain, _ = ops.spectrogram(*_batch(reference_waves(tmp_path, bank, np.full(6, -1), ORDER), dev), 320, 160, "hamming", "constant", True)
    assert float((x - plain).abs().max()) > 0.1                        # (the reverberation is there)
    assert pct.tolist() == [float(np.float32(min(1 + LENS[i] // 160, 32) / 32.0)) for i in ORDER]
    assert sizes.tolist() == [len(TEXTS[i]) for i in ORDER]
    assert targets.tolist() == [" abc".index(ch) for i in ORDER for ch in TEXTS[i]]


def test_loader_without_reverb_is_unchanged(dev, tmp_path):
    manifest, labels = _corpus(tmp_path)
    rir = _rirs(tmp_path)
    for prefetch in (0, 2):
        base, fe = _epoch(conf(), labels, manifest, prefetch)
        assert fe.reverb is None
        for c in (conf(rir_dir=rir, reverb_prob=0.0), conf(rir_dir=None, reverb_prob=1.0)):
            got, _ = _epoch(c, labels, manifest, prefetch)
            assert len(base) == len(got) == 1 and _same(got[0], base[0])


def test_loader_with_reverb_and_noise(dev, tmp_path):
    """Reverb and a noise bank both on: the batch equals ops.spectrogram_augmented given the oracle-reverberated waveforms and the same
    noise draws, within the same bar — the noise is scaled by the rms of the REVERBERATED signal."""
    from asr_amd import ops
    from asr_amd.data import draw_augmentation, draw_reverb
    manifest, labels = _corpus(tmp_path)
    c = conf(rir_dir=_rirs(tmp_path), reverb_prob=1.0, noise_dir=_noise(tmp_path), noise_prob=1.0, noise_levels=(0.2, 0.5))
    got, fe = _epoch(c, labels, manifest, 0)
    rng = np.random.default_rng(fe.seed)
    file, _, _ = draw_reverb(rng, 6, fe.reverb, 1.0)
    n = [LENS[i] for i in ORDER]
    p = draw_augmentation(rng, n, 160, 161, fe.noise, 1.0)
    assert (p["file"] >= 0).all() and (p["level"] >= 0.2).all()
    batch, n_t = _batch(reference_waves(tmp_path, fe.reverb, file, ORDER), dev)
    ref, _ = ops.spectrogram_augmented(batch, n_t, 320, 160, "hamming", "constant", True, noise=fe.noise.device_samples(dev),
                                       noise_base=p["base"], noise_period=p["period"], noise_start=p["start"], noise_level=p["level"])
    diff = float((got[0][0] - ref).abs().max())
    print("loader vs oracle-reverberated noisy spectrogram:", diff)
    assert diff < 2e-4
    dry, _ = ops.spectrogram_augmented(*_batch(reference_waves(tmp_path, fe.reverb, np.full(6, -1), ORDER), dev), 320, 160, "hamming",
                                       "constant", True, noise=fe.noise.device_samples(dev), noise_base=p["base"],
                                       noise_period=p["period"], noise_start=p["start"], noise_level=p["level"])
    assert float((got[0][0] - dry).abs().max()) > 0.1


def test_front_end_with_a_synthetic_bank(dev):
    from asr_amd import ops
    from asr_amd.data import GpuSpectrogramFrontEnd, ImpulseResponses, draw_reverb
    bank = ImpulseResponses.synthetic(3, t60_range=(0.01, 0.02), max_seconds=0.012, seed=3)
    assert bank.lengths.max() <= 192
    fe = GpuSpectrogramFrontEnd(conf(reverb_prob=0.6), normalize=True, device=dev, augment=True, seed=21, reverb=bank)
    waves = [pcm(n, 30 + i).astype(np.float32) / 32768.0 for i, n in enumerate((4000, 3000, 2500, 1000, 161))]
    spect, pct = fe(waves)
    file, _, _ = draw_reverb(np.random.default_rng(21), 5, bank, 0.6)
    assert 0 < (file >= 0).sum() < 5                                   # some utterances pass through
    want = [V.reverb(w, bank.taps[bank.starts[f]:bank.starts[f] + bank.lengths[f]])[0].astype(np.float32) if f >= 0 else w
            for w, f in zip(waves, file)]
    ref, frames = ops.spectrogram(*_batch(want, dev), 320, 160, "hamming", "constant", True)
    diff = float((spect - ref).abs().max())
    print("front-end with a synthetic bank vs oracle:", diff)
    assert diff < 2e-4 and pct.tolist() == (frames.float() / 26.0).tolist()
