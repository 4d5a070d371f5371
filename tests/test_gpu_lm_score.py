"""-m gpu: the LM scoring kernel (ds2_lm_score_seqs, ops.lm_score) against its host twin, which tests/test_cpu_lm_score.py holds to the
plain-Python restatement: n_tok and n_oov to the integer, lm_sum to the bit; and the grid sweep (ds2_nbest_sweep, ops.nbest_sweep)
against a float32 NumPy restatement: picks and totals to the integer.  MI355X figures are in profiles/rescore_timing.txt."""
import math
import tempfile
import pathlib

import numpy as np
import pytest
import torch

import lm_score_oracle as SO
from test_cpu_lm_score import CASES, host_score, make_lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lm_dir():
    with tempfile.TemporaryDirectory() as d:
        yield pathlib.Path(d)


def device_score(dev, lm, seqs, max_len=None, pad=0):
    """ops.lm_score on a list of label lists, packed flat with `pad` unused labels between them -> three NumPy arrays"""
    from asr_amd import ops
    flat, off = [], []
    for s in seqs:
        off.append(len(flat))
        flat += list(s) + [1] * pad
    flat.append(1)                                              # (never an empty buffer)
    lens = [len(s) for s in seqs]
    max_len = max(lens, default=0) if max_len is None else max_len
    out = ops.lm_score(torch.tensor(flat, dtype=torch.int32, device=dev), torch.tensor(off, dtype=torch.int64, device=dev),
                       torch.tensor(lens, dtype=torch.int32, device=dev), lm, max_len)
    return tuple(t.cpu().numpy() for t in out)


def same(got, want):
    """three outputs against (lm_sum float32, n_tok, n_oov): the integers equal, lm_sum equal to the bit (NaN matches NaN)"""
    s, nt, no = got
    return (nt, no) == want[1:] and (np.float32(s).tobytes() == np.float32(want[0]).tobytes() or (math.isnan(s) and math.isnan(want[0])))


@pytest.mark.parametrize("mode,order", CASES)
def test_kernel_matches_host_twin(dev, lm_dir, mode, order):
    lm, _ = make_lm(lm_dir, mode, order)
    names, seqs = zip(*SO.sequences(mode, order))
    s, nt, no = device_score(dev, lm, seqs)
    for p, (name, labels) in enumerate(zip(names, seqs)):
        want = host_score(lm, labels)[1:]
        assert same((s[p], int(nt[p]), int(no[p])), want), (name, s[p], nt[p], no[p], want)
    assert no.max() > 0 and nt.max() > 64


@pytest.mark.parametrize("mode,order", [("word", 3), ("char", 6)])
def test_outputs_do_not_depend_on_the_batch(dev, lm_dir, mode, order):
    lm, _ = make_lm(lm_dir, mode, order)
    by_name = dict(SO.sequences(mode, order))
    others = [v for v in by_name.values()]
    for name in ("words129", "many words", "long word", "random300"):
        seq = by_name[name]
        alone = tuple(a[0] for a in device_score(dev, lm, [seq]))
        assert same((alone[0], int(alone[1]), int(alone[2])), host_score(lm, seq)[1:]), name
        longest = max(len(v) for v in others)
        for pos, max_len, pad in ((0, longest, 0), (17, longest + 1, 3), (39, 4096, 1)):
            batch = (others * 2)[:39]
            batch.insert(pos, seq)
            got = device_score(dev, lm, batch, max_len=max_len, pad=pad)
            assert len(batch) == 40 and tuple(a[pos].tobytes() for a in got) == tuple(a.tobytes() for a in alone), (name, pos)


def test_refused_sequences_leave_their_neighbours_alone(dev, lm_dir):
    lm, _ = make_lm(lm_dir, "word", 3)
    good = [SO.spell("AB CAB DE"), SO.spell("EDA BAD"), SO.spell("CAB " * 25), []]                      # (100 labels: exactly max_len)
    bad = [SO.spell("AB") + [SO.BLANK] + SO.spell("CAB"), [7, 1, 2], [1, -1], SO.spell("A " * 60)]     # the last one: longer than max_len
    batch = [bad[0], good[0], bad[1], good[1], bad[2], good[2], bad[3], good[3]]
    s, nt, no = device_score(dev, lm, batch, max_len=100)
    for p, labels in enumerate(batch):
        if p % 2 == 0:
            assert math.isnan(s[p]) and nt[p] == -1 and no[p] == -1, p
        else:
            assert same((s[p], int(nt[p]), int(no[p])), host_score(lm, labels)[1:]), p
    # a range that leaves the label buffer
    from asr_amd import ops
    flat = torch.tensor(good[0], dtype=torch.int32, device=dev)
    out = ops.lm_score(flat, torch.tensor([0, 4, -1], dtype=torch.int64, device=dev),
                       torch.tensor([len(good[0]), len(good[0]), 2], dtype=torch.int32, device=dev), lm, 100)
    s, nt, no = (t.cpu().numpy() for t in out)
    assert same((s[0], int(nt[0]), int(no[0])), host_score(lm, good[0])[1:])
    assert math.isnan(s[1]) and math.isnan(s[2]) and nt[1:].tolist() == [-1, -1] and no[1:].tolist() == [-1, -1]
    # a corrupted header is refused with a message, before any launch
    from asr_amd._lib import DS2LibraryError

    class Broken:
        pass
    broken = Broken()
    broken.__dict__.update(lm.__dict__)
    broken.packed = lm.packed.copy()
    broken.packed.view(np.int32)[0] = 0
    broken.device_tables = lm.device_tables
    with pytest.raises(DS2LibraryError, match="not a packed language model"):
        ops.lm_score(flat, torch.zeros(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev), broken, 4)
    with pytest.raises(ValueError, match="int64"):
        ops.lm_score(flat, torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev), lm, 4)


def sweep_reference(ac, lm_sum, n_tok, n_oov, err, oov_score, alphas, betas):
    """ds2_nbest_sweep in float32 NumPy, every operation rounded on its own -> (pick (Ga,Gb,N), total (Ga,Gb,R))"""
    f = np.float32
    N = ac.shape[0]
    pick = np.zeros((len(alphas), len(betas), N), np.int32)
    total = np.zeros((len(alphas), len(betas), err.shape[2]), np.int64)
    with np.errstate(all="ignore"):
        lm = lm_sum + f(oov_score) * n_oov.astype(f)
        for i, a in enumerate(alphas):
            for j, b in enumerate(betas):
                s = (ac + f(a) * lm) + f(b) * n_tok.astype(f)
                assert s.dtype == np.float32
                s = np.where(np.isnan(s), f(-np.inf), s)
                pick[i, j] = np.argmax(s, axis=1)             # the first of equal maxima; slot 0 when every slot is -inf
                total[i, j] = err[np.arange(N), pick[i, j]].sum(axis=0, dtype=np.int64)
    return pick, total


def sweep_problem(N, K, R, seed):
    """features on a coarse lattice of values, so that exact ties are common, with planted duplicates, -inf rows and NaN slots"""
    rng = np.random.default_rng(seed)
    ac = (-rng.integers(0, 40, size=(N, K)) * 0.5).astype(np.float32)
    lm_sum = (-rng.integers(0, 24, size=(N, K)) * 0.25).astype(np.float32)
    n_tok = rng.integers(0, 6, size=(N, K)).astype(np.int32)
    n_oov = (rng.random((N, K)) < 0.2).astype(np.int32) * rng.integers(1, 3, size=(N, K)).astype(np.int32)
    err = rng.integers(0, 50, size=(N, K, R)).astype(np.int32)
    for n in range(N):
        kind = n % 5
        if kind == 1 and K > 1:                                # a duplicate of some slot, later in the list: an exact tie
            i, j = sorted(rng.choice(K, size=2, replace=False))
            ac[n, j], lm_sum[n, j], n_tok[n, j], n_oov[n, j] = ac[n, i], lm_sum[n, i], n_tok[n, i], n_oov[n, i]
        elif kind == 2:
            ac[n] = -np.inf                                    # no surviving slot: slot 0
        elif kind == 3:
            lm_sum[n, rng.integers(0, K)] = np.nan             # a refused sequence: never picked
            n_tok[n, rng.integers(0, K)] = -1
        elif kind == 4:
            ac[n, rng.integers(0, K):] = -np.inf               # empty slots at the end of the list
    return ac, lm_sum, n_tok, n_oov, err


@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 100])
def test_sweep_matches_float32_numpy(dev, N, K):
    from asr_amd import ops
    R = 2
    ac, lm_sum, n_tok, n_oov, err = sweep_problem(N, K, R, seed=1000 * N + K)
    t = [torch.from_numpy(a).to(dev) for a in (ac, lm_sum, n_tok, n_oov, err)]
    moved = 0
    for alphas, betas, oov in (([0.5], [0.25], -1000.0), ([0.0, 1.5, -0.5], [0.0, -1.0, 0.5, 2.0], -7.5)):
        pick, total = ops.nbest_sweep(*t, alphas, betas, oov)
        want_pick, want_total = sweep_reference(ac, lm_sum, n_tok, n_oov, err, oov, alphas, betas)
        assert pick.dtype == torch.int32 and total.dtype == torch.int64
        assert np.array_equal(pick.cpu().numpy(), want_pick), (N, K, alphas)
        assert np.array_equal(total.cpu().numpy(), want_total), (N, K, alphas)
        none, total2 = ops.nbest_sweep(*t, alphas, betas, oov, want_pick=False)
        assert none is None and torch.equal(total, total2)
        moved += int((want_pick > 0).sum())
    assert K == 1 or N == 1 or moved > 0                      # (the picks are not all slot 0)


def test_sweep_ties_and_dead_rows_are_exercised(dev):
    """the planted cases do occur at the sizes above: an exact tie between two slots at the top, a row of -inf, a NaN slot"""
    from asr_amd import ops
    ac = np.array([[-1.0, -1.0, -2.0], [-np.inf] * 3, [-3.0, -1.0, -1.0], [-1.0, np.nan, -0.5]], np.float32)
    z = np.zeros_like(ac)
    err = np.arange(12, dtype=np.int32).reshape(4, 3, 1)
    pick, total = ops.nbest_sweep(*(torch.from_numpy(a).to(dev) for a in (ac, z, z.astype(np.int32), z.astype(np.int32), err)), [1.0], [0.0])
    assert pick.view(-1).tolist() == [0, 0, 1, 2] and total.view(-1).tolist() == [0 + 3 + 7 + 11]
    with pytest.raises(ValueError, match="err must be"):
        ops.nbest_sweep(*(torch.from_numpy(a).to(dev) for a in (ac, z, z.astype(np.int32), z.astype(np.int32), err[:, :2].copy())), [1.0], [0.0])
