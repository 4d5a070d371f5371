"""No GPU: the fp64 restatement of the wildcard CTC loss (tests/ctc_star_loss_oracle.py) against a brute-force enumeration of state paths
and against torch's own CTC over C + 1 classes with a constant last column; the host rules (decoders.wildcard_ends, CTCLoss's
constructor and target preparation, the datasets' `star`)."""
import math

import numpy as np
import pytest
import torch

import ctc_star_loss_oracle as O
import det

C = 4                                           # classes 0 .. 3, the wildcard is the id 4


def _problems():
    """(T, labels, flag) for T <= 6, U <= 3, every flag value, wildcards in every position, repeated labels."""
    targets = [[], [2], [C], [1, 1], [1, C], [C, 3], [C, C], [2, 3], [1, C, 1], [C, 2, C], [3, 3, C], [1, 2, 3], [C, C, 2], [2, C, C]]
    return [(T, lab, flag) for T in range(1, 7) for lab in targets for flag in range(4)]


def _logits(T, seed):
    return det.unitvar((T, C), seed).astype(np.float64) * 2.0


def test_oracle_equals_brute_force_over_state_paths():
    worst, n_inf = 0.0, 0
    for k, (T, lab, flag) in enumerate(_problems()):
        em = O.extended_emissions(_logits(T, 11 + k), math.log(0.5))
        _, _, nll = O.lattice(em, lab, flag)
        want = O.brute_force_nll(em, lab, flag)
        if np.isinf(want):
            n_inf += 1
            assert np.isinf(nll) and nll > 0, (T, lab, flag)
        else:
            worst = max(worst, abs(nll - want))
            assert abs(nll - want) <= 1e-12, (T, lab, flag, nll, want)
    print(f"oracle vs brute force: worst {worst:.2e}, {n_inf} infeasible")
    assert n_inf > 0                             # the set holds problems without a legal path too


def _torch_nll(lp_ext, labels):
    """-log p(labels) by torch's CTC over the C + 1 columns, (1,) fp64 with graph; +inf when infeasible."""
    T = lp_ext.shape[0]
    return torch.nn.functional.ctc_loss(lp_ext.unsqueeze(1), torch.tensor([labels], dtype=torch.long).reshape(1, -1), torch.tensor([T]),
                                        torch.tensor([len(labels)]), blank=0, reduction="sum")


def _variants(labels, flag):
    """The flagged likelihood is the sum of the likelihoods of the target with and without its first / last token (one flag needs
    U >= 1, both need U >= 2: decoders.wildcard_ends guarantees it for the loss)."""
    out = [labels]
    if flag & 1:
        out = out + [v[1:] for v in out]
    if flag & 2:
        out = out + [v[:-1] for v in out]
    return out


def test_oracle_equals_torch_ctc_with_a_constant_column():
    pen = -0.9
    worst_l, worst_g, n = 0.0, 0.0, 0
    for k, (T, lab, flag) in enumerate(_problems()):
        if (flag in (1, 2) and len(lab) < 1) or (flag == 3 and len(lab) < 2):
            continue
        x = torch.from_numpy(_logits(T, 400 + k)).requires_grad_(True)
        lp_ext = torch.cat([x.log_softmax(1), torch.full((T, 1), pen, dtype=torch.float64)], 1)
        terms = [t for t in (_torch_nll(lp_ext, v) for v in _variants(lab, flag)) if torch.isfinite(t)]
        nll, grad = O.loss_and_grad(x.detach().numpy()[:, None, :], [lab], [T], pen, [flag], grad_scale=0.5)
        if not terms:
            assert np.isinf(nll[0]) and not grad.any(), (T, lab, flag)
            continue
        want = -torch.logsumexp(torch.stack([-t for t in terms]), 0)
        (0.5 * want).backward()
        worst_l = max(worst_l, abs(float(want.detach()) - nll[0]))
        worst_g = max(worst_g, float(np.abs(x.grad.numpy() - grad[:, 0]).max()))
        n += 1
    print(f"oracle vs torch ctc_loss over {n} problems: loss {worst_l:.2e} grad {worst_g:.2e}")
    assert n > 200 and worst_l <= 1e-9 and worst_g <= 1e-9


def test_oracle_edges():
    x = _logits(5, 3)[:, None, :].repeat(4, axis=1)
    nll, grad = O.loss_and_grad(x, [[1, C + 1], [0, 2], [1, 2, 3, 1], [C]], [5, 5, 3, 4], -1.0)
    assert np.isinf(nll[:3]).all() and np.isfinite(nll[3])                  # bad labels, more labels than frames
    assert not grad[:, :3].any() and not grad[4:, 3].any() and grad[:4, 3].any()
    nll, _ = O.loss_and_grad(x[:, :2], [[], [1]], [0, 0], -1.0)
    assert nll[0] == 0.0 and np.isinf(nll[1])
    # the target [C] alone with penalty 0: blank* star+ blank*, every frame of the star scoring log 1
    nll, grad = O.loss_and_grad(x[:, :1], [[C]], [5], 0.0)
    assert np.isfinite(nll[0]) and abs(grad.sum()) < 1e-12                    # rows of the gradient sum to 0: softmax (1 - occ*) - occ


def test_wildcard_ends():
    from asr_amd.decoders import encode_transcripts, wildcard_ends
    S = 9
    t, f = wildcard_ends([[1, 2], [S, 1], [1, S], [], [S], [S, S, 3, S, S]], S)
    assert t == [[1, 2], [S, 1], [1, S], [], [S], [S, 3, S]] and f == [0] * 6            # no option: only the runs collapse
    t, f = wildcard_ends([[1, 2], [S, 1], [1, S], [], [S]], S, free_start=True)
    assert t == [[S, 1, 2], [S, 1], [S, 1, S], [S], [S]] and f == [1] * 5                # inserted only when absent
    t, f = wildcard_ends([[1, 2], [S, 1], [1, S], [], [S]], S, free_end=True)
    assert t == [[1, 2, S], [S, 1, S], [1, S], [S], [S]] and f == [2] * 5
    t, f = wildcard_ends([[1, 2], [S, S, 1], [], [S], [4]], S, True, True)
    assert t == [[S, 1, 2, S], [S, 1, S], [S], [S], [S, 4, S]] and f == [3] * 5          # the aligner's flags: the same for every target
    t, f = wildcard_ends([[1, 2], [], [S]], S, True, True, distinct_paths=True)
    assert t == [[S, 1, 2, S], [S], [S]] and f == [3, 1, 1]                              # the loss: one token is not first AND last
    # strings through the label map, then the ends
    labels = "_abc "
    ids = encode_transcripts(["ab**c", "*a", "c"], labels, star="*")
    assert ids == [[1, 2, 5, 3], [5, 1], [3]]
    t, f = wildcard_ends(ids, len(labels), True, True)
    assert t == [[5, 1, 2, 5, 3, 5], [5, 1, 5], [5, 3, 5]] and f == [3, 3, 3]


def test_aligner_uses_the_shared_helper():
    import inspect
    from asr_amd.decoders import CTCAligner
    assert "wildcard_ends(" in inspect.getsource(CTCAligner.align)


def test_ctcloss_constructor_and_plain_path():
    from asr_amd import CTCLoss
    for bad in (0.5, float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError):
            CTCLoss(star=True, star_penalty=bad)
    plain = CTCLoss(reduction="sum")
    assert not plain.wildcards and plain.star_penalty == math.log(0.5)
    assert (plain.star, plain.free_start, plain.free_end) == (False, False, False)
    for kw in (dict(star=True), dict(free_start=True), dict(free_end=True), dict(star_penalty=-2.0)):
        assert CTCLoss(**kw).wildcards, kw
    crit = CTCLoss(star=True, star_penalty=0.0)
    crit.star_penalty = -1.5                                                 # a plain attribute: the caller may anneal it
    assert crit.star_penalty == -1.5


def test_ctcloss_target_preparation():
    from asr_amd import CTCLoss
    crit = CTCLoss(star=True, free_start=True, free_end=True)
    flat = torch.tensor([1, 2, 7, 7, 3, 7, 4, 5], dtype=torch.int32)         # [1 2 * * 3], [* 4], [5], []
    t, off, tl, max_u, flags = crit.prepare_targets(flat, torch.tensor([5, 2, 1, 0]), 7)
    assert t.tolist() == [7, 1, 2, 7, 3, 7, 7, 4, 7, 7, 5, 7, 7] and off.tolist() == [0, 6, 9, 12] and tl.tolist() == [6, 3, 3, 1]
    assert max_u == 6 and flags.tolist() == [3, 3, 3, 1] and all(v.dtype == torch.int32 for v in (t, off, tl, flags))
    padded = torch.tensor([[1, 7, 7, 2], [3, 0, 0, 0]])
    t, off, tl, max_u, flags = CTCLoss(star=True).prepare_targets(padded, torch.tensor([4, 1]), 7)
    assert t.tolist() == [1, 7, 2, 3] and tl.tolist() == [3, 1] and flags.tolist() == [0, 0] and max_u == 3


def _manifest(tmp_path, texts):
    import pandas as pd
    path = tmp_path / "manifest.csv"
    pd.DataFrame({"audio_filepath": [f"a{i}.wav" for i in range(len(texts))], "text": texts, "duration": [1.0] * len(texts)}).to_csv(path, index=False)
    return str(path)


def test_datasets_parse_transcript_with_star(tmp_path):
    from asr_amd.data import SpectrogramDataset, WaveformDataset
    from types import SimpleNamespace

    def audio_conf():
        return SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                               spec_augment=False, noise_dir=None)
    labels = {c: i for i, c in enumerate("_'abc ")}
    texts = ["ab c", "*ab9**c*", "a*?*b", "_a"]
    path = _manifest(tmp_path, texts)
    for cls in (SpectrogramDataset, WaveformDataset):
        plain = cls(audio_conf(), path, labels)
        star = cls(audio_conf(), path, labels, star="*")
        assert [plain.parse_transcript(t) for t in texts] == [[2, 3, 5, 4], [2, 3, 4], [2, 3], [2]]       # today's ids: unknowns dropped
        assert [star.parse_transcript(t) for t in texts] == [[2, 3, 5, 4], [6, 2, 3, 6, 4, 6], [2, 6, 3], [2]]
        for bad in ("a", "**", "", 3):
            with pytest.raises(ValueError):
                cls(audio_conf(), path, labels, star=bad)
