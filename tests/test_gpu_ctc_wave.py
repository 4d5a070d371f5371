"""-m gpu: the one-wavefront-per-lattice CTC kernel (ctc_lattice_wave_kernel, taken when 2 * max_target_len + 1 <= 128) against the
one-workgroup-per-lattice kernel it stands in for (ctc_lattice_kernel, `lattice=1` of ds2_ctc_loss_ex_f32): the alpha / beta lattices, the
per-utterance losses and the gradient must be the SAME BITS — the new kernel evaluates the same expressions in the same operand order."""
import numpy as np
import pytest
import torch

import det

pytestmark = pytest.mark.gpu


def _labels(n, C, seed, repeat=False):
    lab = det.randint((max(n, 1),), seed, 1, C).astype(np.int32)[:n]
    if repeat and n >= 4:
        lab[1:4] = lab[1]                      # a run of three
        lab[n // 2:] = lab[n // 2]             # and a long run (needs a blank between every pair)
    return lab


# name -> (C, T, target lengths, input lengths, repeated labels)
CASES = {
    # U in {0, 1, 50, 63} (S = 127: the last shape the wave kernel takes), ragged lengths on both sides of the 8-frame prefetch groups
    "u_edges_c29": (29, 150, [0, 1, 50, 63, 7, 3, 1, 0], [150, 149, 150, 145, 9, 10, 1, 17], False),
    "u_edges_c80": (80, 150, [63, 50, 1, 0, 12, 33], [150, 131, 2, 8, 77, 140], False),
    "repeats_c29": (29, 140, [50, 63, 8, 4, 21], [140, 140, 17, 8, 60], True),
    "repeats_c80": (80, 96, [40, 4, 17, 30], [96, 7, 50, 61], True),
    # no valid alignment: more labels than frames, repeated labels without room for the blanks, an empty input
    "infeasible": (29, 64, [15, 20, 5, 3, 2, 0], [11, 20, 64, 0, 1, 0], True),
    # S = 129 > 128: the launcher keeps the workgroup kernel (U = 64), also for the short utterances of that batch
    "u64_old_path": (29, 150, [64, 63, 1, 0], [150, 150, 40, 13], False),
    "u200_old_path_c80": (80, 420, [200, 64, 5], [420, 300, 9], True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_wave_lattice_is_bit_identical_to_workgroup_lattice(case):
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from asr_amd import ops
    from asr_amd.ctc import _prep_targets
    dev = torch.device("cuda:0")
    C, T, tl, il, rep = CASES[case]
    B = len(tl)
    logits = torch.from_numpy(det.unitvar((T, B, C), 7 + C + T) * np.float32(2.0)).to(dev)
    targets = np.concatenate([_labels(u, C, 100 + i, rep) for i, u in enumerate(tl)] or [np.zeros(0, np.int32)])
    if case == "infeasible":
        targets[: tl[0]] = 3                   # 15 equal labels need 29 frames, 11 exist
    tg, off, tld, max_u = _prep_targets(torch.from_numpy(targets), torch.tensor(tl, dtype=torch.int32), dev)
    ild = torch.tensor(il, dtype=torch.int32, device=dev)
    got = ops.ctc_loss(logits, tg, off, ild, tld, max_u, 0.125, lattice=0, return_ab=True)
    ref = ops.ctc_loss(logits, tg, off, ild, tld, max_u, 0.125, lattice=1, return_ab=True)
    torch.cuda.synchronize()
    for name, a, b in zip(("nll", "grad", "ab"), got, ref):
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        print(f"{case}: {name} differing words: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()}")
        assert same, (case, name)
    nll = got[0].cpu().numpy()
    if case == "infeasible":
        assert np.isinf(nll[0]) and np.isinf(nll[3]) and np.isinf(nll[4]) and nll[5] == 0.0 and np.isfinite(nll[2])
    else:
        assert np.isfinite(nll).all() and (nll[np.asarray(tl) > 0] > 0).all()
    # and against torch's own CTC on the CPU, so that "equal" is not "equally wrong"
    lp = logits.cpu().double().log_softmax(2)
    keep = [b for b in range(B) if il[b] > 0]
    offs = np.concatenate([[0], np.cumsum(tl)])
    for b in keep:
        want = torch.nn.functional.ctc_loss(lp[: il[b], b:b + 1], torch.from_numpy(targets[offs[b]:offs[b + 1]]).long().unsqueeze(0),
                                            torch.tensor([il[b]]), torch.tensor([tl[b]]), blank=0, reduction="sum")
        if np.isinf(float(want)):
            assert np.isinf(nll[b]), (case, b)
        else:
            assert abs(float(want) - nll[b]) <= 1e-4 + 1e-5 * abs(float(want)), (case, b, float(want), nll[b])
