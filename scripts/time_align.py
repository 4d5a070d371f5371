"""Time CTC forced alignment (ops.ctc_forced_align) at the c3 eval shape next to its yardstick, the CTC loss lattice without gradient.

B = 64, T = 501, C = 29 probabilities from a random-init c3 eval forward.  Leg U = 60 takes the one-wavefront variant, leg U = 150 the
workgroup variant (the library's own choice, variant 0, and the loss's own lattice choice at the same shapes).  Device events around
`iters` back-to-back calls, the legs alternated within every round; the float32 NumPy oracle (tests/ctc_align_oracle.py) is timed on the
host once.  Prints a table and one JSON line.  (Kernel-only times: run this under `rocprofv3 --kernel-trace --stats -- python ...`.)"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def c3_probs(dev, B, tin, hidden, layers):
    import pandas as pd
    from asr_amd import DeepSpeech
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    conf = SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                           spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.csv")
        pd.DataFrame({"label": chars}).to_csv(path, index=False)
        model = DeepSpeech(audio_conf=conf, decoder=None, label_path=path, rnn_type="gru", rnn_hidden_size=hidden, rnn_hidden_layers=layers,
                           bidirectional=True)
    model.to(dev).eval()
    x = torch.randn(B, 1, 161, tin, device=dev)
    with torch.no_grad():
        probs, sizes = model.forward(x, torch.full((B,), tin, dtype=torch.int32))
    torch.cuda.synchronize()
    return probs, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1001, help="input frames (the output has (frames + 1) // 2)")
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    from asr_amd import ops
    assert torch.cuda.is_available(), "time_align.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    probs, sizes = c3_probs(dev, args.batch, args.frames, args.hidden, args.layers)      # (B,T,C) view of (T,B,C) storage
    B, T, C = probs.shape
    logits_tbc = probs.transpose(0, 1)
    assert logits_tbc.is_contiguous()
    rng = np.random.default_rng(0)
    legs = {}
    for U in (60, 150):
        lab = rng.integers(1, C, (B, U)).astype(np.int32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        legs[U] = dict(lab=lab, targets=t(lab.reshape(-1)), off=t(np.arange(B, dtype=np.int32) * U), lens=t(np.full(B, U, np.int32)),
                       in_lens=sizes.to(dev).int().contiguous())

    def align(U):
        g = legs[U]
        return ops.ctc_forced_align(probs, g["targets"], g["off"], g["in_lens"], g["lens"], U, False, 0)

    def loss(U):
        g = legs[U]
        return ops.ctc_loss(logits_tbc, g["targets"], g["off"], g["in_lens"], g["lens"], U, 1.0, want_grad=False)

    calls = {f"align_U{U}": (lambda U=U: align(U)) for U in legs}
    calls.update({f"loss_U{U}": (lambda U=U: loss(U)) for U in legs})
    for fn in calls.values():                                                        # warm up every shape of the timed window
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for U in legs:
        assert bool(torch.isfinite(align(U)[0]).all()), "an utterance of the timing batch is infeasible"
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                  # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)                  # us per call
    res = dict(B=B, T=T, C=C, rounds=args.rounds, iters=args.iters)
    print(f"B = {B}, T = {T}, C = {C}; us per call (device events, {args.iters} calls back to back), mean over {args.rounds} rounds [rounds] spread = max - min")
    print(f"{'leg':<14}{'us/call':>10}{'us/frame':>10}   rounds")
    for k, v in times.items():
        m = float(np.mean(v))
        res[k + "_us"], res[k + "_us_rounds"], res[k + "_spread_us"] = round(m, 2), [round(a, 2) for a in v], round(max(v) - min(v), 2)
        res[k + "_us_per_frame"] = round(m / T, 4)
        print(f"{k:<14}{m:>10.2f}{m / T:>10.4f}   {[round(a, 2) for a in v]}  spread {max(v) - min(v):.2f}")
    if not args.no_oracle:
        import ctc_align_oracle as A
        e = torch.log(probs).cpu().numpy()
        for U in legs:
            t0 = time.perf_counter()
            A.align_batch(e, legs[U]["lab"].reshape(-1), np.arange(B) * U, None, np.full(B, U))
            res[f"numpy_oracle_U{U}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(f"float32 NumPy oracle on the host, U = {U}: {res[f'numpy_oracle_U{U}_ms']} ms per batch")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
