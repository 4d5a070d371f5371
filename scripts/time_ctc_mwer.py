"""Time the minimum-error-rate loss (ops.ctc_mwer, MWERLoss) next to the plain loss (ops.ctc_loss) of the same run.

T = 501, B = 64, C = 29 logits, every frame valid.  The logits are peaked (a random label path with blanks, margin --peak) so that the
beam search returns transcripts of a realistic length (about --labels labels) and not the noise of flat posteriors.  Legs:
  plain          ops.ctc_loss on the references, gradient included                                    (the yardstick)
  mwer_K         ops.ctc_mwer alone on the K best beams of a search done once outside the timed window, gradient included,
                 max_hyp_len = the longest hypothesis of the list (what a caller who knows a bound passes)
  mwer_K_T       the same with max_hyp_len = T (MWERLoss's default: the workgroup lattice, the 8 B K T (2T + 1) byte workspace)
  full_K         MWERLoss.run: softmax, beam search (beam_width --beam), label risks, plain loss at ctc_weight, ops.ctc_mwer at
                 max_hyp_len = T
for K in 2, 4, 8.  Device events around `iters` back-to-back calls, the legs alternated within every round.  Prints a table with the
ratio of every leg to the plain leg, and one JSON line; --out also writes both to a file.  No threshold is set here."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=501)
    ap.add_argument("--classes", type=int, default=29)
    ap.add_argument("--labels", type=int, default=60)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--peak", type=float, default=8.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import BeamCTCDecoder, MWERLoss, ops
    assert torch.cuda.is_available(), "time_ctc_mwer.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    B, T, C, U = args.batch, args.frames, args.classes, args.labels
    rng = np.random.default_rng(0)
    refs = rng.integers(1, C, (B, U)).astype(np.int32)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    span = T // U                                                                      # every label holds span // 2 frames, then blanks
    for b in range(B):
        path = np.zeros(T, np.int64)
        for u in range(U):
            path[u * span:u * span + max(span // 2, 1)] = refs[b, u]
        x[np.arange(T), b, path] += args.peak
    logits = torch.from_numpy(x).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                    # noqa: E731
    in_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    tg, off, tl = t(refs.reshape(-1)), t(np.arange(B, dtype=np.int32) * U), t(np.full(B, U, np.int32))
    labels = ["_"] + [chr(65 + i) for i in range(C - 2)] + [" "]
    dec = BeamCTCDecoder(labels, beam_width=args.beam)
    calls, info = {}, {}
    calls["plain"] = lambda: ops.ctc_loss(logits, tg, off, in_lens, tl, U, 1.0 / B, want_grad=True)
    for K in (2, 4, 8):
        crit = MWERLoss(dec, nbest=K, ctc_weight=0.01)
        crit.run(logits, tg, off, in_lens, tl, U, 1.0 / B, True)
        lab, lens, valid, risk, post = crit.last_nbest
        lab, risk = lab.contiguous().view(-1), risk.contiguous()
        hoff = (torch.arange(B * K, device=dev, dtype=torch.int64) * T).view(B, K)
        longest = int(lens.max())
        bound = longest
        info[f"K{K}"] = dict(longest_hyp=longest, max_hyp_len=bound, valid_slots=int(valid.sum()), mean_risk=round(float(risk.mean()), 3),
                             mean_top_post=round(float(post.max(1).values.mean()), 4),
                             ws_bound_MB=round(ops._lib.load().ds2_ctc_mwer_workspace_bytes(T, B, K, bound) / 2 ** 20, 1),
                             ws_T_MB=round(ops._lib.load().ds2_ctc_mwer_workspace_bytes(T, B, K, T) / 2 ** 20, 1))
        calls[f"mwer_{K}"] = lambda lab=lab, hoff=hoff, lens=lens, valid=valid, risk=risk, bound=bound: ops.ctc_mwer(
            logits, lab, hoff, lens, valid, in_lens, bound, risk, 1.0 / B)
        calls[f"mwer_{K}_T"] = lambda lab=lab, hoff=hoff, lens=lens, valid=valid, risk=risk: ops.ctc_mwer(
            logits, lab, hoff, lens, valid, in_lens, T, risk, 1.0 / B)
        calls[f"full_{K}"] = lambda crit=crit: crit.run(logits, tg, off, in_lens, tl, U, 1.0 / B, True)
    for k, fn in calls.items():                                                        # warm up every shape of the timed window
        for _ in range(2):
            out = fn()
        assert bool(torch.isfinite(out[0]).all()), f"{k}: a value of the timing batch is not finite"
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():                                                    # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)                    # us per call
    res = dict(B=B, T=T, C=C, labels=U, beam=args.beam, peak=args.peak, rounds=args.rounds, iters=args.iters, nbest=info)
    lines = [f"B = {B}, T = {T}, C = {C}, references of {U} labels, beam_width {args.beam}; us per call (device events, {args.iters} calls "
             f"back to back), mean over {args.rounds} rounds; ratio = to the plain loss of the same run",
             f"{'leg':<14}{'us/call':>12}{'ratio':>9}   rounds"]
    base = float(np.mean(times["plain"]))
    for k, v in times.items():
        m = float(np.mean(v))
        res[k + "_us"], res[k + "_ratio"] = round(m, 1), round(m / base, 3)
        lines.append(f"{k:<14}{m:>12.1f}{m / base:>9.2f}   {[round(a, 1) for a in v]}")
    for K, d in info.items():
        lines.append(f"{K}: {d}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
