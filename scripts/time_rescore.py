"""Time n-best rescoring against the decode it replaces in a sweep of LM weights, in one process: B = 64 utterances of T = 501 frames,
C = 29, beam width K = 100, cutoff_top_n 40, on peaked random frames (scripts/time_beam_decode.py's), with the synthetic 200k-n-gram
word and character models of scripts/make_synthetic_arpa.py (seed 0).  Legs, per model:
  (a) decode   the LM first pass alone (ops.ctc_beam_decode with the model): the cost of ONE grid point done by decoding again;
  (b) lm_score ops.lm_score on its B * K hypotheses;
  (c) host     the same scores through the host loop over NgramLM.score (one library call per token), on the first --host-hyps
               hypotheses, wall clock, scaled to B * K;
  (d) exact    the exact likelihoods of the B * K hypotheses (NBestRescorer.exact_likelihoods: ops.ctc_mwer in chunks within the
               default 2 GiB workspace);
  (e) sweep    ops.nbest_sweep over a 21 x 21 grid, at N = 64 and at N = 2688 (the batch tiled 42 times: a dev set's size).
The device legs are alternated over --rounds rounds and timed with device events; each leg's median over the rounds (each the
median of --reps calls) and its spread (max - min) are reported.  The expectation to confirm or refute: (b) + (d) + (e) < (a).
Prints one JSON line; --out PATH also writes the table.
Usage: python scripts/time_rescore.py [--reps N] [--rounds R] [--host-hyps H] [--out PATH]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.time_beam_decode import _time   # noqa: E402


def _host_scores(lm, labels_h, lens_h, chars, n):
    """the host loop: tokens by string, one NgramLM.score call each -> seconds for n hypotheses"""
    flat_l, flat_n = labels_h.reshape(-1, labels_h.shape[-1]), lens_h.reshape(-1)
    t0 = time.perf_counter()
    for p in range(n):
        text = "".join(chars[i] for i in flat_l[p, :flat_n[p]].tolist())
        toks = list(text) if lm.mode_name == "char" else text.split()
        total = np.float32(0.0)
        for i, w in enumerate(toks):
            s = lm.score(toks[max(0, i - lm.order + 1):i], w)
            if s != -1000.0:
                total = np.float32(total + np.float32(s))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-hyps", type=int, default=128)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import ops
    from asr_amd.decoders import BeamCTCDecoder, NBestRescorer
    from scripts.make_synthetic_arpa import make
    B, T, C, K = 64, 501, 29, 100
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    g = torch.Generator().manual_seed(0)
    z = torch.randn((B, T, C), generator=g) * 16.0
    z[..., 0] += 2.0
    probs = torch.softmax(z, -1).cuda()
    logp = torch.log(probs)
    dev = probs.device
    alphas, betas = [0.1 * i for i in range(21)], [0.2 * i - 2.0 for i in range(21)]
    res = dict(batch=B, frames=T, classes=C, beam_width=K, rounds=args.rounds, reps=args.reps, grid=[len(alphas), len(betas)], models={})
    lines = [f"# scripts/time_rescore.py: B={B} T={T} C={C} K={K} cutoff_top_n=40, peaked random frames, synthetic 3-gram models (make_synthetic_arpa.py, "
             "200k n-grams asked for; the n-grams each model holds are in its last line)",
             f"# ms per batch of {B * K} hypotheses: median of {args.rounds} alternated rounds (each the median of {args.reps} calls), spread = max - min",
             f"# (c) host: wall clock of the NgramLM.score loop on the first {args.host_hyps} hypotheses, scaled to {B * K}",
             "model  leg                      ms   (spread)"]
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("word", "char"):
            path, n_ngrams = make(os.path.join(tmp, f"{mode}.arpa"), mode=mode)
            dec = BeamCTCDecoder({c: i for i, c in enumerate(chars)}, lm_path=path, alpha=args.alpha, beta=args.beta, beam_width=K)
            lm = dec.lm
            resc = NBestRescorer(dec)
            decode = lambda: ops.ctc_beam_decode(probs, None, 0, K, 40, 1.0, lm, args.alpha, args.beta)   # noqa: E731
            labels, _, lens, scores = decode()
            off = (torch.arange(B * K, device=dev, dtype=torch.int64) * T).view(B, K)
            lens_h, valid = lens.cpu().numpy(), scores > -float("inf")
            in_lens = torch.full((B,), T, dtype=torch.int32, device=dev)
            lm_sum, n_tok, n_oov = (t.view(B, K) for t in ops.lm_score(labels, off.view(-1), lens.view(-1), lm, T))
            ac = resc.exact_likelihoods(logp, labels, off, lens, valid, in_lens, lens_h)
            err = torch.randint(0, 20, (B, K, 2), dtype=torch.int32, device=dev)
            big = [t.repeat(42, *([1] * (t.dim() - 1))).contiguous() for t in (ac, lm_sum, n_tok, n_oov, err)]
            legs = {"a_decode": decode,
                    "b_lm_score": lambda: ops.lm_score(labels, off.view(-1), lens.view(-1), lm, T),
                    "d_exact": lambda: resc.exact_likelihoods(logp, labels, off, lens, valid, in_lens, lens_h),
                    "e_sweep_N64": lambda: ops.nbest_sweep(ac, lm_sum, n_tok, n_oov, err, alphas, betas, want_pick=False),
                    "e_sweep_N2688": lambda: ops.nbest_sweep(*big, alphas, betas, want_pick=False)}
            ms = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    ms[k].append(_time(fn, args.reps))
            r = {k: dict(ms=round(sorted(v)[len(v) // 2], 3), spread=round(max(v) - min(v), 3)) for k, v in ms.items()}
            n_host = min(args.host_hyps, B * K)
            host_s = _host_scores(lm, labels.cpu().numpy(), lens_h, chars, n_host)
            r["c_host_scaled"] = dict(ms=round(1e3 * host_s * B * K / n_host, 1), measured_hyps=n_host, measured_ms=round(1e3 * host_s, 1))
            r["rescore_total"] = round(r["b_lm_score"]["ms"] + r["d_exact"]["ms"] + r["e_sweep_N64"]["ms"], 3)
            r["rescore_below_one_decode"] = r["rescore_total"] < r["a_decode"]["ms"]
            r["model"] = dict(mode=lm.mode_name, order=lm.order, ngrams=n_ngrams, packed_mb=round(lm.packed.nbytes / 2 ** 20, 2))
            r["hypotheses"] = dict(valid=int(valid.sum()), mean_len=round(float(lens_h.mean()), 1), max_len=int(lens_h.max()),
                                   tokens=int(n_tok.clamp(min=0).sum()), oov=int(n_oov.clamp(min=0).sum()),
                                   chunks=len(resc._chunks(lens_h, T, K)))
            res["models"][mode] = r
            for k in ("a_decode", "b_lm_score", "d_exact", "e_sweep_N64", "e_sweep_N2688"):
                lines.append(f"{mode:5s}  {k:16s} {r[k]['ms']:10.3f}   ({r[k]['spread']:.3f})")
            lines.append(f"{mode:5s}  {'c_host_scaled':16s} {r['c_host_scaled']['ms']:10.1f}   ({n_host} hypotheses took {r['c_host_scaled']['measured_ms']} ms)")
            lines.append(f"{mode:5s}  (b)+(d)+(e, N=64) = {r['rescore_total']:.3f} ms against (a) = {r['a_decode']['ms']:.3f} ms: "
                         f"{'below' if r['rescore_below_one_decode'] else 'NOT below'} one decode; {r['model']}; {r['hypotheses']}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
