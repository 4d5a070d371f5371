"""Time the CTC beam decode (ds2_ctc_beam_decode_f32) against the eval-mode forward that produces its input, in one process:
B = 64 utterances of T = 501 frames (c3's output length for 1001 input frames), C = 29, beam widths 10 / 100 / 256, cutoff_top_n 40.
The decode is timed on the forward's output (a randomly initialised c3: near-uniform frames) and on peaked random frames of the
same shape.  With --profile each timed decode is followed by one run of the profiling build (DS2_EXPERIMENTAL=1 DS2_BEAM_PROFILE=1),
which prints the per-frame time of each step and the tie-rule chain walks to stderr.  With --lm PATH (an ARPA file, e.g. from
scripts/make_synthetic_arpa.py) the LM arm is timed too, at beam widths 10 and 100 with --alpha / --beta; the 29 labels are bound with
the last one ("|") read as the space, so that a word-level model has its space label.
With --hotwords N the hotword arm is timed instead of all of the above: N random phrases of 4 to 12 labels (--hotword-weight each,
seed 0), at beam widths 10 and 100, on both kinds of frames, hot-only and (with --lm) hot + LM, next to the no-LM kernel and the LM
entry without hotwords in the same run: the legs are alternated over --rounds rounds, each leg's median over the rounds and its
spread (max - min) are reported with the ratios hot-only / no-LM and hot + LM / LM, and --out PATH also writes them as a table.
Prints one JSON line.  Usage: python scripts/time_beam_decode.py [--reps N] [--profile] [--lm PATH [--alpha A] [--beta B]]
       [--hotwords N [--hotword-weight W] [--rounds R] [--out PATH]]"""
import argparse
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def _time_hotwords(args, ops, C, inputs):
    """the four legs (no-LM kernel, hot-only, LM entry, hot + LM) per (frames, K), alternated over args.rounds rounds"""
    import numpy as np
    from asr_amd.decoders.hotwords import Hotwords
    from asr_amd.decoders.lm import NgramLM
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
    rng = np.random.default_rng(0)
    phrases = {}
    while len(phrases) < args.hotwords:                   # prefix-free by construction: a candidate that clashes is drawn again
        p = tuple(int(x) for x in rng.integers(1, C, size=int(rng.integers(4, 13))))
        if all(p[:len(q)] != q and q[:len(p)] != p for q in phrases):
            phrases[p] = None
    hot = Hotwords([list(p) for p in phrases], chars[:C], 0, args.hotword_weight)
    lm = NgramLM(args.lm, dict(enumerate(chars[:C])), 0, 28 if C > 28 else None) if args.lm else None
    out = dict(phrases=len(phrases), trie_nodes=hot.n_nodes, packed_kb=round(hot.packed.nbytes / 1024, 1), weight=args.hotword_weight,
               rounds=args.rounds, reps=args.reps, legs={})
    if lm is not None:
        out["lm"] = dict(path=os.path.basename(args.lm), mode=lm.mode_name, order=lm.order, ngrams=lm.n_ngrams, alpha=args.alpha, beta=args.beta)
    lines = [f"# scripts/time_beam_decode.py --hotwords {args.hotwords}: B=64 T={inputs[0][1].shape[1]} C={C} cutoff_top_n=40, "
             f"{len(phrases)} phrases of 4..12 labels ({hot.n_nodes} trie nodes), weight {args.hotword_weight}"
             + (f", LM {out['lm']['mode']} {lm.order}-gram ({lm.n_ngrams} n-grams) alpha {args.alpha} beta {args.beta}" if lm else ""),
             f"# ms per batch: median of {args.rounds} alternated rounds (each the median of {args.reps} calls), spread = max - min",
             "frames   K    no_lm (spread)   hot_only (spread)  ratio |   lm (spread)   hot_lm (spread)  ratio"]
    for name, p, sz in inputs:
        for K in (10, 100):
            legs = {"no_lm": lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0),
                    "hot_only": lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0, hotwords=hot)}
            if lm is not None:
                legs["lm"] = lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0, lm, args.alpha, args.beta)
                legs["hot_lm"] = lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0, lm, args.alpha, args.beta, hotwords=hot)
            ms = {k: [] for k in legs}
            for _ in range(args.rounds):
                for k, fn in legs.items():
                    ms[k].append(_time(fn, args.reps))
            r = {k: dict(ms=round(sorted(v)[len(v) // 2], 3), spread=round(max(v) - min(v), 3)) for k, v in ms.items()}
            r["hot_only_over_no_lm"] = round(r["hot_only"]["ms"] / r["no_lm"]["ms"], 3)
            row = f"{name:8s} {K:3d} {r['no_lm']['ms']:9.3f} ({r['no_lm']['spread']:.3f}) {r['hot_only']['ms']:9.3f} ({r['hot_only']['spread']:.3f}) " \
                  f"{r['hot_only_over_no_lm']:6.3f} |"
            if lm is not None:
                r["hot_lm_over_lm"] = round(r["hot_lm"]["ms"] / r["lm"]["ms"], 3)
                row += f" {r['lm']['ms']:9.3f} ({r['lm']['spread']:.3f}) {r['hot_lm']['ms']:9.3f} ({r['hot_lm']['spread']:.3f}) {r['hot_lm_over_lm']:6.3f}"
            out["legs"][f"{name}_K{K}"] = r
            lines.append(row)
            if args.profile:
                print(f"[{name} K={K}: the profiling build exists for the no-LM kernel only]", end=" ", file=sys.stderr, flush=True)
                os.environ["DS2_EXPERIMENTAL"], os.environ["DS2_BEAM_PROFILE"] = "1", "1"
                ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0)
                del os.environ["DS2_EXPERIMENTAL"], os.environ["DS2_BEAM_PROFILE"]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--lm", default=None)
    ap.add_argument("--alpha", type=float, default=0.8)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--hotwords", type=int, default=0)
    ap.add_argument("--hotword-weight", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from asr_amd import DeepSpeech, ops
    rnn, H, L, C, B, tin = bench.WORKLOADS["c3"]
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = DeepSpeech(audio_conf=bench.audio_conf(), decoder=None, label_path=bench.label_file(tmp, C), rnn_type=rnn,
                           rnn_hidden_size=H, rnn_hidden_layers=L, bidirectional=True)
    model.cuda().eval()
    x, _, pct, _ = bench.synthetic_batch(B, tin, C, 1)
    x = x.cuda()
    lens = (pct * x.size(3)).int()
    with torch.no_grad():
        out, out_lens = model.forward(x, lens)
        fwd_ms = _time(lambda: model.forward(x, lens), args.reps)
    probs = out.detach().float().contiguous()
    g = torch.Generator().manual_seed(0)
    z = torch.randn(probs.shape, generator=g) * 16.0
    z[..., 0] += 2.0
    peaked = torch.softmax(z, -1).cuda()
    res = dict(batch=B, frames=int(probs.shape[1]), classes=int(probs.shape[2]), eval_forward_ms=round(fwd_ms, 3),
               max_prob_mean={"forward": round(float(probs.max(-1).values.mean()), 4), "peaked": round(float(peaked.max(-1).values.mean()), 4)},
               decode_ms={"forward": {}, "peaked": {}})
    if args.hotwords:
        res.pop("decode_ms")
        res["hotwords"] = _time_hotwords(args, ops, C, (("forward", probs, out_lens), ("peaked", peaked, None)))
        print(json.dumps(res))
        return
    for name, p, sz in (("forward", probs, out_lens), ("peaked", peaked, None)):
        for K in (10, 100, 256):
            res["decode_ms"][name][K] = round(_time(lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0), args.reps), 3)
            if args.profile:
                os.environ["DS2_EXPERIMENTAL"], os.environ["DS2_BEAM_PROFILE"] = "1", "1"
                print(f"[{name}]", end=" ", file=sys.stderr, flush=True)
                ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0)
                del os.environ["DS2_EXPERIMENTAL"], os.environ["DS2_BEAM_PROFILE"]
    if args.lm:
        from asr_amd.decoders.lm import NgramLM
        chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + [" "]
        lm = NgramLM(args.lm, dict(enumerate(chars[:C])), 0, 28 if C > 28 else None)
        res["lm"] = dict(path=os.path.basename(args.lm), mode=lm.mode_name, order=lm.order, ngrams=lm.n_ngrams, packed_mb=round(lm.packed.nbytes / 2**20, 2),
                         alpha=args.alpha, beta=args.beta, decode_ms={"forward": {}, "peaked": {}})
        for name, p, sz in (("forward", probs, out_lens), ("peaked", peaked, None)):
            for K in (10, 100):
                res["lm"]["decode_ms"][name][K] = round(_time(lambda: ops.ctc_beam_decode(p, sz, 0, K, 40, 1.0, lm, args.alpha, args.beta),
                                                              args.reps), 3)
        res["lm"]["k10_within_forward"] = res["lm"]["decode_ms"]["forward"][10] <= fwd_ms
    res["greedy_ms"] = round(_time(lambda: ops.greedy_decode(probs, out_lens, 0), args.reps), 3)
    res["k100_within_forward"] = res["decode_ms"]["forward"][100] <= fwd_ms
    print(json.dumps(res))


if __name__ == "__main__":
    main()
