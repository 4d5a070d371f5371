"""Time the n-gram pruning and evaluation (asr_amd/decoders/lm_train.py, ops.ngram_prune / ngram_eval, csrc/ngram_prune.h) on the
estimator's Zipf corpora (scripts/time_ngram_train.py: "char" 26 letters order 5, "word" 50 000 words order 3; --sizes tokens).

The last 10 % of the sentences are held out; the model is estimated on the rest, on the GPU, and its sorted arrays stay there.
Per corpus, wall clock with a device synchronisation on either side, the median of --reps runs and spread = max - min:
  eval        ops.ngram_eval of the held-out sentences under the full model (one launch), and its host twin
  values      ops.ngram_prune_values: the context-sum launches of every order and the entropy launch
  prune       ops.ngram_prune at each threshold: values, closure, gathering of the kept rows (torch), the new backoffs
  host twin   ops.ngram_prune on the same arrays on the host (one thread), at --host-theta only, once
  write       NgramEstimate.write_arpa of each model (Python); the file's bytes
  fit         estimate_ngram(...).write_arpa end to end, with and without prune=: tokenise, count, solve, (prune,) download, write
and per threshold the n-grams kept per order, the bytes of the search's packed tables without the dictionary trie
(ds2_ctc_lm_packed_bytes) and the held-out perplexity.  BeamCTCDecoder.fit_lm adds the loading of the written file (NgramLM, Python),
timed with --fit-lm on the sizes up to --fit-lm-max only.  NOT measured here: decode time against the table's size
(scripts/time_lm_table_size.py), WER, more than one GPU.  Prints a table and one JSON line per corpus."""
import argparse
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from time_ngram_train import CONFIGS, corpus, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=float, nargs="+", default=[1e6, 1e7])
    ap.add_argument("--kinds", nargs="+", default=list(CONFIGS))
    ap.add_argument("--thetas", type=float, nargs="+", default=[1e-8, 1e-7, 1e-6])
    ap.add_argument("--host-theta", type=float, default=1e-7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fit-lm", action="store_true")
    ap.add_argument("--fit-lm-max", type=float, default=1e6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import _lib, ops
    from asr_amd.decoders import BeamCTCDecoder, lm_train
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def ppl(lp, order):
        scored = order > 0
        return 10.0 ** (-float(torch.sum(torch.where(scored, lp, torch.zeros_like(lp)))) / int(scored.sum()))

    say(f"n-gram pruning and evaluation, {torch.cuda.get_device_name(0)}; seconds, median of reps, spread = max - min")
    for kind in args.kinds:
        cfg = CONFIGS[kind]
        labels = "_abcdefghijklmnopqrstuvwxyz" if kind == "char" else "_w0123456789 "
        for size in args.sizes:
            n = int(size)
            sentences = corpus(kind, n)
            cut = len(sentences) - len(sentences) // 10
            train, held = sentences[:cut], sentences[cut:]
            vocab, flat, offsets, n_empty = lm_train.tokenize(train, cfg["mode"])
            d_flat, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offsets).to(dev)
            full = ops.ngram_collect_model(ops.ngram_solve(ops.ngram_count(d_flat, d_off, len(vocab), cfg["order"])))
            sizes = (int(flat.size), len(offsets) - 1, n_empty)
            est = lm_train.NgramEstimate(ops.ngram_model_download(full), cfg["mode"], vocab, *sizes, model=full)
            h_flat, h_off = est.tokens(held)
            e_flat, e_off = torch.from_numpy(h_flat).to(dev), torch.from_numpy(h_off).to(dev)
            ops.ngram_eval(full, e_flat[:10].contiguous(), torch.tensor([0, 10], device=dev))   # warm-up
            legs, rows = {}, []
            (lp, order), legs["eval"] = timed(lambda: ops.ngram_eval(full, e_flat, e_off), args.reps, True)
            host_model = est.model("cpu")
            (lp_h, order_h), legs["eval host twin"] = timed(lambda: ops.ngram_eval(host_model, torch.from_numpy(h_flat), torch.from_numpy(h_off)),
                                                            1, False)
            eval_agree = bool(torch.equal(order.cpu(), order_h)) and float((lp.cpu() - lp_h).abs().nan_to_num().max()) <= 1e-12
            _, legs["values"] = timed(lambda: ops.ngram_prune_values(full, args.thetas[0]), args.reps, True)
            say(f"{kind} order {cfg['order']}, {n} tokens, {len(train)} + {len(held)} held-out sentences ({h_flat.size} tokens, "
                f"{int((h_flat == 0).sum())} OOV), n_vocab {len(vocab)}; evaluation equals the host twin's: {eval_agree}")
            with tempfile.TemporaryDirectory() as d:
                for theta in [None] + list(args.thetas):
                    name = "full" if theta is None else f"{theta:g}"
                    model, t_prune = (full, None) if theta is None else timed(lambda: ops.ngram_prune(full, theta), args.reps, True)
                    one = est if model is full else lm_train.NgramEstimate(ops.ngram_model_download(model), cfg["mode"], vocab, *sizes, model=model)
                    _, t_write = timed(lambda: one.write_arpa(os.path.join(d, "m.arpa")), 1, False)
                    kept = [len(s[0]) for s in one.ngrams]
                    packed = int(_lib.load().ds2_ctc_lm_packed_bytes(one.order, sum(kept) + 1, 0, 1, len(labels)))
                    row = {"theta": name, "kept": kept, "arpa_bytes": os.path.getsize(os.path.join(d, "m.arpa")), "packed_bytes": packed,
                           "held_out_ppl": round(ppl(*ops.ngram_eval(model, e_flat, e_off)), 3), "prune": t_prune, "write": t_write}
                    _, row["fit"] = timed(lambda: lm_train.estimate_ngram(train, cfg["order"], cfg["mode"], device=dev, prune=theta)
                                          .write_arpa(os.path.join(d, "f.arpa")), 1, True)
                    if args.fit_lm and n <= args.fit_lm_max:
                        dec = BeamCTCDecoder(labels)
                        _, row["fit_lm"] = timed(lambda: dec.fit_lm(train, order=cfg["order"], mode=cfg["mode"], device=dev,
                                                                    **({} if theta is None else {"prune": theta})), 1, True)
                    rows.append(row)
                    say(f"  theta {name:6s} kept {kept}  arpa {row['arpa_bytes'] / 1e6:8.1f} MB  packed {packed / 1e6:8.1f} MB  held-out ppl "
                        f"{row['held_out_ppl']:10.3f}  prune {'-' if t_prune is None else format(t_prune['s'], '.4f'):>7s} s  write "
                        f"{t_write['s']:7.3f} s  fit {row['fit']['s']:7.3f} s" + (f"  fit_lm {row['fit_lm']['s']:7.3f} s" if "fit_lm" in row else ""))
            _, legs["prune host twin"] = timed(lambda: ops.ngram_prune(host_model, args.host_theta), 1, False)
            for name, r in legs.items():
                say(f"  {name:16s} {r['s']:10.4f} s   spread {r['spread']:8.4f}   ({r['reps']} reps)")
            say(json.dumps({"kind": kind, "tokens": n, "order": cfg["order"], "legs": legs, "rows": rows, "eval_agree": eval_agree}))


if __name__ == "__main__":
    main()
