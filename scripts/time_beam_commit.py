"""Time the streaming beam search's commit and compaction (ops.ctc_beam_stream_commit, csrc/ctc_beam_commit.h) and check that the
streaming instances it touched cost what they did.

Planted posteriors as scripts/time_beam_stream.py makes them.  B = 64, T = 501, C = 29, K = 100, plain and word LM, chunks of 50 and 250:
  entry legs   ds2_ctc_beam_decode(_lm)_f32 and a whole uncommitted stream through ds2_ctc_beam_stream_feed_f32 (zeroed state, nodes for
               T frames, no partials, the final read-out of K slots), with preallocated buffers, on this library and, with --parent-lib,
               on a library built from the parent commit: both loaded into this process, the same buffers, run as this, parent, parent,
               this within every round, so that drift hits both alike;
  committed    the same frames through ds2_ctc_beam_stream_commit before every feed but the first and
               ds2_ctc_beam_stream_feed_committed_f32, the bounds taken from the frames (no copy to the host: device time alone);
  commit       one commit launch alone, on the state after 250 frames (restored from a copy before every call, outside the events);
  class        BeamCTCDecoder.open_stream(capacity=256) against open_stream(capacity=256, commit=True), partial=False, finish(): what a
               caller sees, the commit's device-to-host copy and the host's bookkeeping included.
long: B = 1, T = 30 000, K = 16, plain, 1000-frame chunks: open_stream() against open_stream(commit=True), each with and without
partials; the node bytes and the partial's row width at the end against 12 * K * T and T.
Device events around each leg, the median of --reps calls after one warm-up, spread = max - min.  Nothing here times an hour-long
one-utterance decode.  Prints a table and one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def event_ms(fn, before=None):
    if before is not None:
        before()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 3), "spread": round(ms[-1] - ms[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libds2hip.so built from the parent commit")
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from asr_amd import _lib, ops
    from asr_amd.decoders import BeamCTCDecoder
    from make_synthetic_arpa import make
    from time_beam_stream import LABELS, planted
    dev = torch.device("cuda", 0)
    this = _lib.load()
    libs = {"this": this}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("ds2_ctc_beam_decode_f32", "ds2_ctc_beam_decode_lm_f32", "ds2_ctc_beam_stream_feed_f32", "ds2_ctc_beam_workspace_bytes"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        libs["parent"] = parent
    B, T, K, C = 64, 501, 100, len(LABELS)
    with tempfile.TemporaryDirectory() as tmp:
        arpa = os.path.join(tmp, "word3.arpa")
        make(arpa, "word", 3, 20000, 2000, 0)
        decoder_lm = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, lm_path=arpa, alpha=0.8, beta=1.0, cutoff_top_n=38, beam_width=K)
        with open(arpa) as f:
            text = f.read()
    lm = decoder_lm.lm
    unigrams = text[text.index("\\1-grams:"):text.index("\\2-grams:")].splitlines()[1:]
    words = [ln.split("\t")[1] for ln in unigrams if "\t" in ln and not ln.split("\t")[1].startswith("<")]
    x = torch.from_numpy(planted(B, T, words, 1)).to(dev)
    arms = {"plain": dict(cutoff_top_n=40, lm=None, alpha=0.0, beta=0.0), "word_lm": dict(cutoff_top_n=38, lm=lm, alpha=0.8, beta=1.0)}
    res = {"batch": {"B": B, "T": T, "K": K}, "reps": args.reps, "parent": bool(args.parent_lib), "legs": {}}
    lines = [f"# python scripts/time_beam_commit.py {' '.join(sys.argv[1:])}",
             "# ms: median of %d calls after a warm-up (spread = max - min)" % args.reps, f"{'leg':44s} {'ms':>10s} {'spread':>8s}"]

    def report(name, ms):
        r = summary(ms)
        res["legs"][name] = r
        lines.append(f"{name:44s} {r['ms']:10.3f} {r['spread']:8.3f}")
        print(lines[-1], flush=True)
        return r

    lab, off = (torch.empty((B, K, T), dtype=torch.int32, device=dev) for _ in range(2))
    lens, scores = torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.float32, device=dev)
    tail = torch.empty((2, B), dtype=torch.int32, device=dev)
    ws = torch.empty(this.ds2_ctc_beam_workspace_bytes(B, T, K), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for arm, search in arms.items():
        lm_args, hot_args, _keep = ops._beam_arm_args(search["lm"], search["alpha"], search["beta"], None, dev)
        head = (x.data_ptr(), x.stride(0), x.stride(1), B, T, C, None, 0, K, search["cutoff_top_n"], 1.0)
        state = ops.ctc_beam_stream_state(B, K, search["lm"], None, dev)
        nodes, nodes2 = ops.ctc_beam_stream_nodes(B, T, K, dev), ops.ctc_beam_stream_nodes(B, T, K, dev)

        def one_call(lib):
            out = (lab.data_ptr(), off.data_ptr(), lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(), s)
            rc = lib.ds2_ctc_beam_decode_f32(*head, *out) if search["lm"] is None else lib.ds2_ctc_beam_decode_lm_f32(*head, *lm_args, *out)
            assert rc == 0

        def feed(lib, t0, n, n_out, committed=False, rows=0):
            p = x[:, t0:t0 + n]
            args_ = (p.data_ptr() if n else None, x.stride(0), x.stride(1), B, n, C, None, 0, K, search["cutoff_top_n"], 1.0, *lm_args, *hot_args,
                     state.data_ptr(), state.numel(), nodes.data_ptr(), nodes.numel() * 4, T, rows)
            outs = (n_out, T, lab.data_ptr(), off.data_ptr(), lens.data_ptr(), scores.data_ptr(), tail[0].data_ptr(), tail[1].data_ptr(), s)
            rc = lib.ds2_ctc_beam_stream_feed_committed_f32(*args_, rows, *outs) if committed else lib.ds2_ctc_beam_stream_feed_f32(*args_, *outs)
            assert rc == 0, this.ds2_last_error()

        def stream(lib, chunk):
            state.zero_()
            for t0 in range(0, T, chunk):
                feed(lib, t0, min(chunk, T - t0), 0, rows=t0)
            feed(lib, T, 0, K, rows=T)

        def committed(chunk, width=T):
            nonlocal nodes, nodes2
            state.zero_()
            for t0 in range(0, T, chunk):
                if t0:
                    ops.ctc_beam_stream_commit(state, nodes, T, nodes2, T, K, search["lm"], None, width)
                    nodes, nodes2 = nodes2, nodes
                feed(this, t0, min(chunk, T - t0), 0, True, t0)      # (rows in use <= frames so far: a bound that needs no copy)
            feed(this, T, 0, K, True, T)

        one_call(this)
        want = [t.clone() for t in (lab, off, lens, scores)]
        for fn in (lambda: stream(this, 50), lambda: committed(50, 0)):   # the bits first (rows of width 0: no pair leaves, the read-out stays whole)
            fn()
            assert all(torch.equal(a, b) for a, b in zip((lab, off, lens), want[:3])) and torch.equal(scores.view(torch.int32), want[3].view(torch.int32))
        legs = [(f"B64 {arm} one-call", one_call)] + [(f"B64 {arm} stream {c}", lambda lib, c=c: stream(lib, c)) for c in (50, 250)]
        for name, fn in legs:
            times = {k: [] for k in libs}
            for k in libs:
                fn(libs[k])                                           # warm-up
            for _ in range(args.reps):
                for k in (("this", "parent", "parent", "this") if "parent" in libs else ("this",)):
                    times[k].append(event_ms(lambda: fn(libs[k])))
            got = {k: report(f"{name} [{k}]", v) for k, v in times.items()}
            if "parent" in got:
                lines.append(f"#   this - parent = {got['this']['ms'] - got['parent']['ms']:+.3f} ms")
                print(lines[-1])
        for c in (50, 250):
            committed(c)
            report(f"B64 {arm} committed stream {c}", [event_ms(lambda: committed(c)) for _ in range(args.reps)])
        stream(this, 250)
        state.zero_()
        feed(this, 0, 250, 0)
        saved = state.clone()
        info = ops.ctc_beam_stream_commit(state, nodes, T, nodes2, T, K, search["lm"], None, 250)[0].cpu()
        report(f"B64 {arm} one commit after 250 frames", [event_ms(lambda: ops.ctc_beam_stream_commit(state, nodes, T, nodes2, T, K, search["lm"], None, 250),
                                                                   lambda: state.copy_(saved)) for _ in range(args.reps + 1)][1:])
        lines.append(f"#   that commit: pairs committed mean {info[:, 0].float().mean():.1f}, live nodes mean {info[:, 1].float().mean():.0f} "
                     f"max {int(info[:, 1].max())} of {250 * K} written")
        print(lines[-1])
        dec = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, beam_width=K, cutoff_top_n=search["cutoff_top_n"], alpha=search["alpha"], beta=search["beta"])
        dec.lm = search["lm"]

        def klass(commit, chunk):
            st = dec.open_stream(batch=B, capacity=256, commit=commit)
            for t0 in range(0, T, chunk):
                st.feed(x[:, t0:t0 + chunk], partial=False)
            return st.finish(), st

        for c in (50, 250):
            for commit in (False, True):
                klass(commit, c)
                report(f"B64 {arm} class {c}{' commit' if commit else ''}", [event_ms(lambda: klass(commit, c)) for _ in range(args.reps)])
        (a, _), (b, st) = klass(False, 50), klass(True, 50)
        assert a[0] == b[0]
        lines.append(f"#   class 50 commit: {st.commits} commits, capacity {st.capacity} rows, live nodes max {max(st.live_nodes)}")
        print(lines[-1])
    if not args.skip_long:
        from time_transcribe_long import posteriors
        Tl, Kl = 30000, 16
        y = torch.from_numpy(posteriors(Tl, C, Tl)).to(dev)[None]
        dec = BeamCTCDecoder({c: i for i, c in enumerate(LABELS)}, beam_width=Kl)

        def long(commit, partial, max_lag=None):
            st = dec.open_stream(commit=commit, max_lag=max_lag)
            width = 0
            for t0 in range(0, Tl, 1000):
                st.feed(y[:, t0:t0 + 1000], partial=partial)
                width = max(st._lab) if commit else st.frames[0]
            cap = st.capacity
            return st.finish(), st, cap, width

        texts = {}
        for commit in (False, True):
            for partial in (False, True):
                out, st, cap, width = long(commit, partial)
                texts[commit] = out[0]
                report(f"B1 T30000 K16 class 1000{' commit' if commit else ''}{' +partial' if partial else ''}",
                       [event_ms(lambda: long(commit, partial)) for _ in range(3)])
            lines.append(f"#   {'commit' if commit else 'uncommitted'}: node bytes at the end {12 * Kl * cap} (12 * K * T = {12 * Kl * Tl}), the partial's row "
                         f"width at the end {width} (T = {Tl})" + (f", {st.commits} commits, live nodes at the last {st.live_nodes[0]}" if commit else ""))
            print(lines[-1])
        assert texts[False] == texts[True]
        out, st, cap, width = long(True, True, 500)                     # the stated bound: the text older than 500 frames is forced
        report("B1 T30000 K16 class 1000 commit max_lag 500 +partial", [event_ms(lambda: long(True, True, 500)) for _ in range(3)])
        wd, nw, cd, nc = dec.score_batch([out[0][0][0]], [texts[False][0][0]])[0].tolist()
        lines.append(f"#   max_lag 500: node bytes at the end {12 * Kl * cap}, the partial's row width at the end {width}, {st.commits} commits, {st.forced[0]} of "
                     f"them dropped a beam, live nodes at the last {st.live_nodes[0]}; against the exact stream's best text ({nw} words, {nc} characters) "
                     f"the forced one is {wd} word edits and {cd} character edits away (planted posteriors, no language model: not a WER)")
        print(lines[-1])
    lines.append(json.dumps(res))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
