"""What the CTC entries of the library say when they refuse a call, without a GPU: the four aligner entries, the wildcard row, the
three one-call beam-search entries and the two streaming feed entries (each in its plain, LM and hotword form) share their argument
checks, and this file holds, per entry and form, one valid argument set and a list of variations with ONE fault each.  Every variation returns non-zero before any HIP call (the pointers are dummy addresses), and
ds2_last_error() is compared byte for byte with tests/golden/ctc_entry_refusals.json, which `python tests/test_cpu_ctc_entries.py`
records (record() below) from the library that DS2_LIB_PATH names: the build of the commit BEFORE a change to these entries, never
the code under test."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_entry_refusals.json")
P = 4096                                    # any non-null address: no call below gets as far as reading through it
NAN, INF = float("nan"), float("inf")
B, T, C, U, K = 2, 10, 29, 3, 8
BIG_C = 16384                               # the most classes an entry takes: with K = 256 the LM arm's LDS layout does not fit
LABELS = ["_"] + [chr(65 + i) for i in range(27)] + [" "]               # C = 29 classes, the blank first and the space last


def _lib():
    from asr_amd import _lib
    return _lib.load()


def _hot(labels=LABELS):
    from asr_amd.decoders.hotwords import Hotwords
    return Hotwords(["BAD", ("ACE", 2.0)], labels, 0).packed


def _hot_big():
    """an automaton packed for BIG_C classes"""
    from asr_amd.decoders.hotwords import Hotwords
    return Hotwords([[2, 1, 4]], {"_": 0, "~": BIG_C - 1}, 0).packed


def _align_cases(lib, entry):
    """(valid arguments, variations) of one of the five aligner entries"""
    star, tiled, row = "star" in entry, "tiled" in entry, "row" in entry
    ok = dict(x=P, ld_b=T * C, ld_t=C, B=B, T=T, C=C, is_log=1)
    bad = [dict(x=None), dict(B=0), dict(B=-1), dict(T=0), dict(T=-1), dict(C=0), dict(C=-1), dict(ld_b=0), dict(ld_t=0), dict(ld_t=-C),
           dict(is_log=2), dict(is_log=-1)]
    penalties = [dict(penalty=v) for v in (0.25, 1e-3, NAN, -INF, INF)]
    if row:
        ok.update(in_lens=None, penalty=-0.5, g=P, stream=None)
        return ok, bad + [dict(g=None)] + penalties
    ok.update(targets=P, off=P, in_lens=None, lens=P, max_u=U)
    bad += [dict(off=None), dict(lens=None), dict(max_u=-1), dict(targets=None), dict(ts=None), dict(te=None), dict(lp=None),
            dict(score=None), dict(states=None), dict(ws=None)]
    if tiled:
        ok.update(tf=8, tp=64)
        bad += [dict(tf=12), dict(tf=-8), dict(tp=32), dict(tp=-64), dict(tp=2048)]
    else:
        ok.update(variant=0)
        bad += [dict(variant=3), dict(variant=-1), dict(variant=1, max_u=64)]
    if star:
        ok.update(penalty=-0.5, flags=None)
        bad += penalties
    shape = (ok["tf"], ok["tp"]) if tiled else ()
    need = getattr(lib, entry[:-len("f32")] + "workspace_bytes")(B, T, U, *shape)
    assert need > 0
    ok.update(score=P, states=P, ts=P, te=P, lp=P, ws=P, wsb=need, stream=None)
    return ok, bad + [dict(wsb=need - 1), dict(wsb=0)]


def _beam_cases(lib, entry):
    """(valid arguments, variations) of one of the three beam-search entries"""
    lm, hot = entry != "ds2_ctc_beam_decode_f32", "hot" in entry
    kmax, need = lib.ds2_ctc_beam_max_width(), lib.ds2_ctc_beam_workspace_bytes(B, T, K)
    ok = dict(probs=P, ld_b=T * C, ld_t=C, B=B, T=T, C=C, sizes=None, blank=0, K=K, top_n=40, cutoff_prob=1.0)
    bad = [dict(probs=None), dict(labels=None), dict(offsets=None), dict(lens=None), dict(scores=None), dict(ws=None), dict(B=0), dict(B=-1),
           dict(T=0), dict(T=-1), dict(T=1 << 20), dict(K=0), dict(K=-1), dict(K=kmax + 1), dict(C=1), dict(C=0), dict(C=16385),
           dict(blank=C), dict(blank=-1), dict(top_n=0), dict(top_n=-3), dict(cutoff_prob=NAN), dict(wsb=need - 1), dict(wsb=0)]
    if lm:
        ok.update(lm=P, lm_bytes=4096, order=3, mode=1, space=C - 1, alpha=0.5, beta=0.1)
        bad += [dict(order=0), dict(order=7), dict(mode=0), dict(mode=3), dict(lm_bytes=63), dict(mode=2, space=0), dict(mode=2, space=-1),
                dict(mode=2, space=C), dict(alpha=NAN), dict(alpha=INF), dict(beta=NAN), dict(beta=-INF)]
        grid = kmax * (min(40, C - 1) + 2)
        assert grid > lib.ds2_ctc_beam_lm_max_candidates()
        bad += [dict(K=kmax, wsb=lib.ds2_ctc_beam_workspace_bytes(B, T, kmax))]
        if not hot:                                                       # within the candidate slots (256 * 16), too large for the LDS
            bad += [dict(C=BIG_C, K=kmax, top_n=14, wsb=lib.ds2_ctc_beam_workspace_bytes(B, T, kmax))]
        bad += [dict(hot=None)] if hot else [dict(lm=None)]               # (the hotword entry takes no language model as hot-only)
    keep = []
    if hot:
        blob = _hot()
        other, magic = _hot(LABELS[:-1] + ["'", " "]), blob.copy()
        magic.view(np.int32)[0] ^= 1
        big = _hot_big()
        keep += [blob, other, magic, big]
        ok.update(hot=P, hot_host=blob.ctypes.data, hot_bytes=blob.nbytes)
        bad += [dict(C=BIG_C, K=kmax, top_n=14, wsb=lib.ds2_ctc_beam_workspace_bytes(B, T, kmax), hot_host=big.ctypes.data, hot_bytes=big.nbytes)]
        bad += [dict(hot_host=None), dict(hot_bytes=63), dict(hot_bytes=0), dict(hot_bytes=blob.nbytes - 1), dict(hot_host=magic.ctypes.data),
                dict(hot_host=other.ctypes.data, hot_bytes=other.nbytes)]
    ok.update(labels=P, offsets=P, lens=P, scores=P, ws=P, wsb=need, stream=None)
    return ok, bad, keep


def _stream_cases(lib, entry, form):
    """(valid arguments, variations) of one of the two streaming feed entries in its "plain", "lm" or "hot" form: the one-call entries'
    variations that apply to a stream (the node buffer is its workspace, `cap` its T) and the stream's own"""
    lm, hot, committed = form != "plain", form == "hot", "committed" in entry
    kmax, cap, bound = lib.ds2_ctc_beam_max_width(), 16, 2
    state_need = lambda k=K, l=lm, h=hot: lib.ds2_ctc_beam_stream_state_bytes(B, k, l, h)
    nodes_need = lambda k=K, c=cap: lib.ds2_ctc_beam_stream_nodes_bytes(B, c, k)
    wide = dict(K=kmax, state_bytes=state_need(kmax), nodes_bytes=nodes_need(kmax))
    ok = dict(probs=P, ld_b=T * C, ld_t=C, B=B, T=T, C=C, sizes=None, blank=0, K=K, top_n=40, cutoff_prob=1.0,
              lm=None, lm_bytes=0, order=0, mode=0, space=-1, alpha=0.0, beta=0.0, hot=None, hot_host=None, hot_bytes=0,
              state=P, state_bytes=state_need(), nodes=P, nodes_bytes=nodes_need(), cap=cap, bound=bound)
    bad = [dict(probs=None), dict(labels=None), dict(offsets=None), dict(lens=None), dict(scores=None), dict(nodes=None), dict(state=None),
           dict(stable_len=None), dict(frames=None), dict(B=0), dict(B=-1), dict(T=-1), dict(T=1 << 20), dict(K=0), dict(K=-1),
           dict(K=kmax + 1), dict(wide, K=kmax + 1), dict(C=1), dict(C=0), dict(C=16385), dict(blank=C), dict(blank=-1), dict(top_n=0),
           dict(top_n=-3), dict(cutoff_prob=NAN), dict(cap=0), dict(bound=-1), dict(cap=1 << 20, nodes_bytes=nodes_need(K, 1 << 20)),
           # the stream's own
           dict(state_bytes=state_need() - 1), dict(state_bytes=0), dict(nodes_bytes=nodes_need() - 1), dict(nodes_bytes=0),
           dict(cap=bound + T - 1), dict(n_out=K + 1), dict(n_out=-1), dict(W=bound + T - 1), dict(W=0), dict(T=0, n_out=0)]
    if committed:
        ok.update(labels_bound=bound)
        bad += [dict(labels_bound=-1), dict(labels_bound=bound + 1)]
    if lm:
        ok.update(lm=P, lm_bytes=4096, order=3, mode=1, space=C - 1, alpha=0.5, beta=0.1)
        bad += [dict(order=0), dict(order=7), dict(mode=0), dict(mode=3), dict(lm_bytes=63), dict(mode=2, space=0), dict(mode=2, space=-1),
                dict(mode=2, space=C), dict(alpha=NAN), dict(alpha=INF), dict(beta=NAN), dict(beta=-INF)]
        assert kmax * (min(40, C - 1) + 2) > lib.ds2_ctc_beam_lm_max_candidates()
        bad += [wide]
        if not hot:
            bad += [dict(wide, C=BIG_C, top_n=14)]
    keep = []
    if hot:
        blob, big = _hot(), _hot_big()
        other, magic = _hot(LABELS[:-1] + ["'", " "]), blob.copy()
        magic.view(np.int32)[0] ^= 1
        keep += [blob, other, magic, big]
        ok.update(hot=P, hot_host=blob.ctypes.data, hot_bytes=blob.nbytes)
        bad += [dict(hot_host=None), dict(hot_bytes=63), dict(hot_bytes=0), dict(hot_bytes=blob.nbytes - 1), dict(hot_host=magic.ctypes.data),
                dict(hot_host=other.ctypes.data, hot_bytes=other.nbytes),
                dict(wide, C=BIG_C, top_n=14, hot_host=big.ctypes.data, hot_bytes=big.nbytes),
                # hot-only (no language model): the full grid and the hotword state all the same
                dict(wide, lm=None), dict(wide, lm=None, C=BIG_C, top_n=14, hot_host=big.ctypes.data, hot_bytes=big.nbytes)]
    ok.update(n_out=K, W=bound + T, labels=P, offsets=P, lens=P, scores=P, stable_len=P, frames=P, stream=None)
    return ok, bad, keep


STREAM_ENTRIES = ("ds2_ctc_beam_stream_feed_f32", "ds2_ctc_beam_stream_feed_committed_f32")
ENTRIES = ("ds2_ctc_align_f32", "ds2_ctc_align_tiled_f32", "ds2_ctc_align_star_f32", "ds2_ctc_align_star_tiled_f32",
           "ds2_ctc_align_star_row_f32", "ds2_ctc_beam_decode_f32", "ds2_ctc_beam_decode_lm_f32", "ds2_ctc_beam_decode_hot_f32") + STREAM_ENTRIES


def _name(bad):
    """the key of a variation in the golden file; a host address (of a hotword blob made here) is not spelled out"""
    return ",".join(f"{k}={'<blob>' if k == 'hot_host' and v is not None else v}" for k, v in bad.items())


def _refusals(lib, entry):
    """{variation: (return code, message)} of one entry, by calling it; a stream entry's variations are named <form>/<variation>"""
    if entry in STREAM_ENTRIES:
        forms = [(form + "/", *_stream_cases(lib, entry, form)) for form in ("plain", "lm", "hot")]
    else:
        forms = [("", *(_beam_cases if "beam" in entry else _align_cases)(lib, entry))]
    out = {}
    for prefix, ok, bads, *keep in forms:
        for bad in bads:
            assert set(bad) <= set(ok), (entry, bad)
            name = prefix + _name(bad)
            assert name not in out, (entry, name)
            rc = getattr(lib, entry)(*dict(ok, **bad).values())
            out[name] = (rc, lib.ds2_last_error().decode())
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_read_as_recorded(entry):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden) == set(ENTRIES)
    got = _refusals(_lib(), entry)
    assert sorted(got) == sorted(golden[entry]), "the golden file and the cases of this file differ"
    for name, (rc, msg) in got.items():
        assert rc != 0, (entry, name)
        assert msg.encode() == golden[entry][name].encode(), (entry, name, msg, golden[entry][name])
        assert msg.startswith(entry + ": "), (entry, name, msg)


def record():
    lib = _lib()
    golden = {}
    for entry in ENTRIES:
        got = _refusals(lib, entry)
        assert all(rc != 0 for rc, _ in got.values()), entry
        golden[entry] = {name: msg for name, (_, msg) in got.items()}
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in golden.values())} refusals of {len(golden)} entries -> {GOLDEN}")


if __name__ == "__main__":
    record()
