"""GPU (-m gpu): what the posterior and waveform wrappers of asr_amd.ops say when they refuse a call.  Per wrapper this file holds ONE
valid call at the smallest shape and a list of variations with one fault each; every variation is refused on the host, and
(type(exc).__name__, str(exc)) is compared byte for byte with tests/golden/ops_wrapper_refusals.json (an accepted edge: "accepted" and
its result shapes).  `python tests/test_gpu_wrapper_refusals.py` records that file (record() below) from the ops.py that the
environment variable ASR_AMD_OPS_FILE names: the file of the commit BEFORE a change to these wrappers, loaded as a module of this
package, never the code under test.  The tests honour the variable too, so the recorded file can be shown to pass on both.

The wrappers share one host path per family (_posteriors, _packed_description, _upload_i32, _spectrogram), which may not reword a
refusal.  Two deliberate differences from the wrappers before that sharing, neither of them in the golden file:
  * a one-entry dimension of posteriors may carry the stride 0 (an expanded view); every consumer now takes it and returns the bits it
    returns on the contiguous copy (test_one_entry_dimension_with_stride_0) — greedy_decode, ctc_beam_decode, the aligners and
    ctc_star_row used to hand the 0 to the C entry: the aligner entries and the wildcard row refuse it ("bad dims"), the greedy and
    beam entries read row 0 for every b, harmless with B = 1;
  * with two or more faults in one call, which refusal wins is not pinned: every variation here has one fault, or faults whose order
    did not move."""
import importlib.util
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_wrapper_refusals.json")
OPS_ENV = "ASR_AMD_OPS_FILE"
B, T, C = 2, 10, 29
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    return _ops()


def _ops():
    """asr_amd.ops, or the ops.py that ASR_AMD_OPS_FILE names, loaded under the package (its relative imports are this tree's)"""
    path = os.environ.get(OPS_ENV)
    if not path:
        from asr_amd import ops
        return ops
    import asr_amd  # noqa: F401  (the parent package of the module made here)
    spec = importlib.util.spec_from_file_location("asr_amd._ops_recorded_from", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _probs(dev, shape=(B, T, C)):
    g = torch.Generator().manual_seed(7)
    return torch.softmax(torch.randn(shape, generator=g) * 3.0, -1).to(dev)


def _i32(dev, *v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _strided(t):
    """t's values in a tensor with the element stride 2"""
    wide = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    wide[::2] = t
    return wide[::2]


def _posterior_faults(x, name):
    """the variations of the posteriors themselves, under the wrapper's name for them"""
    return {f"{name}:cpu": {name: x.cpu()}, f"{name}:fp64": {name: x.double()}, f"{name}:2-D": {name: x[0]},
            f"{name}:classes-strided": {name: x.transpose(1, 2)}}


def _int_faults(**ints):
    """int64 / CPU / strided variations of named int32 device tensors (two or more entries each: a one-entry slice is contiguous)"""
    out = {}
    for (name, t), fault in zip(ints.items(), ("int64", "cpu", "strided")):
        assert t.numel() >= 2
        out[f"{name}:{fault}"] = {name: {"int64": t.long(), "cpu": t.cpu(), "strided": _strided(t)}[fault]}
    return out


def _option_faults(name, lo):
    return {f"{name}:bool": {name: True}, f"{name}:2.5": {name: 2.5}, f"{name}:below": {name: lo - 1}}


def _posterior_cases(dev):
    """{wrapper: (valid keyword arguments, {variation: overrides}, {accepted edge: overrides})}"""
    x = _probs(dev)
    xt = _probs(dev, (T, B, C)).transpose(0, 1)             # the model's (T,B,C)-backed eval output: no wrapper copies it
    three = _i32(dev, T, T, T)
    cases = {}
    for layout, p in (("", x), ("/tbc", xt)):
        cases["greedy_decode" + layout] = (dict(probs=p, sizes=None, blank=0), dict(_posterior_faults(p, "probs"), **{"sizes:B+1": dict(sizes=three)}), {})
    cases["ctc_beam_decode"] = (dict(probs=x, sizes=None, blank=0, beam_width=4),
                                dict(_posterior_faults(x, "probs"), **{"sizes:B+1": dict(sizes=three), "beam_width:0": dict(beam_width=0)}), {})
    seg = dict(probs=x, sizes=None, blank=0, threshold=0.9, min_gap=2, pad=1, max_len=8)
    bad = dict(_posterior_faults(x, "probs"), **{"probs:empty": dict(probs=x[:, :0]), "sizes:B+1": dict(sizes=three), "blank:C": dict(blank=C)})
    for name, lo in (("min_gap", 1), ("pad", 0), ("max_len", 2)):
        bad.update(_option_faults(name, lo))
    bad.update({"threshold:0": dict(threshold=0), "threshold:1.5": dict(threshold=1.5), "threshold:nan": dict(threshold=NAN),
                "max_segs:0": dict(max_segs=0)})
    cases["ctc_segment"] = (seg, bad, {})
    gather = dict(probs=xt, seg_b=_i32(dev, 0, 1), seg_start=_i32(dev, 0, 2), seg_len=_i32(dev, 4, 3), t_max=4)
    bad = dict(_posterior_faults(xt, "probs"), **{"probs:empty": dict(probs=xt[:, :0]), "seg_start:count": dict(seg_start=_i32(dev, 0, 2, 3))})
    bad.update(_int_faults(seg_b=gather["seg_b"], seg_start=gather["seg_start"], seg_len=gather["seg_len"]))
    bad.update(_option_faults("t_max", 1))
    none = torch.empty(0, dtype=torch.int32, device=dev)
    cases["ctc_segment_gather"] = (gather, bad, {"S=0": dict(seg_b=none, seg_start=none, seg_len=none)})
    kws = dict(x=x, kw_labels=_i32(dev, 3, 1, 20, 4, 15), kw_off=_i32(dev, 0, 3), kw_lens=_i32(dev, 3, 2), max_kw_len=3,
               thr=torch.tensor([-1.0, -1.0], device=dev), in_lens=None, is_log=False, max_hits=4)
    bad = dict(_posterior_faults(x, "x"), **{"in_lens:B+1": dict(in_lens=three), "kw_off:count": dict(kw_off=_i32(dev, 0, 3, 5)),
                                             "thr:fp64": dict(thr=kws["thr"].double()), "thr:cpu": dict(thr=kws["thr"].cpu()),
                                             "max_kw_len:64": dict(max_kw_len=64), "max_hits:0": dict(max_hits=0)})
    bad.update(_int_faults(kw_labels=kws["kw_labels"], kw_off=kws["kw_off"], kw_lens=kws["kw_lens"]))
    bad.update(_int_faults(in_lens=_i32(dev, T, T)))
    cases["ctc_keyword_search"] = (kws, bad, {})
    for layout, p in (("", x), ("/tbc", xt)):
        align = dict(x=p, targets=_i32(dev, 3, 1, 20, 4), tgt_off=_i32(dev, 0, 3), in_lens=None, tgt_lens=_i32(dev, 3, 1), max_u=3, is_log=False)
        bad = dict(_posterior_faults(p, "x"), **{"in_lens:B+1": dict(in_lens=three), "tgt_off:count": dict(tgt_off=_i32(dev, 0, 3, 4))})
        bad.update(_int_faults(targets=align["targets"], tgt_off=align["tgt_off"], tgt_lens=align["tgt_lens"]))
        cases["ctc_forced_align" + layout] = (align, bad, {})
    row = dict(x=x, in_lens=None, is_log=False, star_penalty=-0.5)
    bad = dict(_posterior_faults(x, "x"), **{"in_lens:B+1": dict(in_lens=three), "star_penalty:0.25": dict(star_penalty=0.25),
                                             "star_penalty:nan": dict(star_penalty=NAN)})
    bad.update(_int_faults(in_lens=_i32(dev, T, T)))
    cases["ctc_star_row"] = (row, bad, {})
    return cases


def _waveform_cases(dev, ops):
    packed = torch.arange(32, dtype=torch.int16, device=dev)
    unpack = dict(packed=packed, offsets=[0, 16], lengths=[9, 16], src_index=[1, 0], n_max=16)
    bad = {"packed:cpu": dict(packed=packed.cpu()), "packed:int32": dict(packed=packed.int()), "packed:2-D": dict(packed=packed.view(4, 8)),
           "packed:strided": dict(packed=_strided(packed)), "packed:31": dict(packed=packed[:31]), "offsets:-8": dict(offsets=[-8, 16]),
           "offsets:4": dict(offsets=[4, 16]), "lengths:-1": dict(lengths=[-1, 16]), "past-the-end": dict(offsets=[0, 24]),
           "src_index:-1": dict(src_index=[-1, 0]), "src_index:B": dict(src_index=[2, 0]), "B=0": dict(offsets=[], lengths=[], src_index=[]),
           "offsets:count": dict(offsets=[0]), "lengths:count": dict(lengths=[9]), "src_index:count": dict(src_index=[1])}
    cases = {"wave_unpack": (unpack, dict(bad, **{"lengths:above-n_max": dict(n_max=8)}), {"n_max=0": dict(lengths=[0, 0], n_max=0)})}
    resample = dict(packed=packed, offsets=[0, 16], lengths=[9, 16], rates=[16000, 16000], src_index=[1, 0], target_rate=16000, n_out_max=16)
    more = {"rates:count": dict(rates=[16000]), "rates:16001": dict(rates=[16001, 16000]), "rates:1000": dict(rates=[1000, 16000]),
            "n_out:wrong": dict(n_out=[9, 15]), "n_out_max:small": dict(n_out_max=8)}
    cases["wave_resample"] = (resample, dict(bad, **more), {"n_out_max=0": dict(lengths=[0, 0], n_out_max=0)})
    cases["resample_ratio"] = (dict(fs=8000, ft=16000), {"fs:bool": dict(fs=True), "fs:16000.5": dict(fs=16000.5), "fs:0": dict(fs=0),
                                                         "ft:bool": dict(ft=True), "ft:0": dict(ft=0)}, {})
    audio = _probs(dev, (2, 16)) - 0.05
    rir = torch.tensor([1.0, 0.5, 0.25, 0.125], device=dev)
    reverb = dict(audio=audio, n_samples=[9, 16], rir=rir, rir_base=[0, 0], rir_taps=[4, 0], n_max=16)
    bad = {"audio:cpu": dict(audio=audio.cpu()), "rir:cpu": dict(rir=rir.cpu()), "n:above-n_max": dict(n_max=8), "n_max:above-row": dict(n_max=17),
           "taps:above-max": dict(rir_taps=[ops.reverb_max_taps() + 1, 0]), "slice:past-bank": dict(rir_base=[1, 0]),
           "rir:None": dict(rir=None), "rir_taps:count": dict(rir_taps=[4])}
    cases["reverb"] = (reverb, bad, {"n_max=0": dict(n_samples=[0, 0], n_max=0)})
    tempo = dict(audio=audio, n_samples=[9, 16], tempo=[1.0, 1.0], gain=[0.0, 0.0], sample_rate=16000)
    cases["tempo_gain"] = (tempo, {"tempo:count": dict(tempo=[1.0]), "n:beyond-row": dict(n_samples=[9, 17]), "tempo:0.4": dict(tempo=[0.4, 1.0])}, {})
    wave = _probs(dev, (2, 480)) - 0.002
    aug = dict(audio=wave, n_samples=torch.tensor([480, 400]), n_fft=320, hop=160)
    noise = dict(noise=wave[0], noise_base=[0, 0], noise_period=[100, 100], noise_start=[0, 0], noise_level=[0.1, 0.0])
    bad = {"noise:three-of-four": dict(noise, noise_level=None), "freq_masks:(B,1,3)": dict(freq_masks=[[[0, 1, 2]], [[0, 1, 2]]]),
           "noise_base:B+1": dict(noise, noise_base=[0, 0, 0])}
    cases["spectrogram_augmented"] = (aug, bad, {})
    return cases


def _outcome(fn, args):
    """("accepted", result shapes) or (exception class, text) of one call"""
    try:
        out = fn(**args)
    except Exception as e:
        return [type(e).__name__, str(e)]
    out = out if isinstance(out, tuple) else (out,)
    return ["accepted", json.dumps([list(t.shape) if torch.is_tensor(t) else t for t in out])]


def _outcomes(ops, dev):
    """{wrapper: {variation: outcome}}: the valid call first (it must be accepted), then every variation and every accepted edge"""
    got = {}
    for who, (ok, bads, edges) in dict(_posterior_cases(dev), **_waveform_cases(dev, ops)).items():
        fn = getattr(ops, who.split("/")[0])
        assert _outcome(fn, ok)[0] == "accepted", (who, _outcome(fn, ok))
        got[who] = {}
        for name, bad in dict(bads, **edges).items():
            res = _outcome(fn, dict(ok, **bad))
            assert (res[0] == "accepted") == (name in edges), (who, name, res)
            assert "libds2hip call failed" not in res[1], (who, name, res)      # refused by the wrapper, not by the entry behind it
            got[who][name] = res
    torch.cuda.synchronize()
    return got


def test_refusals_read_as_recorded(ops, dev):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = _outcomes(ops, dev)
    assert sorted(got) == sorted(golden), "the golden file and the wrappers of this file differ"
    for who in got:
        assert sorted(got[who]) == sorted(golden[who]), (who, "the golden file and the cases of this file differ")
        for name, res in got[who].items():
            assert [r.encode() for r in res] == [r.encode() for r in golden[who][name]], (who, name, res, golden[who][name])


CONSUMERS = ("greedy_decode", "ctc_beam_decode", "ctc_segment", "ctc_segment_gather", "ctc_keyword_search", "ctc_forced_align", "ctc_star_row")


@pytest.mark.parametrize("who", CONSUMERS)
def test_one_entry_dimension_with_stride_0(ops, dev, who):
    """probs[None] of one recording, and the same values as an expanded view whose batch stride is 0: the bits of the contiguous copy."""
    p = _probs(dev, (T, C))
    one = _i32(dev, 0)
    args = dict(greedy_decode=dict(), ctc_beam_decode=dict(beam_width=4), ctc_segment=dict(min_gap=2, pad=1, max_len=8),
                ctc_segment_gather=dict(seg_b=one, seg_start=_i32(dev, 2), seg_len=_i32(dev, 5), t_max=6),
                ctc_keyword_search=dict(kw_labels=_i32(dev, 3, 1, 20), kw_off=one, kw_lens=_i32(dev, 3), max_kw_len=3,
                                        thr=torch.tensor([-1.0], device=dev)),
                ctc_forced_align=dict(targets=_i32(dev, 3, 1, 20), tgt_off=one, in_lens=None, tgt_lens=_i32(dev, 3), max_u=3, is_log=False),
                ctc_star_row=dict(in_lens=None, is_log=False, star_penalty=-0.5))[who]
    fn = getattr(ops, who)
    views = (p[None].clone(), p[None], p.as_strided((1, T, C), (0, C, 1)))          # (expand() itself gives a new dimension of one entry a stride)
    assert views[2].stride(0) == 0 and views[0].is_contiguous()
    def defined(out):
        """greedy_decode defines the first lengths[b] entries of a row only: the rest is zeroed before the comparison"""
        if who != "greedy_decode":
            return out
        ids, offs, lens = out
        keep = torch.arange(T, device=dev)[None] < lens[:, None]
        return ids * keep, offs * keep, lens
    want, *rest = (defined(fn(v, **args)) for v in views)
    for got in rest:
        for a, b in zip(want, got) if isinstance(want, tuple) else ((want, got),):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    torch.cuda.synchronize()


def record():
    assert os.environ.get(OPS_ENV), f"set {OPS_ENV} to the ops.py of the commit before the change"
    golden = _outcomes(_ops(), torch.device("cuda", 0))
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in golden.values())} outcomes of {len(golden)} wrappers -> {GOLDEN}")


if __name__ == "__main__":
    record()
