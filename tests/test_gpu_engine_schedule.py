"""-m gpu: the schedule of the train step — which kernel wrapper asr_amd.engine calls, with which operands, on which stream, behind which
event — against tests/golden/engine_schedules.json, recorded with this same file (DS2_ENGINE_SCHEDULE_RECORD=<output file>) before the engine
was split into stages.  A case runs two consecutive engine.forward + ops.ctc_loss + engine.backward steps on a seeded model and logs, in order:
  * every outermost call into asr_amd.ops (calls from ops into ops are left out): name, current stream (main = the compute stream, side = the
    engine's side stream), every tensor argument as dtype[shape]/strides (strides left out when contiguous), every other argument by value,
    tuples and lists element by element, no pointers.  ops.rnn_last_path() is logged with the value it returned.  Three host-only queries
    that enqueue nothing and read nothing that changes within a step are left out (_pad8, rnn_ctx_key, wgrad_fits_beside_bwd_recurrence):
    where a shape decision is evaluated is not part of the schedule.  Every case runs on a recurrence context of its own, so that what
    rnn_last_path() reports does not depend on the case that ran before;
  * every Stream.wait_stream / Stream.wait_event / Event.record / Tensor.record_stream (events numbered by their order of creation within the step);
  * every on_bucket(name) call with the stream it was called on;
  * ops.rnn_last_path() after each forward and each backward.
The values computed are not looked at (the parity tests do that).  Each case names the records that show its branch was reached, and the
golden must contain them: a golden that silently misses a branch fails.  A starved persistent launch fails the case by its own message."""
import inspect
import json
import os
import re
import sys
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "engine_schedules.json")
QUERIES = ("_pad8", "rnn_ctx_key", "wgrad_fits_beside_bwd_recurrence")
RAW_POINTERS = {"gemm_raw": (5, 8, 11)}                    # positional arguments that are device addresses

GRU256 = dict(rnn="gru", hidden=256, layers=3, B=16, tin=41)
IDLE = dict(rnn="gru", hidden=1024, layers=3, B=48, tin=41)
F32_256 = dict(rnn="gru", hidden=256, layers=3, B=16, tin=65, precision="fp32")
# name -> (model and batch, records (regular expressions) that show the case's branch was reached).  T = 21 output frames for Tin = 41.
CASES = {
    # persistent recurrences, deferred schedule, grouped split-K weight gradients with the folded BatchNorm's epilogue, BatchNorm backward in the recurrence
    "bf16 gru H256 L3 B16": (GRU256, [r"^main gemm_bf16_tn_splitk_group\(.*epilogue=", r"^main rnn_bwd_bn\(3, ", r"^main center_colstats\("]),
    # three products per layer, no d(hn)
    "bf16 lstm H256 L3 B16": (dict(GRU256, rnn="lstm"), [r"^main rnn_bwd_bn\(4, .*dhn_bf16=None", r"^main gemm_bf16_tn_splitk_group\("]),
    # the tanh cell has no aux: (gates, dyn, x, mean, var, gamma, sums, gx = None, aux = None, ...)
    "bf16 rnn H256 L2 B16": (dict(GRU256, rnn="rnn", layers=2), [r"^main rnn_bwd_bn\(1, (\S+, ){6}None, None, "]),
    # 2 x 3 x 32 = 192 of 256 CUs in the backward recurrence: the grouped launch of the layer above runs beside it
    "bf16 gru H1024 L3 B48 idle CUs": (IDLE, [r"^side gemm_bf16_tn_splitk_group\("]),
    # B % 8 != 0: fp32 dGx, cast in both orientations with the bias sums
    "bf16 gru H256 L2 B12": (dict(GRU256, layers=2, B=12), [r"^main cast_bf16_both\(f32\[\S+, colsum=True\)"]),
    # H = 20 has no persistent kernel: the operand passes + NT-form weight gradients, on the compute stream (the backward recurrence of the top
    # layer has reported before the first passes are issued; the passes on the side stream are what the WGRAD_TN=False variant below reaches)
    "bf16 gru H20 L3 B16 no persistent kernel": (dict(GRU256, hidden=20), [r"^main transpose_bf16\(\S+, colsum=", r"^main gemm_bf16_nt_pair\("]),
    # Tin = 1: T = 1, the layer-wise bf16 backward (M = 16 rows) and no dW_hh product at all
    "bf16 gru H256 L2 B16 T1": (dict(GRU256, layers=2, tin=1), [r"^main rnn_bwd\(3, .*dgx_bf16=bf16\[16,1536\]"]),
    # T = 33, M = 528: split-bf16 GEMMs, split recurrences, split conv backward; the second step defers off_path behind the next recurrence (side stream)
    "fp32 gru H256 L3 B16 M528": (F32_256, [r"^main split_bf16\(", r"^main padcast_bf16\(", r"^side gemm_bf16_tn_splitk_group\(", r"^main rnn_bwd\(3, .*bf16=2"]),
    # H % 8 == 4: fp32-MFMA GEMMs and the pointer form of dW_hh
    "fp32 gru H36 L2 B3": (dict(rnn="gru", hidden=36, layers=2, B=3, tin=41, precision="fp32"), [r"^main gemm_raw\(", r"^main gemm\("]),
    "fp32 lstm H32 L2 B4": (dict(rnn="lstm", hidden=32, layers=2, B=4, tin=41, precision="fp32"), [r"^main rnn_bwd\(4, ", r"^main gemm_raw\("]),
    "bf16 gru H256 L3 B16 eval forward": (dict(GRU256, forward_only=True), [r"^main cast_bf16\(\S+, ld=", r"^main bn1d_apply_bf16\("]),
    "fp32 gru H256 L3 B16 eval forward": (dict(F32_256, forward_only=True), [r"^main rnn_pack\(", r"^main bn1d_apply\("]),
    # ---- bucket callbacks: a plain recording callback, and the form of a reducer that orders its collectives into the compute stream
    "bf16 gru H256 L3 B16 buckets": (dict(GRU256, buckets="plain"), [r"^main bucket\(rnns\.0\)", r"^main bucket\(conv\)"]),
    "bf16 gru H1024 L3 B48 idle CUs buckets": (dict(IDLE, buckets="plain"), [r"^side bucket\(rnns\.2\)", r"^main wait_stream\(side\)"]),
    "fp32 gru H256 L3 B16 M528 buckets": (dict(F32_256, buckets="plain"), [r"^side bucket\(rnns\.1\)"]),
    "bf16 gru H256 L3 B16 serial buckets": (dict(GRU256, buckets="serial"), [r"^main bucket\(rnns\.0\)"]),
    "bf16 gru H1024 L3 B48 idle CUs serial buckets": (dict(IDLE, buckets="serial"), [r"^side gemm_bf16_tn_splitk_group\(", r"^main bucket\(rnns\.2\)"]),
    # ---- switch variants (module attributes, set before the step)
    "bf16 gru H256 L3 B16 WGRAD_SIDE=0": (dict(GRU256, switches=dict(WGRAD_SIDE="0")), [r"^main gemm_bf16_tn_pair\(", r"^main scale_rank1_\("]),
    "bf16 gru H256 L3 B16 WGRAD_SIDE=main": (dict(GRU256, switches=dict(WGRAD_SIDE="main")), [r"^main gemm_bf16_tn_group\("]),
    # (the co-resident kernel fits beside the K-split recurrence of H = 1024: the shape of its own bit-equality test)
    "bf16 gru H1024 L3 B48 WGRAD_SIDE=1": (dict(IDLE, switches=dict(WGRAD_SIDE="1")), [r"^side gemm_bf16_tn_group\("]),
    "bf16 gru H256 L3 B16 WGRAD_TN=False": (dict(GRU256, switches=dict(WGRAD_TN=False)), [r"^side cast_transpose_bf16\(", r"^main gemm_bf16_nt_pair\("]),
    "bf16 gru H256 L3 B16 BN_FOLD=False": (dict(GRU256, switches=dict(BN_FOLD=False)), [r"^main bn1d_apply_bf16\(", r"^main add_colstats\("]),
    "bf16 gru H1024 L3 B48 WGRAD_IDLE=False": (dict(IDLE, switches=dict(WGRAD_IDLE=False)), [r"^main gemm_bf16_tn_splitk_group\("]),
    "fp32 gru H256 L3 B16 M528 F32_CONV=f32": (dict(F32_256, switches=dict(F32_CONV="f32")), [r"^main conv2_dgrad\(", r"^main split_bf16\("]),
    "fp32 gru H256 L3 B16 M528 F32_GEMM=f32": (dict(F32_256, switches=dict(F32_GEMM="f32")), [r"^side gemm_raw\(", r"^main padcast_bf16\("]),
    "fp32 gru H256 L3 B16 M528 F32_RNN=f32": (dict(F32_256, switches=dict(F32_RNN="f32")), [r"^main rnn_bwd\(3, .*bf16=0", r"^main split_bf16\("]),
}
CLASSES, FREQ = 29, 161
_MODELS = {}


def _tensor(t):
    dt = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64", torch.float64: "f64"}.get(t.dtype, str(t.dtype))
    s = f"{dt}[{','.join(map(str, t.shape))}]"
    return s if t.is_contiguous() else s + "/" + ",".join(map(str, t.stride()))


class _Log:
    """the ordered record of one step; `depth` > 0 inside a wrapped call (nothing below an outermost call is logged)"""

    def __init__(self, main, side):
        self.main, self.side, self.lines, self.depth, self.events = main, side, [], 0, []

    def stream(self, s=None):
        s = torch.cuda.current_stream() if s is None else s
        return "main" if s == self.main else ("side" if s == self.side else "other")

    def desc(self, v):
        if isinstance(v, torch.Tensor):
            return _tensor(v)
        if isinstance(v, (tuple, list)):
            return ("(%s)" if isinstance(v, tuple) else "[%s]") % ",".join(self.desc(e) for e in v)
        if isinstance(v, torch.cuda.Event):
            return next((f"event{i}" for i, e in enumerate(self.events) if e is v), "event?")
        if isinstance(v, torch.cuda.Stream):
            return self.stream(v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, (torch.device, torch.dtype)):
            return str(v)
        return getattr(v, "__name__", type(v).__name__)

    def add(self, text, stream=None):
        self.lines.append(f"{self.stream(stream)} {text}")


def _wrap(log, name, fn, pre=None, post=None):
    def wrapped(*a, **k):
        if log[0] is None or log[0].depth:
            return fn(*a, **k)
        lg = log[0]
        lg.depth += 1
        try:
            if pre is not None:
                pre(lg, a, k)
            out = fn(*a, **k)
        finally:
            lg.depth -= 1
        if post is not None:
            post(lg, a, k, out)
        return out
    wrapped.__name__ = name
    return wrapped


@pytest.fixture
def recorder(monkeypatch):
    """wraps asr_amd.ops and the stream / event methods; log[0] is the _Log in use (None: nothing is recorded)"""
    from asr_amd import ops
    log = [None]

    def op_pre(name):
        def pre(lg, a, k):
            if name == "rnn_last_path":
                return
            ptr = RAW_POINTERS.get(name, ())
            args = ["ptr" if i in ptr else lg.desc(v) for i, v in enumerate(a)] + [f"{n}={lg.desc(v)}" for n, v in k.items()]
            lg.add(f"{name}({', '.join(args)})")
        return pre

    for name, fn in list(vars(ops).items()):
        if inspect.isfunction(fn) and fn.__module__ == ops.__name__:
            post = (lambda lg, a, k, out: lg.add(f"rnn_last_path() = {out}")) if name == "rnn_last_path" else None
            monkeypatch.setattr(ops, name, _wrap(log, name, fn, None if name in QUERIES else op_pre(name), post))
    new_event = torch.cuda.Event.__new__

    def event_new(cls, *a, **k):
        ev = new_event(cls, *a, **k)
        if log[0] is not None and not log[0].depth:
            log[0].events.append(ev)
        return ev
    monkeypatch.setattr(torch.cuda.Event, "__new__", event_new)
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", _wrap(log, "wait_stream", torch.cuda.Stream.wait_stream,
                                                                lambda lg, a, k: lg.add(f"wait_stream({lg.stream(a[1])})", a[0])))
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", _wrap(log, "wait_event", torch.cuda.Stream.wait_event,
                                                               lambda lg, a, k: lg.add(f"wait_event({lg.desc(a[1])})", a[0])))
    monkeypatch.setattr(torch.cuda.Event, "record", _wrap(log, "record", torch.cuda.Event.record,
                                                          lambda lg, a, k: lg.add(f"record({lg.desc(a[0])})", a[1] if len(a) > 1 else k.get("stream"))))
    monkeypatch.setattr(torch.Tensor, "record_stream", _wrap(log, "record_stream", torch.Tensor.record_stream,
                                                             lambda lg, a, k: lg.add(f"record_stream({lg.desc(a[0])}, {lg.stream(a[1])})")))
    return log


class _Reducer:
    """the two forms of a bucket callback: a plain one, and a bound method of a reducer whose `mode` is "serial" """

    def __init__(self, log, mode):
        self.log, self.mode = log, mode

    def on_bucket(self, name):
        self.log[0].add(f"bucket({name})")


def _model(spec):
    sys.path.insert(0, HERE)
    from test_gpu_model import make_model
    key = (spec["rnn"], spec["hidden"], spec["layers"])
    if key not in _MODELS:
        torch.manual_seed(11)
        _MODELS[key] = make_model(dict(rnn=spec["rnn"], hidden=spec["hidden"], layers=spec["layers"], classes=CLASSES))
    return _MODELS[key]


def run_case(spec, log, model=None, results=None):
    """two steps of the case (forward_only: two eval forwards without a saved context); returns the log lines of each.  results: a list that
    receives (logits, loss, flat gradient, BatchNorm running statistics) of each step"""
    from asr_amd import _lib, engine, ops
    from asr_amd.trainers.deepspeech_trainer import _prep_targets_host
    model = _model(spec) if model is None else model
    model.precision = spec.get("precision", "bf16")
    B, tin = spec["B"], spec["tin"]
    T = _lib.conv_dims(FREQ, tin)[2]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, 1, FREQ, tin, generator=gen).to(DEV)
    tsz = torch.full((B,), max(1, T // 10), dtype=torch.int32)
    targets = torch.randint(1, CLASSES, (int(tsz.sum()),), generator=gen, dtype=torch.int32)
    t_h, off_h, tl_h, max_u = _prep_targets_host(targets, tsz)
    lens_dev, tg, off, tl = torch.full((B,), T, dtype=torch.int32, device=DEV), t_h.to(DEV), off_h.to(DEV), tl_h.to(DEV)
    model._ensure_flat(x.device)
    old = {k: getattr(engine, k) for k in spec.get("switches", {})}
    main, side = torch.cuda.current_stream(), engine._side_stream(torch.device(DEV))
    kw = {}
    if spec.get("buckets"):
        red = _Reducer(log, spec["buckets"])
        kw["on_bucket"] = red.on_bucket if spec["buckets"] == "serial" else (lambda name: red.on_bucket(name))
        if "serial_buckets" in inspect.signature(engine.backward).parameters:
            kw["serial_buckets"] = spec["buckets"] == "serial"
    steps = []
    engine._BWD_PERSISTENT.clear()
    box = []
    th = threading.Thread(target=lambda: box.append(ops.rnn_ctx(DEV)))      # (ops creates one recurrence context per thread and device)
    th.start()
    th.join()
    bound = ops.use_rnn_ctx(box[0], DEV)
    bound.__enter__()
    try:
        for k, v in spec.get("switches", {}).items():
            setattr(engine, k, v)
        for _ in range(2):
            with torch.no_grad():
                W, Gr = model._flat.tensors(model), model._flat.tensors(model, grads=True)
                log[0] = lg = _Log(main, side)
                try:
                    if spec.get("forward_only"):
                        logits, _ = engine.forward(W, model._cfg, x, lens_dev, training=False, save=False)
                        lg.lines.append(f"after forward: rnn_last_path {ops.rnn_last_path()}")
                        nll = None
                    else:
                        logits, ctx = engine.forward(W, model._cfg, x, lens_dev, training=True, save=True)
                        lg.lines.append(f"after forward: rnn_last_path {ops.rnn_last_path()}")
                        nll, dlogits = ops.ctc_loss(logits, tg, off, lens_dev, tl, max_u, 1.0 / B, want_grad=True)
                        engine.backward(W, Gr, model._cfg, ctx, dlogits, **kw)
                        lg.lines.append(f"after backward: rnn_last_path {ops.rnn_last_path()}")
                finally:
                    log[0] = None
                torch.cuda.synchronize()
                steps.append(lg.lines)
                if results is not None:
                    stats = torch.cat([v.detach().float().reshape(-1) for n, v in sorted(model.state_dict().items()) if "running_" in n])
                    results.append((logits.detach().clone(), None if nll is None else nll.detach().clone(),
                                    model.flat_parameters()[1].detach().clone(), stats))
        ops.rnn_persistent_check()                                 # a starved launch fails the case by its own message, not as a schedule diff
    finally:
        bound.__exit__(None, None, None)
        for k, v in old.items():
            setattr(engine, k, v)
    return steps


def _golden():
    tab = json.load(open(GOLDEN))
    return {name: [[tab["lines"][i] for i in step] for step in steps] for name, steps in tab["cases"].items()}


def _record(path, name, steps):
    """the golden keeps every distinct line once and the cases as lists of line numbers (most lines recur from layer to layer and case to case)"""
    tab = json.load(open(path)) if os.path.exists(path) else {"lines": [], "cases": {}}
    index = {s: i for i, s in enumerate(tab["lines"])}
    tab["cases"][name] = [[index.setdefault(s, len(index)) for s in step] for step in steps]
    tab["lines"] = sorted(index, key=index.get)
    with open(path, "w") as f:
        f.write('{\n "lines": [\n' + ",\n".join("  " + json.dumps(s) for s in tab["lines"]) + '\n ],\n "cases": {\n'
                + ",\n".join(f"  {json.dumps(n)}: {json.dumps(v, separators=(',', ':'))}" for n, v in tab["cases"].items()) + "\n }\n}\n")


@pytest.mark.parametrize("name", list(CASES))
def test_the_engine_issues_the_recorded_schedule(name, recorder):
    spec, witnesses = CASES[name]
    got = run_case(spec, recorder)
    out = os.environ.get("DS2_ENGINE_SCHEDULE_RECORD")
    if out:
        _record(out, name, got)
        want = got
    else:
        want = _golden()[name]
    for w in witnesses:
        assert any(re.search(w, s) for step in want for s in step), f"the recorded schedule of {name!r} has no record {w!r}: its branch is not reached"
    for n, (g, w) in enumerate(zip(got, want)):
        if g != w:
            i = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            lo = max(0, i - 3)
            pytest.fail(f"{name}, step {n + 1}: record {i} of {len(g)} (recorded: {len(w)}) differs\n  issued:\n    " + "\n    ".join(g[lo:i + 3])
                        + "\n  recorded:\n    " + "\n    ".join(w[lo:i + 3]))


def test_every_case_is_in_the_golden_and_none_is_left_over():
    if not os.environ.get("DS2_ENGINE_SCHEDULE_RECORD"):
        assert sorted(json.load(open(GOLDEN))["cases"]) == sorted(CASES)
