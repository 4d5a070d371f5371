"""-m gpu: which kernel family takes which recurrence call.  One call each of ops.rnn_fwd, rnn_bwd and rnn_bwd_bn per shape on a private
recurrence context, and after each call what the host path left in it: rnn_last_path(), last_bwd_kind, cooldown — against
tests/golden/rnn_host_paths.json, recorded with this same file (DS2_RNN_PATHS_RECORD=<output file>) before the recurrence entries were
given one host path.  The host code around the kernels decides when a persistent launch is safe; this pins every one of those decisions:
H = 20 has no persistent kernel, 48 an odd slice count, 160 / 320 are 10-unit shapes, 256 / 512 / 1024 / 1280 K-split shapes, 1296 exceeds the
bf16 chunk limit, B = 16 / 17 and 33 cross the tile-height rule, B = 48 at H = 1024 the 256-CU residency rule, and group sizes on both sides
of 32 the XCD-local rule.  Written against asr_amd.ops alone.  The values computed are not looked at (the parity tests do that)."""
import ctypes as C
import json
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnn_host_paths.json")
GATES = (1, 3, 4)
HS = (16, 20, 32, 48, 160, 256, 320, 512, 1024, 1280, 1296)
BS = (1, 16, 17, 33, 48, 64)
VAR_HS, VAR_BS = (256, 320), (16, 33)            # the shapes of the variants (selectors, operand forms, armed workspace, cooldown)


def _private_ctx(ops):
    """a recurrence context of its own: ops creates one per (thread, device)"""
    box = []
    th = threading.Thread(target=lambda: box.append(ops.rnn_ctx(DEV)))
    th.start()
    th.join()
    return box[0]


class _Layer:
    """seeded inputs of one bidirectional layer (gates, H, B, T) and the three calls on them"""

    def __init__(self, ops, mode, g, H, B, T, pack):
        self.ops, self.mode, self.g, self.H, self.B, self.T, self.M = ops, mode, g, H, B, T, T * B
        gen = torch.Generator(device=DEV).manual_seed(1000 * H + 10 * B + g)
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)
        self.wpf, self.wpb = pack
        self.gx = rnd(self.M, 2 * g * H) * 0.5
        self.bhh = rnd(2, g * H) * 0.1
        self.dy, self.dyn, self.x = rnd(self.M, H), rnd(self.M, H), rnd(self.M, H) * 0.7 + 0.2
        self.gamma = torch.rand(H, device=DEV, generator=gen) + 0.5
        self.mean, self.var = self.x.mean(0), self.x.var(0, unbiased=False)
        self.lens = torch.tensor(sorted((1 + (7 * b) % T for b in range(B)), reverse=True), dtype=torch.int32, device=DEV)
        self.lens[0] = T

    def state(self, ctx):
        return [self.ops.rnn_last_path(DEV), ctx.last_bwd_kind, ctx.cooldown]

    def fwd(self, packed=False, bf16_x=False, armed=False):
        o, g, H, B, T = self.ops, self.g, self.H, self.B, self.T
        gx = self.gx.bfloat16() if bf16_x else self.gx.clone()
        hsum = torch.empty(2, (B + 15) // 16, H, device=DEV) if (bf16_x and g != 1) else None
        ws = o.rnn_ws("fwd", g, B, H, self.mode, DEV) if armed else None
        out = o.rnn_fwd(g, gx, self.wpf, self.bhh, self.lens, T, B, H, bf16=self.mode, packed_gates=packed, hsum=hsum, ws=ws)
        self.saved = (None if bf16_x else gx, out[0], out[1], out[2] if packed else None)

    def _bwd_args(self, packed, armed):
        o, g, H, B = self.ops, self.g, self.H, self.B
        gx, hbuf, aux, rec = self.saved
        kw = dict(bf16=self.mode, ws=o.rnn_ws("bwd", g, B, H, self.mode, DEV) if armed else None)
        if packed:
            kw.update(dgx_bf16=torch.empty(self.M, 2 * g * H, dtype=torch.bfloat16, device=DEV), gates_bf16=rec,
                      dhn_bf16=torch.empty(self.M, 2 * H, dtype=torch.bfloat16, device=DEV) if g == 3 else None,
                      bias_part=torch.empty(B, 2, 4, H, device=DEV))
        return (None if packed else gx.clone(), None if aux is None else aux.clone(), hbuf, self.wpb, self.lens, self.T, B, H), kw

    def bwd(self, packed=False, armed=False):
        a, kw = self._bwd_args(packed, armed)
        self.ops.rnn_bwd(self.g, self.dy, *a, **kw)

    def bwd_bn(self, packed=False, armed=False, bf16_x=False):
        a, kw = self._bwd_args(packed, armed)
        o = self.ops
        sums = o.bn1d_bwd_sums(self.dyn, self.x, self.mean, self.var, self.gamma)
        o.rnn_bwd_bn(self.g, self.dyn, self.x.bfloat16() if bf16_x else self.x, self.mean, self.var, self.gamma, sums, *a, **kw)

    def three(self, ctx, **kw):
        """fwd, bwd, bwd_bn: the context's state after each"""
        rec = []
        self.fwd(**{k: v for k, v in kw.items() if k != "bn_bf16_x"})
        rec.append(self.state(ctx))
        kw.pop("bf16_x", None)
        self.bwd(**{k: v for k, v in kw.items() if k != "bn_bf16_x"})
        rec.append(self.state(ctx))
        bn_x = kw.pop("bn_bf16_x", False)
        self.bwd_bn(bf16_x=bn_x, **kw)
        rec.append(self.state(ctx))
        return rec


def _run(mode):
    from asr_amd import ops
    got = {}
    ctx = _private_ctx(ops)
    with ops.use_rnn_ctx(ctx, DEV):
        for g in GATES:
            for H in HS:
                gen = torch.Generator(device=DEV).manual_seed(77 * H + g)
                whh = (torch.rand(2, g * H, H, device=DEV, generator=gen) * 2 - 1) / H ** 0.5
                pack = ops.rnn_pack(g, whh, bf16=mode)
                for B in BS:
                    L = _Layer(ops, mode, g, H, B, 3, pack)
                    got[f"g{g} H{H} B{B} T3"] = L.three(ctx)
                    if H not in VAR_HS or B not in VAR_BS:
                        continue
                    for sel in (64, 128, 256):
                        ops.debug_flags(sel, DEV)
                        got[f"g{g} H{H} B{B} T3 selector {sel}"] = L.three(ctx)
                        ops.debug_flags(0, DEV)
                    got[f"g{g} H{H} B{B} T3 armed ws"] = L.three(ctx, armed=True)
                    if mode == 1:                                   # the operand forms of the bf16 training mode (the only mode that has them)
                        got[f"g{g} H{H} B{B} T3 packed gates"] = L.three(ctx, packed=True)
                        got[f"g{g} H{H} B{B} T3 bf16 x-projections, hsum"] = L.three(ctx, packed=True, bf16_x=True)
                        got[f"g{g} H{H} B{B} T3 bf16 bn_x"] = L.three(ctx, packed=True, bn_bf16_x=True)
                    # where a cooldown is consumed: a context of its own that starts with two calls to go, three consecutive calls
                    for name, seq in (("fwd fwd fwd", ("fwd", "fwd", "fwd")), ("bwd_bn bwd bwd_bn", ("bwd_bn", "bwd", "bwd_bn"))):
                        cold = _private_ctx(ops)
                        with ops.use_rnn_ctx(cold, DEV):
                            L.fwd()
                            cold.cooldown = 2
                            rec = []
                            for call in seq:
                                getattr(L, call)()
                                rec.append(L.state(cold))
                            got[f"g{g} H{H} B{B} T3 cooldown 2, {name}"] = rec
                            ops.rnn_persistent_check(DEV)
            got[f"g{g} H256 B16 T1"] = _Layer(ops, mode, g, 256, 16, 1, ops.rnn_pack(g, torch.zeros(2, g * 256, 256, device=DEV), bf16=mode)).three(ctx)
        ops.rnn_persistent_check(DEV)                               # a starved launch on a shared machine fails the test honestly: no retry
    return got


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_each_call_takes_the_recorded_kernel_family(mode):
    got = _run(mode)
    out = os.environ.get("DS2_RNN_PATHS_RECORD")
    if out:
        tab = json.load(open(out)) if os.path.exists(out) else {}
        tab[f"mode {mode}"] = got
        with open(out, "w") as f:
            f.write("{\n" + ",\n".join(f' "{m}": {{\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in t.items()) + "\n }" for m, t in sorted(tab.items())) + "\n}\n")
        return
    want = json.load(open(GOLDEN))[f"mode {mode}"]
    assert list(got) == list(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} calls left another (last_path, last_bwd_kind, cooldown) than recorded, e.g. {dict(list(wrong.items())[:6])}"
