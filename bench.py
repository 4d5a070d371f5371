#!/usr/bin/env python
"""bench.py — DeepSpeech2 CTC train-step throughput (utterances/sec) on MI355X, BASELINE.json metric.

    python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run)
    python bench.py ... --dump-outputs DIR                 (+ what the last timed step computed, as DIR/<name>.npy: dump_outputs)
    python bench.py ... --full                             (+ the legs that take runs of their own, see below)

A "step" = one full train step of the hot path on one synthetic batch already resident in HBM:
forward, CTC, backward, (RCCL gradient all-reduce,) fused AdamW, loss.item() sync.
Workloads (--workload): c3 = BASELINE metric config (5x1024 BiGRU, 10 s / 161-bin, B=64 per GPU, C=29),
c2 = configs[1] (5x768 BiGRU, B=32).  Weak scaling: per-GPU batch fixed.
Prints ONE JSON line (rank 0) with `roofline` (dominant kernel, measured live with HIP events on the
launch stream).  A plain run does only that: set-up, warm-up, the timed steps, the outputs, the line.
--full (single GPU) adds the legs that run after the timed region: `other_workloads` and `dp_path_1rank`
(short runs of the other configurations and of the one-rank RCCL path), `cpu_baseline` (the CPU oracle
timed on the host cores on a bounded sample) and `loss_parity`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC: RCCL across processes needs it on this driver

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (rnn, hidden, layers, classes, per-GPU batch, input frames)
    "c3": ("gru", 1024, 5, 29, 64, 1001),
    "c2": ("gru", 768, 5, 29, 32, 1001),
    "c1": ("gru", 256, 2, 29, 4, 201),
    "c4": ("lstm", 1280, 7, 29, 32, 1501),
    "c5": ("gru", 1024, 5, 80, 64, 2001),       # ragged 3-20 s (T_b ~ U{301..2001}), length-sorted, ~80 kana classes
}
F32_NOTE = ("fp32 storage, state, accumulation, BatchNorm, CTC, optimizer, conv forward; the large input-to-hidden GEMMs, the persistent "
            "recurrences (where the shape fits) and conv2's backward take each fp32 operand as TWO bf16 terms (hi + lo) and form a product as "
            "hi.hi + hi.lo + lo.hi on the bf16 matrix cores with fp32 accumulation: 4e-6 / 1e-6 / 2e-5 of the fp64 result "
            "(DS2_F32_GEMM=f32 DS2_F32_RNN=f32 DS2_F32_CONV=f32: the fp32-input MFMA kernels)")


def dtype_label(dtype):
    """What "f32" means in THIS process: "fp32-grade (bf16x3)" when any of the three product families runs as three-term split-bf16 products
    (the default), "f32" only when DS2_F32_GEMM = DS2_F32_RNN = DS2_F32_CONV = f32 select the fp32-input MFMA kernels throughout."""
    if dtype != "f32":
        return dtype
    from asr_amd import engine as _eng
    return "f32" if (_eng.F32_GEMM, _eng.F32_RNN, _eng.F32_CONV) == ("f32", "f32", "f32") else "fp32-grade (bf16x3)"


FP32_MFMA_PEAK_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md, dense f32-input matrix rate
BF16_MFMA_PEAK_TFLOPS = 2500.0    # same guide: dense bf16 MFMA (the 5 PF marketing figure is 2:1 sparse)
# fp32 mode, split kernels: an fp32-grade product is THREE bf16 MFMA products (hi.hi + hi.lo + lo.hi), so the roof of such a kernel, in
# algorithmic (one-product) FLOPs, is a third of the bf16 matrix rate - NOT the 157 TF/s of the fp32-input MFMA it no longer uses
SPLIT_BF16_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 3.0
SPLIT_PEAK_NOTE = ("fp32-grade product formed as three bf16 MFMA products (hi.hi + hi.lo + lo.hi): peak = dense bf16 MFMA rate / 3, achieved = "
                   "algorithmic (one-product) FLOPs")
HBM_PEAK_GBS = 8000.0


def kernel_source_sha256():
    """sha256 over the sources the recurrence kernels are built from: rnn.hip, the headers it includes (rnn_bwd_ksplit.h, rnn_fwd_u10.h,
    permlane.h, common.h, ...) and the Makefile (same function as scripts/pmc_summarize.py)"""
    CSRC = os.path.join(ROOT, "asr_amd", "csrc")
    import hashlib, re
    h = hashlib.sha256()
    seen, todo = [], ["rnn.hip"]
    while todo:                                        # rnn.hip and every local header it (transitively) includes, in discovery order
        name = todo.pop(0)
        if name in seen:
            continue
        seen.append(name)
        src = open(os.path.join(CSRC, name), "rb").read()
        h.update(src)
        todo += [m for m in re.findall(r'#include "([^"/]+)"', src.decode("utf-8", "replace")) if os.path.exists(os.path.join(CSRC, m))]
    h.update(open(os.path.join(CSRC, "Makefile"), "rb").read())
    return h.hexdigest()


PMC_SUMMARY = "r06_pmc_persistent.json"


def expected_ksplit_instance(G, H):
    """the template instance of the K-split backward recurrence the library launches for a bf16 training layer (rnn_bwd_ksplit.h:
    <G, NT = H / 128, TR = GRU training instance, SP = fp32 split form>), as rocprofv3 prints it"""
    return f"rnn_bwd_ksplit_kernel<{G}, {H // 128}, {'true' if G == 3 else 'false'}, false>"


def load_pmc_summary():
    """(summary, why_not): profiles/r04_pmc_persistent.json (written by scripts/pmc_summarize.py from the rocprofv3 PMC passes) — but only if
    it was collected for THIS build of the recurrence kernels: the summary carries the sha256 of the kernel sources it was measured on, and
    a summary for other sources is refused (`roofline.traffic` is then null with the reason) instead of silently going stale."""
    path = os.path.join(ROOT, "profiles", PMC_SUMMARY)
    try:
        with open(path) as f:
            pmc = json.load(f)
    except (OSError, ValueError):
        return None, f"profiles/{PMC_SUMMARY} not present"
    try:
        now = kernel_source_sha256()
    except OSError as e:
        return None, f"kernel sources not readable ({e})"
    if pmc.get("kernel_source_sha256") != now:
        return None, (f"profiles/{PMC_SUMMARY} was collected for other kernel sources (sha256 {str(pmc.get('kernel_source_sha256'))[:12]}..., this tree "
                      f"{now[:12]}...): re-run scripts/gpu_pmc_persistent.sh")
    return pmc, None


def _pci_bus_id(index):
    """PCI bus id of a visible device, through the HIP runtime torch has already loaded."""
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        buf = ctypes.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(index)) == 0:
            return buf.value.decode()
    except OSError:
        pass
    return f"unknown:{index}"


def _rccl_version():
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    except Exception as e:                      # noqa: BLE001 - diagnostics only
        return f"unavailable ({type(e).__name__})"


def train_flops_per_utt(rnn, H, L, C, T):
    """FLOPs(train) = 2*conv1 + 3*(conv2 + rnn + fc)."""
    G = 3 if rnn == "gru" else 4
    conv1 = 2 * 32 * 81 * T * 451
    conv2 = 2 * 32 * 41 * T * 7392
    rnn_f = sum(2 * 2 * T * G * H * ((1312 if l == 0 else H) + H) for l in range(L))
    fc = 2 * T * H * C
    return 2 * conv1 + 3 * (conv2 + rnn_f + fc)


def audio_conf():
    return SimpleNamespace(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hamming", speed_volume_perturb=False,
                           spec_augment=False, noise_dir=None, noise_prob=0.4, noise_levels=(0.0, 0.5))


def label_file(tmp, n):
    import pandas as pd
    chars = ["_", "'"] + list("abcdefghijklmnopqrstuvwxyz") + ["|"] + [chr(0x3041 + i) for i in range(200)]
    path = os.path.join(tmp, "labels.csv")
    pd.DataFrame({"label": chars[:n]}).to_csv(path, index=False)
    return path


def synthetic_batch(B, tin, C, seed, ragged=False):
    """Collated batch in the reference's contract (functional.py:9-32).  ragged: T_b ~ U{301..tin}, sorted descending
    (one batch of mixed lengths: the CPU tests' shape; the bench's c4 / c5 batches come from the length-bucketing sampler)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, 161, tin, generator=g)
    if ragged:
        tb = torch.randint(301, tin + 1, (B,), generator=g).sort(descending=True).values
        tb[0] = tin
    else:
        tb = torch.full((B,), tin)
    for i in range(B):
        x[i, :, :, int(tb[i]):] = 0.0
    pct = torch.tensor([int(t) / float(tin) for t in tb], dtype=torch.float32)
    tsz = (tb // 20).to(torch.int32)
    targets = torch.randint(1, C, (int(tsz.sum()),), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.int32)
    return x, targets, pct, tsz


def synthetic_batch_from_lengths(tb, C, seed):
    """Collated batch (functional.py:9-32) for given per-utterance input frame counts: sorted descending, padded to the longest."""
    tb = torch.as_tensor(tb).sort(descending=True).values
    tin, B = int(tb[0]), int(tb.numel())
    x = torch.randn(B, 1, 161, tin, generator=torch.Generator().manual_seed(seed))
    for i in range(B):
        x[i, :, :, int(tb[i]):] = 0.0
    pct = torch.tensor([int(t) / float(tin) for t in tb], dtype=torch.float32)
    tsz = (tb // 20).to(torch.int32)
    targets = torch.randint(1, C, (int(tsz.sum()),), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.int32)
    return x, targets, pct, tsz


def _oracle_state(rnn, H, L, C):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import det
    shapes = det.state_shapes(rnn, H, L, C)
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_var") or (k.endswith("weight") and len(shp) == 1):
            sd[k] = torch.ones(shp)
        elif k.endswith("running_mean") or (k.endswith("bias") and ("batch_norm" in k or k.startswith("fc.") or ".1." in k or ".4." in k)):
            sd[k] = torch.zeros(shp)
        else:
            sd[k] = (torch.rand(shp, generator=g) * 2 - 1) * (1.0 / (H ** 0.5))
    return sd


def _host_description():
    """CPU model / sockets / library versions of the box the baseline runs on (stated next to the number)."""
    model, sockets = "unknown CPU", set()
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown CPU":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                sockets.add(line.split(":", 1)[1].strip())
    except OSError:
        pass
    cfg = torch.__config__.show()
    import re as _re
    mkl = _re.search(r"Math Kernel Library Version ([\w.\-]+(?: Product)?(?: Build \d+)?)", cfg)
    dnn = _re.search(r"(?:MKL-DNN|oneDNN) v([\w.\-]+)", cfg)
    omp = _re.search(r"OpenMP (\d+)", cfg)
    return (f"{model}, {max(len(sockets), 1)} socket(s), {os.cpu_count()} logical cores; torch {torch.__version__}, "
            f"MKL {mkl.group(1) if mkl else 'n/a'}, oneDNN {dnn.group(1) if dnn else 'n/a'}, OpenMP {omp.group(1) if omp else 'n/a'}")


def cpu_baseline_worker(rnn, H, L, C, tin, B):
    """Runs in a child process (hard wall-clock limit enforced by the parent).  SURVEY §8(d) / BASELINE.md §3: the reference's statement
    sequence (fit -> zero_grad -> backward -> AdamW.step) in the reference's own PACKED formulation (oracle/ds2_packed.py:
    pack_padded_sequence -> fused bidirectional gru/lstm -> pad_packed_sequence, blocks.py:87-89; validated against the goldens
    generated from the imported reference, tests/test_oracle_golden.py), on a bounded sample of the same workload: the same model
    and utterance length at the largest batch that fits the time budget.
    Protocol: the thread count is probed AT THE TIMED SHAPE (one full-length utterance, T_in = tin), then ONE warm-up step and TWO timed
    steps of the same batch with the optimizer state carried through; the three loss values are returned so that the parent can run the HIP
    path from the same weights on the same batch and report the matched-loss evidence (`loss_parity`).  Beside it (`fair_cpu_unpacked`):
    the same three steps with the recurrent layers un-packed — the faster, fairer CPU figure BASELINE.md §3.2 asks for."""
    from oracle import ds2_oracle as O
    from oracle import ds2_packed as P
    cores = os.cpu_count() or 1
    sd = _oracle_state(rnn, H, L, C)
    t_start = time.time()

    def fresh_step(b, t_in):
        params = P.leaf_params(sd)
        opt = P.make_optimizer(params)
        x, targets, pct, tsz = synthetic_batch(b, t_in, C, 1)
        t0 = time.time()
        P.train_step(params, opt, (x, targets, pct.clone(), tsz))
        return time.time() - t0

    torch.set_num_threads(min(cores, 16))
    fresh_step(2, 101)                                         # process warm-up (thread pool, allocator, oneDNN primitives)
    fresh_step(1, tin)                                         # ... and the full-length buffers (the first T_in = tin call costs twice a later one)
    probe = {}
    pb = min(2, B)                                             # (B = 1 is not representative: the packed path is SLOWER per step there than at B = 3)
    for n in sorted({min(cores, c) for c in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(n)
        probe[n] = fresh_step(pb, tin)                         # the timed shape's own utterance length
        if probe[n] > 1.4 * min(probe.values()) or time.time() - t_start > 60:
            break                                              # larger teams only get slower from here
    nthr = min(probe, key=probe.get)
    torch.set_num_threads(nthr)
    # largest batch (<= 4) for which warm-up + two timed steps are predicted to stay inside ~100 s
    # (the packed path is SUPER-linear in B — its per-time-step slice gradients allocate packed-sequence-sized buffers: 6 s per step at B = 3,
    #  52 s at B = 8 on the same host — so the batch is capped at 4: three steps then stay well inside the parent's limit on a slower box too)
    b_s = max(1, min(B, 4, int(pb * 100.0 / 3.0 / max(probe[nthr], 1e-9))))
    params = P.leaf_params(sd)
    opt = P.make_optimizer(params)
    x, targets, pct, tsz = synthetic_batch(b_s, tin, C, 1)
    losses, times = [], []
    for k in range(3):                                         # step 0 = warm-up at the timed shape, steps 1-2 timed
        t0 = time.time()
        losses.append(P.train_step(params, opt, (x, targets, pct.clone(), tsz)))
        times.append(time.time() - t0)
    dt = (times[1] + times[2]) / 2.0
    # the FAIR CPU figure: the same model, batch, optimizer and thread count with the recurrent layers as the fused aten
    # gru / lstm on the PADDED tensor — no pack_padded_sequence, hence no per-time-step packed slices in autograd; exactly equivalent here
    # because every utterance of the synthetic batch has the full length (oracle/ds2_packed.py forward(packed=False) asserts it; equality
    # of the two forms' loss is checked below).  1 warm-up + 2 timed steps from the SAME initial weights as the packed run.
    fair = None
    if time.time() - t_start < 170.0:
        params_u = P.leaf_params(sd)
        opt_u = P.make_optimizer(params_u)
        lu, tu = [], []
        for k in range(3):
            t0 = time.time()
            lu.append(P.train_step(params_u, opt_u, (x, targets, pct.clone(), tsz), packed=False))
            tu.append(time.time() - t0)
            if time.time() - t_start > 230.0:
                break
        if len(tu) == 3:
            fair = {"value": b_s / ((tu[1] + tu[2]) / 2.0), "unit": "utterances/sec", "cores": nthr, "batch": b_s, "losses": lu,
                    "step_seconds": [round(t, 2) for t in tu],
                    "loss_vs_packed_form": max(abs(a - b) / abs(b) for a, b in zip(lu, losses)),
                    "sample": f"same model / batch (B={b_s}, T_in={tin}) / AdamW / {nthr} threads with the recurrent layers un-packed (fused aten "
                              f"{rnn} on the padded tensor; equivalent: no utterance is padded): 1 warm-up + 2 timed steps"}
    out = {"value": b_s / dt, "unit": "utterances/sec", "cores": nthr, "kind": "port", "host_cores": cores, "host": _host_description(),
           "batch": b_s, "losses": losses, "step_seconds": [round(t, 2) for t in times],
           "sample": (f"reference statement sequence in packed form (pack_padded_sequence -> aten gru/lstm -> pad_packed_sequence, CTC, backward, "
                      f"torch AdamW) at B={b_s} of the config's {B}, same {L}x{H} {rnn} model, T_in={tin}: 1 warm-up step + 2 timed steps "
                      f"({times[1]:.1f} s, {times[2]:.1f} s; warm-up {times[0]:.1f} s), optimizer state carried through; threads probed at the timed "
                      f"shape (B={pb}, T_in={tin}) {({k: round(v, 2) for k, v in probe.items()})} s -> {nthr} of {cores}"),
           "fair_cpu_unpacked": fair if fair is not None else {"value": None, "sample": "skipped: the packed-form leg used up the time box"}}
    print("CPU_BASELINE_JSON " + json.dumps(out), flush=True)


def loss_parity(rnn, H, L, C, tin, cpu, dev):
    """Matched-loss evidence: the HIP path started from the SAME weights (`_oracle_state`) on the SAME
    batch as the CPU port's three steps just timed, same AdamW hyper-parameters: loss of every step, fp32 mode and bf16 mode, and the
    largest relative gap to the CPU port's loss over the steps."""
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW
    from asr_amd.trainers import DeepSpeechTrainer
    b_s, ref = int(cpu["batch"]), [float(v) for v in cpu["losses"]]
    x, targets, pct, tsz = synthetic_batch(b_s, tin, C, 1)
    sd = _oracle_state(rnn, H, L, C)
    out = {"batch": b_s, "steps": len(ref), "cpu": ref,
           "what": f"{len(ref)} train steps from identical weights on the identical batch (B={b_s}, T_in={tin}), AdamW lr 1.5e-4: CPU port of the "
                   "reference statement sequence vs this library"}
    for mode in ("fp32", "bf16"):
        with tempfile.TemporaryDirectory() as tmp:
            m = DeepSpeech(audio_conf=audio_conf(), decoder=None, label_path=label_file(tmp, C), rnn_type=rnn, rnn_hidden_size=H,
                           rnn_hidden_layers=L, bidirectional=True)
        m.load_state_dict(sd)
        m.to(dev).train()
        m.precision = mode
        opt = FusedAdamW(m, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
        tr = DeepSpeechTrainer(m, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)
        xs = x.to(dev)
        got = [float(tr.step((xs, targets, pct.clone(), tsz))[1]) for _ in ref]
        tr.synchronize() if hasattr(tr, "synchronize") else torch.cuda.synchronize()
        out["gpu_" + mode] = got
        out["rel_" + mode] = max(abs(g - c) / abs(c) for g, c in zip(got, ref))
        del tr, opt, m
    out["rel"] = out["rel_fp32"]
    return out


def cpu_baseline(rnn, H, L, C, tin, B, limit_s=300):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", rnn, str(H), str(L), str(C), str(tin), str(B)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        for line in r.stdout.splitlines():
            if line.startswith("CPU_BASELINE_JSON "):
                return json.loads(line[len("CPU_BASELINE_JSON "):])
        return {"value": None, "unit": "utterances/sec", "cores": 0, "kind": "port", "sample": "worker failed: " + r.stderr[-300:]}
    except subprocess.TimeoutExpired:
        return {"value": None, "unit": "utterances/sec", "cores": 0, "kind": "port", "sample": f"worker exceeded {limit_s}s"}


DUMP_MAX_ELEMS = 1 << 16          # --dump-outputs: a larger tensor is written as a fixed, seeded sample of this many elements
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, model, loss_value):
    """--dump-outputs DIR: what the last timed train step left to a caller of DeepSpeechTrainer.step, one DIR/<name>.npy per array:
    loss.npy (float64, the step's loss value), param.<name>.npy (the updated weights), grad.<name>.npy (the step's gradient buffer that the
    fused AdamW read: with N ranks the all-reduced sum) and buffer.<name>.npy (the BatchNorm running statistics), float32.  A tensor of more than DUMP_MAX_ELEMS
    elements is written flat as the elements at DUMP_MAX_ELEMS sorted positions drawn by a generator seeded with the crc32 of its name:
    the same positions in every run and every build, so that two builds can be compared array by array."""
    import zlib
    import numpy as np

    def sample(name, t):
        t = t.detach()
        if t.numel() <= DUMP_MAX_ELEMS:
            return t.float().cpu().numpy()
        idx = np.random.default_rng(zlib.crc32(name.encode())).choice(t.numel(), DUMP_MAX_ELEMS, replace=False)
        return t.reshape(-1)[torch.from_numpy(np.sort(idx)).to(t.device)].float().cpu().numpy()

    grads = model._flat.tensors(model, grads=True)
    arrays = {"loss": np.array([loss_value], dtype=np.float64)}
    for n, p in model.named_parameters():
        arrays["param." + n] = sample(n, p)
        arrays["grad." + n] = sample(n, grads[n])
    for n, b in model.named_buffers():
        if b.is_floating_point():
            arrays["buffer." + n] = sample(n, b)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, f"--dump-outputs: {total} bytes exceed {DUMP_MAX_BYTES}"
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def _make_trainer(workload, dtype, dev, world=1, rank=0):
    """(trainer, batches resident in HBM, (rnn, H, L, C, B, tin)) for a named workload, built exactly as main() builds the timed one."""
    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW
    from asr_amd.trainers import DeepSpeechTrainer
    rnn, H, L, C, B, tin = WORKLOADS[workload]
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = DeepSpeech(audio_conf=audio_conf(), decoder=None, label_path=label_file(tmp, C), rnn_type=rnn, rnn_hidden_size=H,
                           rnn_hidden_layers=L, bidirectional=True)
    model.to(dev).train()
    model.precision = "bf16" if dtype == "bf16" else "fp32"
    opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)
    if workload in ("c4", "c5"):
        from asr_amd.data import DistributedLengthBucketingSampler
        lo = 1201 if workload == "c4" else 301
        n_items = 8 * world * B
        frames = torch.randint(lo, tin + 1, (n_items,), generator=torch.Generator().manual_seed(1))
        frames[0] = tin
        smp = DistributedLengthBucketingSampler(list(range(n_items)), B, world, rank, durations=frames.tolist(), partial="fill")
        smp.shuffle(0)
        batches = [synthetic_batch_from_lengths(frames[torch.tensor(ids)], C, 10 + 97 * k + rank) for k, ids in enumerate(smp)]
    else:
        batches = [synthetic_batch(B, tin, C, 1 + rank)]
    return tr, [(bx.to(dev), bt, bp, bs) for bx, bt, bp, bs in batches], (rnn, H, L, C, B, tin)


def quick_workload(workload, dtype, dev, steps, warmup):
    """One of the OTHER BASELINE configurations, timed the same way as the headline one (full fused train steps on batches resident in HBM,
    synchronise / K steps / synchronise) but short: the driver-written record then carries every single-GPU config, not only the metric's.
    Returns ms per step, utterances / s, the step's fraction of the fp32 (or bf16) matrix roof and the live-timed recurrence kernels."""
    from asr_amd import ops
    from asr_amd.trainers import DeepSpeechTrainer
    tr, batches, (rnn, H, L, C, B, tin) = _make_trainer(workload, dtype, dev)
    starved0 = DeepSpeechTrainer.starved_steps
    n = [0]

    def one():
        bx, bt, bp, bs = batches[n[0] % len(batches)]
        n[0] += 1
        return tr.step((bx, bt, bp.clone(), bs))
    for _ in range(max(warmup, len(batches) if len(batches) > 1 else 0)):
        one()
    calls = {"fwd": [], "bwd": []}
    orig = (ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn)

    def ev(fn, key, t_arg, bit):
        def w(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            lp = ops.rnn_last_path()
            calls[key].append((e0, e1, int(a[t_arg]), bool(lp & bit), bool(lp & 4), bool(lp & (32 if key == "fwd" else 64)), bool(lp & 256)))
            return r
        return w
    ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn = ev(orig[0], "fwd", 5, 1), ev(orig[1], "bwd", 7, 2), ev(orig[2], "bwd", 12, 2)
    first = n[0]
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            valid, lv = one()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn = orig
    tr.synchronize()
    ms = dt / steps * 1e3
    used = [batches[k % len(batches)] for k in range(first, first + steps)]
    flops = sum(sum(train_flops_per_utt(rnn, H, L, C, (int(round(float(p) * int(b[0].size(3)))) + 1) // 2) for p in b[2]) for b in used) / len(used)
    peak = BF16_MFMA_PEAK_TFLOPS if dtype == "bf16" else FP32_MFMA_PEAK_TFLOPS
    G = 3 if rnn == "gru" else 4
    kern = {}
    for key in ("fwd", "bwd"):
        c = calls[key]
        us = sum(q[0].elapsed_time(q[1]) for q in c) * 1e3
        tsteps = sum(q[2] for q in c)
        pers, ks, sp = all(q[3] for q in c), all(q[4] for q in c), dtype != "bf16" and all(q[5] for q in c)
        u10 = key == "fwd" and pers and all(q[6] for q in c)
        kern[key] = {"kernel": "rnn_bwd_ksplit_kernel" if (key == "bwd" and pers and ks) else ("rnn_fwd_u10_kernel" if u10 else
                               f"rnn_{key}_{'persistent' if pers else 'step'}_kernel"),
                     "us_per_time_step": us / tsteps, "achieved_tflops": 2.0 * 2 * B * H * G * H * tsteps / (us * 1e-6) / 1e12,
                     "ms_per_step": us / 1e3 / steps, "peak": SPLIT_BF16_PEAK_TFLOPS if sp else peak, "split": sp}
        kern[key]["frac"] = kern[key]["achieved_tflops"] / kern[key]["peak"]
    dom = max(kern.values(), key=lambda k: k["ms_per_step"])
    from asr_amd import engine as _eng
    step_peak = SPLIT_BF16_PEAK_TFLOPS if (dtype != "bf16" and _eng.F32_GEMM == "split") else peak      # the GEMMs' roof in this mode
    out = {"workload": f"{workload}: DS2 {L}x{H} bi-{rnn.upper()} {dtype}, T_in {tin}, batch {B}" + (", length-bucketed bins" if len(batches) > 1 else ""),
           "dtype": dtype_label(dtype), **({"dtype_note": F32_NOTE} if dtype_label(dtype).startswith("fp32-grade") else {}),
           "steps": steps, "ms_per_step": ms, "utterances_per_sec": B * steps / dt, "loss": lv, "valid_last_step": bool(valid),
           "step_tflops": flops / (ms * 1e-3) / 1e12, "step_frac_of_matrix_peak": flops / (ms * 1e-3) / 1e12 / step_peak, "matrix_peak_tflops": step_peak,
           **({"matrix_peak_note": SPLIT_PEAK_NOTE, "step_vs_fp32_mfma_peak": flops / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS} if step_peak != peak else {}),
           "roofline": {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["achieved_tflops"], "peak": dom["peak"], "unit": "TFLOP/s",
                        "frac": dom["frac"], **({"peak_note": SPLIT_PEAK_NOTE} if dom["split"] else {}),
                        "us_per_time_step": dom["us_per_time_step"], "ms_per_step_in_this_kernel": dom["ms_per_step"]},
           "persistent_starved_steps": DeepSpeechTrainer.starved_steps - starved0}
    del tr, batches
    torch.cuda.empty_cache()
    return out


def quick_workload_true_f32(workload, steps, limit_s=120):
    """quick_workload(workload, "f32") in a child process with DS2_F32_GEMM / _RNN / _CONV = f32: the fp32-INPUT MFMA kernels for every product
    (the reference's own arithmetic, `v_mfma_f32_32x32x2_f32` / `16x16x4_f32`) instead of the default three-term split-bf16 products — the
    selectors are read once per process, hence the child."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--quick-worker", workload, "f32", str(steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s,
                           env=dict(os.environ, DS2_F32_GEMM="f32", DS2_F32_RNN="f32", DS2_F32_CONV="f32", HSA_ENABLE_IPC_MODE_LEGACY="0"))
        for line in r.stdout.splitlines():
            if line.startswith("QUICK_JSON "):
                return json.loads(line[len("QUICK_JSON "):])
        return {"error": "worker failed: " + (r.stderr or r.stdout)[-300:]}
    except subprocess.TimeoutExpired:
        return {"error": f"worker exceeded {limit_s}s"}


def dp_path_one_rank(limit_s=120):
    """dp_path_one_rank_worker in a child process: RCCL prints its banner through C stdio when the process exits, i.e. BEHIND this process's
    JSON line if it ran here — and the line must stay the last thing on stdout."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--dp-one-rank-worker"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        for line in r.stdout.splitlines():
            if line.startswith("DP1_JSON "):
                return json.loads(line[len("DP1_JSON "):])
        return {"error": "worker failed: " + (r.stderr or r.stdout)[-300:]}
    except subprocess.TimeoutExpired:
        return {"error": f"worker exceeded {limit_s}s"}


def dp_path_one_rank_worker(dev, steps=5, warmup=3):
    """The data-parallel code path of the metric configuration with ONE rank: an RCCL process group of size 1, the
    bucketed reducer forced on (DS2_FORCE_ALLREDUCE=1, schedule "conv": one big all-reduce on the communication stream beside the conv-stack
    backward, the MIN-reduced validity flag) — what that path costs by itself, before there are peers to wait for."""
    import socket
    if dist.is_initialized():
        return {"error": "a process group already exists"}
    import random
    old = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT", "DS2_FORCE_ALLREDUCE", "DS2_DP_MODE")}
    os.environ.update(MASTER_ADDR="127.0.0.1", DS2_FORCE_ALLREDUCE="1", DS2_DP_MODE="conv")
    try:
        for attempt in range(4):                             # (a probed port can be taken before the store binds it: retry on another one)
            port = random.randint(20000, 31999)
            with socket.socket() as sk:
                try:
                    sk.bind(("127.0.0.1", port))
                except OSError:
                    continue
            os.environ["MASTER_PORT"] = str(port)
            try:
                dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                break
            except Exception as e:
                if attempt == 3 or not ("EADDRINUSE" in str(e) or "address already in use" in str(e).lower()):
                    raise
        tr, batches, (rnn, H, L, C, B, tin) = _make_trainer("c3", "bf16", dev)
        bx, bt, bp, bs = batches[0]
        for _ in range(warmup):
            tr.step((bx, bt, bp.clone(), bs))
        red = tr._get_reducer()
        red.timing = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step((bx, bt, bp.clone(), bs))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tr.synchronize()
        out = {"ms_per_step": dt / steps * 1e3, "schedule": red.mode, "backend": dist.get_backend(), "world_size": dist.get_world_size(),
               **red.timing_summary()}
        del tr, batches
        torch.cuda.empty_cache()
        return out
    except Exception as e:                                   # a box without a usable RCCL must not cost the headline line
        return {"error": f"{type(e).__name__}: {e}"[:300]}
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v



def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line as N ranks (one per GPU, RCCL) under
    torch.distributed.run and pass rank 0's JSON line through.  Fails loudly when the node has fewer than N GPUs — it never
    prints a 1-GPU number labelled as N."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < n and "--ranks-on-one-gpu" not in sys.argv:
        sys.exit(f"bench.py: --gpus {n} requested but this node exposes {have} GPU(s); refusing to run (a scaling point must use {n} devices)")
    import random
    rc = 1
    for attempt in range(4):
        # a port that binds NOW, taken from below the ephemeral range (a probe of port 0 hands out a port the kernel may give to any outgoing
        # connection before the launcher's store binds it: seen once as EADDRINUSE); if the launcher still loses the race, try another port
        port = None
        for _ in range(64):
            cand = random.randint(20000, 31999)
            with socket.socket() as sk:
                try:
                    sk.bind(("127.0.0.1", cand))
                    port = cand
                    break
                except OSError:
                    continue
        if port is None:
            sys.exit("bench.py: no free rendezvous port found on 127.0.0.1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        r = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stderr=subprocess.PIPE, text=True)
        rc = r.returncode
        in_use = rc != 0 and ("EADDRINUSE" in r.stderr or "address already in use" in r.stderr.lower())
        if not in_use or attempt == 3:
            sys.stderr.write(r.stderr)
            break
        sys.stderr.write(f"bench.py: rendezvous port {port} was taken between probe and bind, retrying with another one\n")
    return sys.exit(rc)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--quick-worker":      # `bench.py --quick-worker c2 f32 6`: quick_workload in a child (its own DS2_F32_* env)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        print("QUICK_JSON " + json.dumps(quick_workload(sys.argv[2], sys.argv[3], dev, int(sys.argv[4]), 2)), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--dp-one-rank-worker":
        torch.cuda.set_device(0)
        print("DP1_JSON " + json.dumps(dp_path_one_rank_worker(torch.device("cuda", 0))), flush=True)
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-worker":
        rnn, H, L, C, tin, B = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
        return cpu_baseline_worker(rnn, H, L, C, tin, B)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=None,
                    help="untimed steps (default 3; c4 / c5: one per length bin, so that every batch shape has been seen - the caching "
                         "allocator grows with a device synchronisation the first time a shape appears)")
    ap.add_argument("--workload", default="c3", choices=list(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override per-GPU batch")
    ap.add_argument("--dtype", default="", choices=["", "f32", "bf16"], help="default: the config dtype (bf16 for c3 and c5, f32 otherwise)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the legs that take runs of their own (single GPU): the other BASELINE "
                         "configurations, the 1-rank data-parallel path, the CPU baseline and the matched-loss runs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the matched-loss runs")
    ap.add_argument("--breakdown", action="store_true", help="print a per-section time breakdown to stderr")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="with --full: skip the short runs of the other single-GPU BASELINE configurations (c2 f32, c4 f32) and of the 1-rank "
                         "data-parallel path")
    ap.add_argument("--ranks-on-one-gpu", action="store_true",
                    help="TEST MODE for the N > 1 code path on a 1-GPU box: every rank uses cuda:0 and the process group is gloo (RCCL cannot put "
                         "two ranks on one device) unless DS2_DIST_BACKEND says otherwise.  The line is labelled; it is not a scaling point.")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (loss, updated weights, gradients, BatchNorm running "
                         "statistics; large tensors as a fixed, seeded sample) as DIR/<name>.npy, rank 0 only")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup is not None and args.warmup < 0:
        ap.error("--warmup must not be negative")

    if args.gpus > 1 and "RANK" not in os.environ:
        return spawn_ranks(args.gpus)                   # `python bench.py --gpus N`: one rank per GPU under torch.distributed.run
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1):
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; they must agree")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.ranks_on_one_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = args.gpus > 1 or world > 1 or "RANK" in os.environ     # launched by torch.distributed.run
    backend = os.environ.get("DS2_DIST_BACKEND", "gloo" if args.ranks_on_one_gpu else "nccl")      # "nccl" IS RCCL on ROCm
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # an N-GPU line comes from N ranks: a process group of any other size never reaches the timed region
        assert dist.get_world_size() == max(args.gpus, 1), f"--gpus {args.gpus} but the process group has {dist.get_world_size()} rank(s)"

    from asr_amd import CTCLoss, DeepSpeech, FusedAdamW, ops
    from asr_amd.trainers import DeepSpeechTrainer

    rnn, H, L, C, B, tin = WORKLOADS[args.workload]
    if args.batch:
        B = args.batch
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        model = DeepSpeech(audio_conf=audio_conf(), decoder=None, label_path=label_file(tmp, C), rnn_type=rnn, rnn_hidden_size=H,
                           rnn_hidden_layers=L, bidirectional=True)
    model.to(dev).train()
    dtype = args.dtype or ("bf16" if args.workload in ("c3", "c5") else "f32")
    model.precision = "bf16" if dtype == "bf16" else "fp32"
    opt = FusedAdamW(model, lr=1.5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    tr = DeepSpeechTrainer(model, CTCLoss(reduction="sum"), 1, None, opt, None, None, dev, dev, False, None)
    # batches resident in HBM before the timed region.  c1-c3: one fixed-length batch.  c4 / c5 (BASELINE configs[3] "bucketed sampler",
    # configs[4] "length-sorted batching"): a synthetic manifest of 8 rounds x world x B utterance lengths goes through the product's
    # DistributedLengthBucketingSampler (asr_amd/data) and the steps cycle through THIS rank's bins in the sampler's shuffled order —
    # every batch is homogeneous in length and concurrent ranks hold neighbouring lengths.
    sampler_note = None
    if args.workload in ("c4", "c5"):
        from asr_amd.data import DistributedLengthBucketingSampler
        lo = 1201 if args.workload == "c4" else 301
        n_items = 8 * world * B
        frames = torch.randint(lo, tin + 1, (n_items,), generator=torch.Generator().manual_seed(1))
        frames[0] = tin
        smp = DistributedLengthBucketingSampler(list(range(n_items)), B, world, rank, durations=frames.tolist(), partial="fill")
        smp.shuffle(0)
        batches = [synthetic_batch_from_lengths(frames[torch.tensor(ids)], C, 10 + 97 * k + rank) for k, ids in enumerate(smp)]
        sampler_note = (f"DistributedLengthBucketingSampler over {n_items} synthetic lengths U{{{lo}..{tin}}} frames, {len(batches)} bins per rank cycled; "
                        f"T_in per bin {[int(b[0].size(3)) for b in batches]}")
    else:
        batches = [synthetic_batch(B, tin, C, 1 + rank)]
    batches = [(bx.to(dev), bt, bp, bs) for bx, bt, bp, bs in batches]
    x, targets, pct, tsz = max(batches, key=lambda b: b[0].size(3))          # the longest batch: the roofline probe's layer shape
    tin_probe = int(x.size(3))
    if args.warmup is None:
        args.warmup = max(3, len(batches) if len(batches) > 1 else 0)
    step_no = [0]
    starved_before = DeepSpeechTrainer.starved_steps

    def one_step():
        bx, bt, bp, bs = batches[step_no[0] % len(batches)]
        step_no[0] += 1
        return tr.step((bx, bt, bp.clone(), bs))

    for _ in range(args.warmup):
        valid, lv = one_step()
    # The dominant kernels (the two recurrences) are timed live INSIDE the timed region: a HIP event pair on the launch stream around every
    # ops.rnn_fwd / ops.rnn_bwd call of the K steps (recording an event does not synchronise anything), read back after the final sync.
    rnn_calls = {"fwd": [], "bwd": []}
    orig_rnn = (ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn)

    def with_events(fn, key, t_arg, bit):
        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            rnn_calls[key].append((e0, e1, int(a[t_arg]), bool(ops.rnn_last_path() & bit), bool(ops.rnn_last_path() & 4), bool(ops.rnn_last_path() & 16), bool(ops.rnn_last_path() & (32 if key == "fwd" else 64)),
                                   bool(ops.rnn_last_path() & 256)))
            return r
        return wrapped

    ops.rnn_fwd, ops.rnn_bwd = with_events(orig_rnn[0], "fwd", 5, 1), with_events(orig_rnn[1], "bwd", 7, 2)
    ops.rnn_bwd_bn = with_events(orig_rnn[2], "bwd", 12, 2)      # the same recurrence with the BatchNorm1d backward of the layer above applied inside
    red = tr._get_reducer() if use_dist else None
    if red is not None:
        red.timing = []                               # event records of every collective of the timed steps (asr_amd/parallel.py)
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        valid, lv = one_step()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ops.rnn_fwd, ops.rnn_bwd, ops.rnn_bwd_bn = orig_rnn
    tr.synchronize()                                  # settle the last step's device-side verdict (starved-step counter)
    dist_info = None
    if use_dist:
        # every rank's own wall clock of the K steps (between the same two barriers), then the MAX is what the line reports
        mine = torch.tensor([dt], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank = [float(t.item()) / args.steps * 1e3 for t in every]
        tt = mine.clone()
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        assert abs(dt / args.steps * 1e3 - max(per_rank)) < 1e-6
        # which device every rank really ran on (index + PCI bus id: what tells N ranks on one GPU from N GPUs) and what starved launches cost it
        where = [None] * world
        dist.all_gather_object(where, {"rank": rank, "device_index": dev.index, "pci_bus_id": _pci_bus_id(dev.index),
                                       "name": torch.cuda.get_device_properties(dev).name,
                                       "starved_steps": DeepSpeechTrainer.starved_steps - starved_before})
        dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "schedule": red.mode,
                     "rccl_version": _rccl_version(), "device_count": torch.cuda.device_count(),
                     "ranks": [{k: w[k] for k in ("rank", "device_index", "pci_bus_id", "name")} for w in where],
                     "distinct_devices": len({w["pci_bus_id"] for w in where}),
                     "persistent_starved_steps_all_ranks": int(sum(w["starved_steps"] for w in where)),
                     "rank_ms_per_step": {"min": min(per_rank), "max": max(per_rank)}, **red.timing_summary()}
        if args.ranks_on_one_gpu:
            dist_info["ranks_on_one_gpu"] = "TEST MODE: all ranks share cuda:0 - exercises the N > 1 code path, NOT a scaling measurement"
        red.timing = None
    ms = dt / args.steps * 1e3
    utts = world * B * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, lv)

    # ---- roofline of the dominant kernels (the two recurrences): timed live with HIP events on torch's current stream, which is the
    # stream libds2hip launches on - inside the timed region (event pairs recorded above); a stand-alone probe only as a fallback.
    G = 3 if rnn == "gru" else 4
    T = (tin_probe + 1) // 2
    M = T * B
    bf = dtype == "bf16"
    pack = bf and B % 8 == 0                              # the train step's own mode (engine.forward)
    # the train step's own mode (engine.py): the persistent kernels also write the bf16 copies of h / d(hn) and the bias-gradient partial
    # sums that the TN-form weight-gradient GEMMs consume
    from asr_amd import engine as _engine
    tn = pack and _engine.WGRAD_TN and _engine.OVERLAP_MODE == "2" and T > 1
    timed_in_region = bool(rnn_calls["fwd"]) and bool(rnn_calls["bwd"])
    bn_fused = False
    if timed_in_region:
        # averages over the calls of the timed region (per layer call); T = the mean number of time steps per call (c4 / c5 vary)
        def avg(key):
            calls = rnn_calls[key]
            us = sum(c[0].elapsed_time(c[1]) for c in calls) * 1e3
            return us / len(calls), sum(c[2] for c in calls) / len(calls), all(c[3] for c in calls), all(c[4] for c in calls)
        layer_us, T_f, p_f, _ = avg("fwd")
        bwd_layer_us, T_b, p_b, ks_b = avg("bwd")
        assert T_f == T_b
        T = T_f
        path_bits = (1 if p_f else 0) | (2 if p_b else 0) | (4 if (p_b and ks_b) else 0)
        bn_fused = all(c[5] for c in rnn_calls["bwd"])       # BatchNorm1d backward applied inside the K-split kernel (ds2_rnn_bwd_bn)
        path_bits |= (32 if all(c[6] for c in rnn_calls["fwd"]) else 0) | (64 if all(c[6] for c in rnn_calls["bwd"]) else 0)   # fp32 mode: split kernels
        path_bits |= 256 if all(c[7] for c in rnn_calls["fwd"]) else 0                                                         # ... the 10-unit-slice one
    else:
        # fallback (no recurrence call was seen in the timed region): one layer's recurrences stand-alone, same shape and mode
        gx = torch.randn(M, 2 * G * H, device=dev) * 0.5
        whh = (torch.rand(2, G * H, H, device=dev) * 2 - 1) / H ** 0.5
        bhh = torch.zeros(2, G * H, device=dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        wpf, wpb_probe = ops.rnn_pack(G, whh, bf16=bf)
        ops.rnn_fwd(G, gx.clone(), wpf, bhh, lens, T, B, H, bf16=bf, packed_gates=pack)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        gx2 = gx.clone()
        dyp = torch.randn(M, H, device=dev)
        side = torch.empty(M, 2 * G * H, dtype=torch.bfloat16, device=dev) if pack else None
        h_bf = torch.empty(M, 2 * H, dtype=torch.bfloat16, device=dev) if tn else None
        dhn_bf = torch.empty(M, 2 * H, dtype=torch.bfloat16, device=dev) if (tn and G == 3) else None
        bias_part = torch.empty(B, 2, 4, H, device=dev) if tn else None
        torch.cuda.synchronize()
        e0.record()
        fwd_out = ops.rnn_fwd(G, gx2, wpf, bhh, lens, T, B, H, bf16=bf, packed_gates=pack, **({"h_bf16": h_bf} if pack else {}))
        e1.record()
        if pack:
            ops.rnn_bwd(G, dyp, None, fwd_out[1], fwd_out[0], wpb_probe, lens, T, B, H, bf16=True, dgx_bf16=side, gates_bf16=fwd_out[2],
                        dhn_bf16=dhn_bf, bias_part=bias_part)
        else:
            ops.rnn_bwd(G, dyp, gx2, fwd_out[1], fwd_out[0], wpb_probe, lens, T, B, H, bf16=bf)
        e2.record()
        torch.cuda.synchronize()
        bwd_layer_us = e1.elapsed_time(e2) * 1e3
        layer_us = e0.elapsed_time(e1) * 1e3             # one layer's whole forward recurrence (T time steps, both directions)
        path_bits = ops.rnn_last_path()
    # bf16 mode runs the recurrence as ONE persistent launch per layer (rnn_fwd_persistent_kernel) when every workgroup can be resident at
    # once (grid <= CU count) — what ds2_rnn_fwd decides; otherwise (and in fp32) it is one rnn_fwd_step_kernel launch per time step.
    persistent = bool(path_bits & 1)                     # what ds2_rnn_fwd actually did (ds2_rnn_last_path)
    launches = 1 if persistent else T
    us_per_launch = layer_us / launches
    flops_per_launch = 2.0 * 2 * B * H * G * H * (T if persistent else 1)      # both directions; all T steps in the persistent launch
    achieved = flops_per_launch / (us_per_launch * 1e-6) / 1e12
    peak = BF16_MFMA_PEAK_TFLOPS if bf else FP32_MFMA_PEAK_TFLOPS
    # HBM-side bytes per launch from the committed rocprofv3 PMC summary (separate FETCH_SIZE / WRITE_SIZE passes, FETCH x2 gfx950
    # correction: scripts/gpu_pmc_persistent.sh -> profiles/r04_pmc_persistent.json), collected for exactly this layer shape and mode
    # (GRU H=1024 B=64, bf16 operands, packed gate records); null for any other shape or when the file is absent.
    pmc, pmc_why_not = load_pmc_summary()
    same_shape = args.workload in ("c3", "c5") and bf and B == 64 and G == 3 and H == 1024
    if pmc is not None and not same_shape:
        pmc_why_not = "the PMC summary was collected for the c3 layer shape (GRU H=1024 B=64 bf16)"
    # the template instance the library launches for this shape (rnn.hip / rnn_bwd_ksplit.h): a summary for another instance is refused too
    expect = {"rnn_bwd_ksplit_kernel": expected_ksplit_instance(G, H)}

    def pmc_traffic(kernel, steps):
        nonlocal pmc_why_not
        k = (pmc or {}).get("kernels", {}).get(kernel)
        if not (same_shape and k):
            return None
        if kernel in expect and k.get("kernel") != expect[kernel]:
            pmc_why_not = f"the PMC summary holds {k.get('kernel')}, this run launched {expect[kernel]}"
            return None
        return k["hbm_bytes_per_time_step"] * steps if ("persistent" in kernel or "ksplit" in kernel) else k["hbm_bytes_per_launch"]
    traffic = pmc_traffic("rnn_fwd_persistent_kernel" if persistent else "rnn_fwd_step_kernel", T)
    # x-projections 3 x 4 + gate record 8 + h 4 + packed h 2 (+ the bf16 copy of h 2) bytes per hidden unit and direction (packed mode)
    alg_bytes_step = (3 * 4 + 8 + 4 + 2 + (2 if tn else 0) if pack else 8 * 4 + (2 if bf else 4)) * B * 2 * H
    split_f, split_b = (not bf) and bool(path_bits & 32), (not bf) and bool(path_bits & 64)
    peak_f, peak_b = (SPLIT_BF16_PEAK_TFLOPS if split_f else peak), (SPLIT_BF16_PEAK_TFLOPS if split_b else peak)
    roofline = {"kernel": ("rnn_fwd_u10_kernel" if (path_bits & 256) else "rnn_fwd_persistent_kernel") if persistent else "rnn_fwd_step_kernel",
                "bound": "mfma", "achieved": achieved,
                "peak": peak_f, "unit": "TFLOP/s", "frac": achieved / peak_f, "traffic": traffic,
                **({"peak_note": SPLIT_PEAK_NOTE} if split_f else {}),
                "algorithmic_hbm_bytes_per_launch": alg_bytes_step * (T if persistent else 1),
                "us_per_launch": us_per_launch, "us_per_time_step": layer_us / T, "launches_per_step": (1 if persistent else T) * L}
    # the backward recurrence (same FLOPs per time step): on a single GPU it is persistent too wherever its W_hh^T slice fits the
    # registers.  Whichever of the two kernels takes longer per train step is THE dominant kernel and goes first.
    bwd_persistent = bool(path_bits & 2)
    bl = 1 if bwd_persistent else T
    bl_steps = T if bwd_persistent else 1
    b_ach = flops_per_launch / (T if persistent else 1) * (T if bwd_persistent else 1) / (bwd_layer_us / bl * 1e-6) / 1e12
    # which backward kernel: the K-split persistent kernel (bf16 partial sums of dh exchanged; csrc/rnn_bwd_ksplit.h) where the shape
    # qualifies, else the all-gather persistent kernel, else one launch per time step
    ksplit = bwd_persistent and bool(path_bits & 4)
    bwd_name = "rnn_bwd_ksplit_kernel" if ksplit else ("rnn_bwd_persistent_kernel" if bwd_persistent else "rnn_bwd_step_kernel")
    bwd_traffic = pmc_traffic(bwd_name, T)
    # gate record 8 + previous state 4 + dGx G x 2 bytes per hidden unit and direction, dy 4 bytes per unit (packed mode; + 4 for the BatchNorm
    # input when the BatchNorm1d backward of the layer above is applied inside the kernel); d(hn) (GRU): 4 bytes
    # fp32, + 2 for the bf16 copy in the TN-form mode — the K-split kernel writes ONLY the bf16 copy then
    dhn_bytes = 0 if G != 3 else ((2 if ksplit else 6) if tn else 4)
    roofline_bwd = {"kernel": bwd_name, "bound": "mfma", "achieved": b_ach,
                    "peak": peak_b, "unit": "TFLOP/s", "frac": b_ach / peak_b, "traffic": bwd_traffic,
                    **({"peak_note": SPLIT_PEAK_NOTE} if split_b else {}),
                    "algorithmic_hbm_bytes_per_launch": ((8 + 4 + 2 * G + dhn_bytes) * 2 + 4 + (4 if (ksplit and bn_fused) else 0) if pack
                                                         else (4 * G + 4 + 4 + 4 * G + 4) * 2 + 4) * B * H * bl_steps,
                    **({"traffic_note": "the L2 of this part writes every stored byte through to the fabric (MI355X_MICROARCH.md, store table): "
                                        "of the counted bytes, 8 groups x 1 MB per time step are the partial-dh exchange itself (published once, read once "
                                        "from L2), not re-reads of operands"} if ksplit else {}),
                    **({"fused": "BatchNorm1d backward (elementwise half) of the layer above"} if (ksplit and bn_fused) else {}),
                    "us_per_launch": bwd_layer_us / bl,
                    "us_per_time_step": bwd_layer_us / T, "launches_per_step": bl * L}
    # The recurrences are serial chains of T dependent steps: beside the MFMA fraction each carries the LATENCY FLOOR of a time step — the
    # phases in which its waves wait (exchange publish -> visible -> gathered, the workgroup barrier, the loop-top drain), measured on the
    # product's own kernels built with phase stamps (scripts/probe_persist_timeline.hip -> profiles/r06_persist_phases.json) — and, where the
    # PMC summary applies, counted HBM traffic over algorithmic bytes (> 1: the exchange's write-through, not operand re-reads: traffic_note)
    try:
        with open(os.path.join(ROOT, "profiles", "r06_persist_phases.json")) as f:
            phases = json.load(f)
    except (OSError, ValueError):
        phases = None
    for rl, key, pers_ in ((roofline, "fwd", persistent and not (path_bits & 256)), (roofline_bwd, "bwd", ksplit)):
        if phases and same_shape and pers_ and key in phases.get("kernels", {}):
            k_ = phases["kernels"][key]
            rl["latency_floor_us_per_time_step"] = k_["latency_floor_us"]
            rl["latency_floor_frac_of_time_step"] = k_["latency_floor_us"] / k_["us_per_time_step_traced_build"]
            rl["phases_us_per_time_step"] = k_["phases_us"]
            rl["phases_source"] = phases["source"] + " (phase-stamped build of the same kernel sources: " + str(k_["us_per_time_step_traced_build"]) + " us per time step)"
        if rl.get("traffic"):
            rl["wasted_traffic_ratio"] = rl["traffic"] / rl["algorithmic_hbm_bytes_per_launch"]
    if bwd_layer_us > layer_us:
        roofline, roofline_bwd = roofline_bwd, roofline
    if roofline["traffic"] is None and pmc_why_not:
        roofline["traffic_unavailable"] = pmc_why_not
    roofline["second_kernel"] = roofline_bwd
    roofline["timing"] = (f"HIP event pairs around the {len(rnn_calls['fwd'])} + {len(rnn_calls['bwd'])} recurrence calls of the timed region"
                          if timed_in_region else "stand-alone probe after the timed region")

    if args.breakdown and rank == 0:
        breakdown(model, tr, x, targets, pct, tsz)

    if rank == 0:
        used = [batches[k % len(batches)] for k in range(args.warmup, args.warmup + args.steps)]
        step_flops = sum(sum(train_flops_per_utt(rnn, H, L, C, (int(round(float(p) * int(b[0].size(3)))) + 1) // 2) for p in b[2]) for b in used) / len(used)
        out = {
            "metric": "utterances/sec (10 s, 161-bin) DS2 5x1024 BiGRU CTC train step" if args.workload == "c3"
                      else f"utterances/sec DS2 {L}x{H} bi-{rnn} CTC train step",
            "value": utts, "unit": "utterances/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype_label(dtype),
            **({"dtype_note": F32_NOTE} if dtype_label(dtype).startswith("fp32-grade") else {}),
            "data": "synthetic N(0,1) 161-bin spectrograms, random-init weights, random labels U=T_in/20",
            "config": {"workload": f"{args.workload}: DS2 {L}x{H} bi-{rnn.upper()} {dtype}, {tin} input frames ({tin // 100} s), "
                                   f"batch {B}/GPU, {C} classes", "global_batch": B * world, "parallelism": f"dp{world}",
                       **({"sampler": sampler_note} if sampler_note else {})},
            "loss": lv, "step_tflops": step_flops * world / (ms * 1e-3) / 1e12,
            "step_frac_of_fp32_mfma_peak": step_flops / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
            **({"step_frac_of_split_bf16_peak": step_flops / (ms * 1e-3) / 1e12 / SPLIT_BF16_PEAK_TFLOPS, "split_bf16_peak_note": SPLIT_PEAK_NOTE}
               if (dtype == "f32" and _engine.F32_GEMM == "split") else {}),
            "step_frac_of_bf16_mfma_peak": step_flops / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
            "roofline": roofline,
            # train steps of this run (warm-up included) in which a persistent recurrence launch starved and the step was skipped
            "persistent_starved_steps": DeepSpeechTrainer.starved_steps - starved_before,
            "valid_last_step": bool(valid),
            **({"dist": dist_info} if dist_info else {}),
        }
        if args.full and world == 1 and not args.no_other_workloads and args.workload == "c3" and not args.dtype and not args.batch:
            # the other single-GPU configurations of BASELINE.json in the driver-written record (short, after the timed region)
            del model, tr, opt, batches, x
            torch.cuda.empty_cache()
            t_other = time.time()
            other = {}
            # (c3_f32: the metric configuration itself at fp32-grade parity — the number behind "matched CTC loss +-1e-3" beyond four steps)
            for name, wl, dt_, st in (("c2_f32", "c2", "f32", 6), ("c4_f32", "c4", "f32", 8), ("c3_f32", "c3", "f32", 6)):
                try:
                    other[name] = quick_workload(wl, dt_, dev, st, 2) if time.time() - t_other < 40 else {"skipped": "time box"}
                except Exception as e:
                    other[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
            # BASELINE configs[1] (1 x MI355X, fp32) on the reference's own arithmetic, next to the emulated one: fp32-input MFMA kernels throughout
            other["c2_true_f32"] = quick_workload_true_f32("c2", 5) if time.time() - t_other < 60 else {"skipped": "time box"}
            out["other_workloads"] = other
            out["dp_path_1rank"] = dp_path_one_rank() if time.time() - t_other < 60 else {"skipped": "time box"}
            model = tr = opt = batches = None
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(rnn, H, L, C, tin, B)
            if out["cpu_baseline"].get("losses"):
                model = tr = opt = batches = None                # the parity runs build their own models from the CPU port's weights
                torch.cuda.empty_cache()
                out["loss_parity"] = loss_parity(rnn, H, L, C, tin, out["cpu_baseline"], dev)
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


def breakdown(model, tr, x, targets, pct, tsz):
    """Section timing with events (one extra step, outside the timed region)."""
    from asr_amd import engine, ops
    from asr_amd.ctc import _prep_targets
    dev = x.device
    B = x.size(0)
    ev = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        ev.append((name, e))

    input_sizes = pct.clone().mul_(int(x.size(3))).int()
    out_lens = model.get_seq_lens(input_sizes)
    lens_dev = out_lens.to(dev)
    tg, off, tl, max_u = _prep_targets(targets, tsz, dev)
    W = model._flat.tensors(model)
    Gr = model._flat.tensors(model, grads=True)
    orig_rnn_fwd, orig_rnn_bwd, orig_gemm, orig_rnn_bwd_bn = ops.rnn_fwd, ops.rnn_bwd, ops.gemm_raw, ops.rnn_bwd_bn
    acc = {"rnn_fwd": 0.0, "rnn_bwd": 0.0, "gemm": 0.0}

    def timed(fn, key):
        def w(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            pend.append((key, s, e))
            return r
        return w
    pend = []
    ops.rnn_fwd, ops.rnn_bwd, ops.gemm_raw = timed(orig_rnn_fwd, "rnn_fwd"), timed(orig_rnn_bwd, "rnn_bwd"), timed(orig_gemm, "gemm")
    ops.rnn_bwd_bn = timed(orig_rnn_bwd_bn, "rnn_bwd")
    try:
        with torch.no_grad():
            torch.cuda.synchronize()
            mark("start")
            logits, ctx = engine.forward(W, model._cfg, x, lens_dev, training=True, save=True)
            mark("forward")
            nll, dlogits = ops.ctc_loss(logits, tg, off, lens_dev, tl, max_u, 1.0 / B)
            mark("ctc")
            engine.backward(W, Gr, model._cfg, ctx, dlogits)
            mark("backward")
            tr._optimizer.step()
            mark("adamw")
            torch.cuda.synchronize()
    finally:
        ops.rnn_fwd, ops.rnn_bwd, ops.gemm_raw, ops.rnn_bwd_bn = orig_rnn_fwd, orig_rnn_bwd, orig_gemm, orig_rnn_bwd_bn
    for key, s, e in pend:
        acc[key] += s.elapsed_time(e)
    msg = ["breakdown (ms):"]
    for (n0, e0), (n1, e1) in zip(ev[:-1], ev[1:]):
        msg.append(f"  {n1}: {e0.elapsed_time(e1):.2f}")
    msg.append("  of which " + ", ".join(f"{k}={v:.2f}" for k, v in acc.items()))
    print("\n".join(msg), file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
