#!/bin/bash
export DS2_EXPERIMENTAL=1   # the A/B switches below are honoured only with this (asr_amd/engine.py::_tune, csrc/common.h::ds2_exp_getenv)
# whole GPU suite + smoke + the full bench line (bench.py --full); the logs go to the directory given as the only argument.
# A step that times out, aborts or dies on a signal (exit status > 123) ends the script: nothing more is started on that GPU.
OUT=$(mkdir -p "${1:?usage: scripts/gpu_full.sh OUT_DIR}" && cd "$1" && pwd) || exit 1
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
stop_on_fault() { local rc=$1; echo "$2 rc=$rc"; [ "$rc" -le 123 ] || exit "$rc"; }
timeout -k 10 1500 python -m pytest tests -m gpu -x -q -p no:cacheprovider > "$OUT/full_gpu.log" 2>&1; stop_on_fault $? "gpu tests"; tail -5 "$OUT/full_gpu.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1; stop_on_fault $? smoke; tail -2 "$OUT/smoke.log"
timeout -k 10 900 python bench.py --full > "$OUT/full_bench.log" 2>&1; stop_on_fault $? bench; grep -v amdgpu.ids "$OUT/full_bench.log" | tail -2 | cut -c1-1500
