#!/bin/bash
# GPU-box quick pass: parity tests, smoke, then the default bench (one JSON line).
# Run via gpurun from the repo root:  gpurun -- bash scripts/gpu_quick.sh
cd $GRAFT_REPO_ROOT
# results go to $OUT (default: run_out/ under the repository root)
OUT=${OUT:-run_out}
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 && \
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 && \
timeout -k 10 300 python -u bench.py --full --cpu-seconds 5 > "$OUT/bench_default.json" 2> "$OUT/bench_default.log"
