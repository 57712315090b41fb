#!/bin/bash
# GPU-box check: parity tests, then a short bench, then a kernel-trace profile of the bench.
# Run via gpurun from the repo root:  gpurun -- bash scripts/gpu_check.sh [rows]
cd $GRAFT_REPO_ROOT
# results go to $OUT (default: run_out/ under the repository root)
ROOT=$PWD
OUT=$(realpath -m "${OUT:-run_out}")
mkdir -p "$OUT"
ROWS=${1:-1048576}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 && \
timeout -k 10 400 python -u bench.py --full --steps 2 --warmup 1 --rows-per-gpu $ROWS --cpu-seconds 8 > "$OUT/bench_small.json" 2> "$OUT/bench_small.log" && \
cd /tmp && export TMPDIR=/tmp && \
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run --output-format csv -- python3 "$ROOT/bench.py" --full --steps 2 --warmup 1 --rows-per-gpu $ROWS --no-cpu-baseline > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.log"
