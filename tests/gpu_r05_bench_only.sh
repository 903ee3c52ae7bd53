#!/bin/bash
# the driver's bench command on its own (after the capture guard: a dropped engine's hipGraphs must not be destroyed inside another capture)
cd "${GRAFT_REPO_ROOT:-.}"; mkdir -p gpurun_out; export TMPDIR=/tmp
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"       # where the bench.py lines of this session write
timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT"/r05_bench.json 2> "$OUT"/r05_bench.err; echo "bench=$?"; tail -2 "$OUT"/r05_bench.err
python tools/bench_summary.py "$OUT"/r05_bench.json
