#!/bin/bash
# round 6 session F: two engines as the default at 512 rows -- bit-equality test, the bench line with it
cd "${GRAFT_REPO_ROOT:-.}"; mkdir -p gpurun_out; export TMPDIR=/tmp
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"       # where the bench.py lines of this session write
timeout 900 python -m pytest tests/test_model_gpu.py -q -x -k "two_engines or picks_two" 2>&1 | grep -v amdgpu.ids | tail -3
timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-train --no-cpu-baseline --no-chunk > "$OUT"/r06_f_bench.json 2> "$OUT"/r06_f_bench.err; echo "bench=$?"; tail -3 "$OUT"/r06_f_bench.err
python tools/bench_summary.py "$OUT"/r06_f_bench.json 2>&1 | head -40
