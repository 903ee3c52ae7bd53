#!/bin/bash
# round 6 session H: the opt-in bf16 recurrent state -- kernel + engine parity on the GPU, the bench block
cd "${GRAFT_REPO_ROOT:-.}"; mkdir -p gpurun_out; export TMPDIR=/tmp
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"       # where the bench.py lines of this session write
LINA_PARITY_TAG=r06h timeout 1200 python -m pytest tests/test_kernels_gpu.py tests/test_model_gpu.py -q -x -k "bf16_state or decode_window" 2>&1 | grep -v amdgpu.ids | tail -4
timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-train --no-cpu-baseline > "$OUT"/r06_h_bench.json 2> "$OUT"/r06_h_bench.err; echo "bench=$?"; tail -3 "$OUT"/r06_h_bench.err
python tools/bench_summary.py "$OUT"/r06_h_bench.json 2>&1 | head -40
