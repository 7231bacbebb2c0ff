set -o pipefail
cd "$(dirname "$0")/.."
OUT=${NEMO_OUT:-bench_out} && mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gpu_tests_r02c.log 2>&1 && \
timeout -k 10 300 python bench.py --full > $OUT/bench_r02c.json 2> $OUT/bench_r02c.err && \
timeout -k 10 400 python bench.py --full --config c5 --steps 3 --warmup 1 --no-cpu-baseline --e2e-runs 0 > $OUT/bench_c5_r02c.json 2> $OUT/bench_c5_r02c.err
echo rc=$?
