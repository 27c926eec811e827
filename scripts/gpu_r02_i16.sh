OUT="${EWK_OUT:-$PWD/out}"; mkdir -p "$OUT"   # logs and profiler output
# int16 rings: parity tests, then the streaming sections of the bench
set -o pipefail
timeout -k 10 500 python -u -m pytest tests/test_gpu_int16_ring.py tests/test_gpu_level3.py tests/test_gpu_compact_ring.py -v -m gpu -x -p no:cacheprovider --timeout 300 --timeout-method thread > $OUT/pytest_i16.log 2>&1 && \
timeout -k 10 600 python bench.py --full --steps 5 --warmup 3 --no-cpu-baseline --fixed-len 0 --confirm-batch 0 > $OUT/bench_i16.log 2>&1
rc=$?; tail -3 $OUT/pytest_i16.log; exit $rc
