set -o pipefail
mkdir -p gpurun_out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > gpurun_out/pytest_gpu.log 2>&1; rc=$?
echo "pytest rc=$rc"; tail -15 gpurun_out/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
mkdir -p bench_out
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 > bench_out/bench1.json 2> bench_out/bench1.err; rc=$?
echo "bench rc=$rc"; cat bench_out/bench1.json; tail -3 bench_out/bench1.err
