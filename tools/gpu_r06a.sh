set -o pipefail
OUT=${OUT:-bench_out/r06a}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest -x -v --timeout 200 --timeout-method thread -m gpu tests/test_host_pipeline.py "tests/test_gpu_parity.py::test_product_full_size_parity" "tests/test_gpu_parity.py::test_ragged_batch_sizes" "tests/test_gpu_parity.py::test_debug_switches_do_not_change_results" > $OUT/pytest.txt 2>&1 &&
timeout -k 10 300 python -u bench.py --host --full --steps 20 --warmup 3 --cpu-sample 65536 > $OUT/bench_host.json 2> $OUT/bench_host.err &&
timeout -k 10 300 python -u bench.py --steps 20 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err
rc=$?
tail -15 $OUT/pytest.txt; cat $OUT/bench_host.json $OUT/bench.json; exit $rc
