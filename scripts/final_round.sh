set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/r05n_gputest.log 2>&1 || { echo "gpu tests failed"; tail -30 $OUT/r05n_gputest.log; exit 3; }
tail -3 $OUT/r05n_gputest.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/r05n_smoke.log 2>&1 || { echo "smoke failed"; tail -20 $OUT/r05n_smoke.log; exit 4; }
tail -2 $OUT/r05n_smoke.log
timeout -k 10 900 python -u bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/r05n_bench.log 2>&1 || { echo "bench failed"; tail -20 $OUT/r05n_bench.log; exit 5; }
tail -1 $OUT/r05n_bench.log | cut -c1-400
