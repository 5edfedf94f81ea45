#!/bin/bash
# One gpurun call: GPU tests, smoke, a short bench and a rocprofv3 kernel trace.
# Each GPU step has its own time limit; a crash / timeout / abort ends the script there.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$PWD
# where the logs and the JSON lines go (RESULTS=dir; default bench_out/ in the tree)
RESULTS=$(mkdir -p "${RESULTS:-bench_out}" && cd "${RESULTS:-bench_out}" && pwd)
export TMPDIR=/tmp
ok() { local rc=$1; [ "$rc" -eq 0 ] || [ "$rc" -eq 1 ]; }   # 1 = test failures, not a fault

timeout -k 10 900 python -u -m pytest tests -m gpu -v -rf --timeout 300 --timeout-method thread ${PYTEST_ARGS:-} > $RESULTS/pytest_gpu.log 2>&1
rc=$?; echo "pytest exit $rc" | tee -a $RESULTS/pytest_gpu.log; tail -5 $RESULTS/pytest_gpu.log
ok $rc || exit $rc

timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $RESULTS/smoke.log 2>&1
rc=$?; echo "smoke exit $rc"; tail -3 $RESULTS/smoke.log
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc

timeout -k 10 400 python bench.py --full --steps ${BENCH_STEPS:-10} --warmup 3 > $RESULTS/bench.json 2> $RESULTS/bench.err
rc=$?; echo "bench exit $rc"; cat $RESULTS/bench.json; tail -3 $RESULTS/bench.err
[ $rc -eq 0 ] || exit $rc

if [ -z "${NO_PROF:-}" ]; then
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $RESULTS/prof -o run -- \
      python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $RESULTS/prof_bench.log 2>&1
  rc=$?; echo "rocprof exit $rc"
fi
exit 0
