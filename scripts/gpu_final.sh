#!/bin/bash
# Round-end check on the final tree: the GPU suite, smoke(), the default bench line, the driver's
# short form (--steps 20 --warmup 5), and the C2 / C5 lines.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$PWD
# where the logs and the JSON lines go (RESULTS=dir; default bench_out/ in the tree)
RESULTS=$(mkdir -p "${RESULTS:-bench_out}" && cd "${RESULTS:-bench_out}" && pwd)
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -v -rf --timeout 300 --timeout-method thread > $RESULTS/pytest_gpu.log 2>&1
rc=$?; tail -2 $RESULTS/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $RESULTS/smoke.log 2>&1
rc=$?; tail -1 $RESULTS/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full > $RESULTS/bench.json 2> $RESULTS/bench.err
rc=$?; echo "bench exit $rc"; [ $rc -eq 0 ] || { tail -5 $RESULTS/bench.err; exit $rc; }
timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 > $RESULTS/bench_20_5.json 2> $RESULTS/bench_20_5.err
rc=$?; echo "bench 20/5 exit $rc"; [ $rc -eq 0 ] || exit $rc
for c in c2 c5; do
  timeout -k 10 300 python bench.py --full --config $c --no-cpu-baseline --no-extras > $RESULTS/bench_$c.json 2> $RESULTS/bench_$c.err
  rc=$?; echo "bench $c exit $rc"; [ $rc -eq 0 ] || exit $rc
done
