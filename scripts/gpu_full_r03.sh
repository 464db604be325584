#!/bin/bash
# Round-3 full pass: GPU tests, smoke, default bench (N=1, all aux), and the
# headline's kernel trace.  Each GPU step has its own time limit.
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"; LOGS=${LOGS:-bench_logs}; mkdir -p "$LOGS"; export TMPDIR=/tmp
if [ "${SKIP_TESTS:-0}" != 1 ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q -rf -p no:cacheprovider --timeout 240 --timeout-method thread > $LOGS/gpu_tests.log 2>&1; rc=$?
  echo "tests rc=$rc"; tail -6 $LOGS/gpu_tests.log
  if [ $rc -gt 1 ]; then exit $rc; fi
  timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $LOGS/smoke.log 2>&1 || { echo smoke failed; tail $LOGS/smoke.log; exit 3; }
  tail -1 $LOGS/smoke.log
fi
timeout -k 10 600 python -u bench.py --full > $LOGS/bench.log 2>&1 || { echo bench failed; tail -20 $LOGS/bench.log; exit 4; }
grep "^{" $LOGS/bench.log | tail -1 | cut -c1-600
if [ "${SKIP_KT:-0}" != 1 ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $LOGS/kt -o kt -- python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-aux > $LOGS/kt.log 2>&1 || { echo ktrace failed; tail -5 $LOGS/kt.log; exit 5; }
  find $LOGS/kt -name "*stats*.csv" | head
fi
echo done
