#!/bin/bash
# GPU-box check: smoke, GPU parity suite, a short bench.  Each GPU step has its
# own time limit; logs go to $OUT/ (AMX_OUT, default out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1
rc=$?; echo "smoke_rc=$rc" >> $OUT/smoke.log
case $rc in 124|134|137|139) exit $rc;; esac
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread ${PYTEST_ARGS} > $OUT/gpu_tests.log 2>&1
rc=$?; echo "tests_rc=$rc" >> $OUT/gpu_tests.log
case $rc in 124|134|137|139) exit $rc;; esac
timeout -k 10 300 python bench.py --full --steps 5 --warmup 2 ${BENCH_ARGS} > $OUT/bench.log 2>&1
rc=$?; echo "bench_rc=$rc" >> $OUT/bench.log
exit $rc
