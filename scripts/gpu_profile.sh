#!/bin/bash
# rocprofv3 kernel-trace summary of the default bench (writes $OUT/prof_*)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-r01}
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline ${BENCH_ARGS} > $OUT/prof_${TAG}.log 2>&1
echo "prof_rc=$?" >> $OUT/prof_${TAG}.log
