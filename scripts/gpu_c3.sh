#!/bin/bash
# C3 (multiband + width + analog) bench + rocprof summary
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-r01_c3}
timeout -k 10 300 python bench.py --full --config c3 --steps 5 --warmup 2 > $OUT/bench_c3.log 2>&1
rc=$?; echo "rc=$rc" >> $OUT/bench_c3.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- python3 bench.py --full --config c3 --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_${TAG}.log 2>&1
echo "prof_rc=$?" >> $OUT/prof_${TAG}.log
