#!/bin/bash
# C2 kernel-trace summary + one SQ PMC pass (separate runs; counters never mixed with traces)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-r01_c2}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline ${BENCH_ARGS} > $OUT/prof_${TAG}.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU -d $OUT/pmc_${TAG}_sq -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS} > $OUT/pmc_${TAG}_sq.log 2>&1 || exit $?
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_LDS SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR GRBM_GUI_ACTIVE -d $OUT/pmc_${TAG}_lds -o run --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS} > $OUT/pmc_${TAG}_lds.log 2>&1
