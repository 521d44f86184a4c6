#!/bin/bash
# C3 PMC passes (SQ wave-state counters; TA busy) -- separate runs, no traces mixed in
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-r01_c3}
CMD="python3 bench.py --full --config c3 --steps 2 --warmup 1 --no-cpu-baseline"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU -d $OUT/pmc_${TAG}_sq -o run --output-format csv -- $CMD > $OUT/pmc_${TAG}_sq.log 2>&1 || exit $?
timeout -k 10 120 rocprofv3 -L > $OUT/counters_list.txt 2>&1
timeout -k 10 300 rocprofv3 --pmc TA_BUSY_avr TA_BUSY_max SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE -d $OUT/pmc_${TAG}_ta -o run --output-format csv -- $CMD > $OUT/pmc_${TAG}_ta.log 2>&1
exit 0
