cd "${GRAFT_REPO_ROOT}"
OUT=${AMX_OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
for cfg in c4 c5; do for wu in 2048 2304; do
  timeout -k 10 300 python3 bench.py --full --config $cfg --env-warm $wu --no-cpu-baseline --no-pipeline --no-other-configs > $OUT/envwarm_${cfg}_$wu.log 2>&1 || exit 1
  python3 -c "
import json
d = json.loads([l for l in open('$OUT/envwarm_${cfg}_$wu.log') if l.startswith('{')][-1])
print('$cfg', $wu, d['ms_per_step'], d['stages_ms'].get('env'), d['stages_ms'].get('fix'), d.get('env_fixup'))
"
done; done
