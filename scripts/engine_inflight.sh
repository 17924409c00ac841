#!/bin/bash
# Mean passes in flight of the job engine: sum(device_ms) / wall_ms from the
# bench's engine block.  SETS="args|args|..." one bench per set, each with its
# own time limit; stops at the first failure.  OUTDIR (default: a
# directory under TMPDIR) receives the logs and OUT, the table.
set -u
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUTDIR=${OUTDIR:-$TMPDIR/engine_inflight}
mkdir -p "$OUTDIR"
OUT=$OUTDIR/${OUT:-inflight.txt}
BASE=${BASE_ARGS:---gpus 1 --warmup 5 --no-extras --no-cpu-baseline --no-prover --msm=}
IFS='|' read -ra SETS <<< "${SETS:-}"
i=0
for s in "${SETS[@]}"; do
  i=$((i + 1))
  log=$OUTDIR/inflight_$i.log
  timeout -k 10 240 python -u bench.py $BASE $s > $log 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "[$s] bench failed rc=$rc"; tail -30 $log; exit 4; fi
  tail -1 $log | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
e=d['engine']
wall=d['ms_per_step']*d['steps']
dev=e['device_ms_per_batch']*e['batches']
print('[$s] value', d['value'], 'exact', d.get('verdicts_bit_exact'), 'batches', e['batches'], 'device_ms/batch', e['device_ms_per_batch'],
      'job_ms', round(wall,1), 'mean_in_flight', round(dev/wall,2), 'max_in_flight', e['max_in_flight'],
      'plan_ms', e['host_plan_ms_per_batch'], 'enqueue_ms', e['enqueue_ms_per_batch'], 'device_only', (d.get('device_only') or {}).get('transfers_per_s'))
" | tee -a $OUT
done
