#!/bin/bash
# Synchronous SGD with backup workers: 1 PS + N workers, one process per MI355X (rank r uses GPU r, every process
# sees every GPU so each PS<->worker pair can take its direct xGMI link; see run_async.sh).  Extra flags are
# forwarded, e.g.  WORKERS=7 bash run_sync_ps.sh --replicas_to_aggregate 6 --steps 50
# Waits for every process and exits non-zero if any of them failed.
cd "$(dirname "$0")"
N=${WORKERS:-7}
pids=()
python resnet50_sync_ps.py --job_name ps --task_index 0 --workers "$N" "$@" &
pids+=($!)
for i in $(seq 0 $((N - 1))); do
  python resnet50_sync_ps.py --job_name worker --task_index "$i" --workers "$N" "$@" &
  pids+=($!)
done
status=0
for p in "${pids[@]}"; do
  wait "$p" || status=1
done
exit $status
