#!/bin/bash
# One-card rehearsal of the synchronous PS with backup workers (parallel/sync_ps.py): 1 PS + N workers, all on
# cuda:0, point-to-point over gloo with host staging (DTG_BACKEND=gloo DTG_GLOO_DEVICE=cuda).  On a node the same
# example runs over RCCL with one GPU per process (examples/ResNet50/run_sync_ps.sh).  Every process runs under
# its own time limit; exits non-zero if any process fails.
#   tools/sync_ps_rehearsal.sh [workers=3] [extra flags for resnet50_sync_ps.py, e.g. --replicas_to_aggregate 2]
set -u
N=${1:-3}; shift || true
cd "$(dirname "$0")/../examples/ResNet50"
export DTG_BACKEND=gloo DTG_GLOO_DEVICE=cuda
export DTG_SYNC_TIMEOUT=${DTG_SYNC_TIMEOUT:-120} DTG_PS_WORKER_TIMEOUT=${DTG_PS_WORKER_TIMEOUT:-120}
PORT=$((25000 + RANDOM % 2000))
pids=()
timeout -k 10 240 python -u resnet50_sync_ps.py --job_name ps --task_index 0 --workers "$N" --base_port $PORT "$@" &
pids+=($!)
for i in $(seq 0 $((N - 1))); do
  timeout -k 10 240 python -u resnet50_sync_ps.py --job_name worker --task_index "$i" --workers "$N" --base_port $PORT "$@" &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait "$p" || rc=$?; done
echo "sync_ps_rehearsal rc=$rc"
exit $rc
