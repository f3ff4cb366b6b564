#!/bin/bash
# row (e) rehearsal on a one-GPU box: bench.py --gpus 2 starts its own two ranks, which share the GPU and exchange over gloo;
# --full adds the two other multi-GPU workloads.  usage: tools/dev/run_two_ranks.sh [log file]
cd "$(dirname "$0")/../.."
LOG=${1:-${TMPDIR:-/tmp}/two_ranks.log}
timeout -k 10 600 python bench.py --gpus 2 --scale 14 --edges 200000 --steps 3 --warmup 1 --no-cpu-baseline --full > "$LOG" 2>&1; echo "rc=$?"
grep "^{" "$LOG" | tail -1 | cut -c1-3000
