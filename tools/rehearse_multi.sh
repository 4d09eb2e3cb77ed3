#!/bin/bash
# 2-rank rehearsal of bench.py's multi-GPU path (--full: with the node-level
# queries) on a 1-GPU box: both ranks on cuda:0, collectives over gloo (RCCL
# needs one GPU per rank).  Output: $OUT_DIR (default bench_out/).
set -o pipefail
O=${OUT_DIR:-bench_out}; mkdir -p $O
TFIDF_BENCH_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 2 --warmup 1 --docs ${DOCS:-200000} \
  --cpu-sample 0 > $O/multi.log 2>&1
rc=$?; tail -3 $O/multi.log | cut -c1-600; exit $rc
