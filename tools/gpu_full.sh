#!/bin/bash
# Whole GPU suite, smoke, the default bench with every leg (--full), then the
# multi-GPU code path over RCCL at one rank (TFIDF_BENCH_DIST=1: process group,
# GLOBAL exchange, node-level batched queries).  Every GPU step bounded; stop at
# the first failure.  Output: $OUT_DIR (default bench_out/).
set -o pipefail
O=${OUT_DIR:-bench_out}; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --durations=15 --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1
rc=$?; tail -4 $O/gpu_tests.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
rc=$?; tail -2 $O/smoke.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > $O/bench.log 2> $O/bench.err
rc=$?; [ $rc -ne 0 ] && { tail -20 $O/bench.err; exit $rc; }
python - $O/bench.log <<'PY'
import json
import sys
r = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value %.4g docs/s  ms/step %.2f" % (r["value"], r["ms_per_step"]))
print("roofline", {k: r["roofline"][k] for k in ("kernel", "achieved", "frac", "avg_launch_ms")})
print("queries", {k: v for k, v in r.get("queries", {}).items() if k != "roofline"})
PY
[ -n "${NO_DIST:-}" ] && exit 0
TFIDF_BENCH_DIST=1 timeout -k 10 300 python -u -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --full --steps 3 --warmup 1 --cpu-sample 0 --no-e2e --batch-queries 2000 > $O/bench_dist1.log 2> $O/bench_dist1.err
rc=$?; [ $rc -ne 0 ] && { tail -20 $O/bench_dist1.err; exit $rc; }
tail -1 $O/bench_dist1.log | cut -c1-600
