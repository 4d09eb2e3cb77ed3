#!/bin/bash
# cfg-2 bench with queries (--full; no CPU sample, no end-to-end): batch and single-query figures.
# Output: $OUT_DIR (default bench_out/).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; O=${OUT_DIR:-bench_out}; mkdir -p $O
timeout -k 10 400 python -u bench.py --full --steps 3 --warmup 1 --cpu-sample 0 --no-e2e "$@" > $O/bq.json 2> $O/bq.err || { tail -5 $O/bq.err; exit 1; }
python3 -c "import json; r=json.loads(open('$O/bq.json').read().strip().splitlines()[-1]); q=r['queries']; print('batch runs', q['batch10k_device_ms_runs'], 'median', q['batch10k_device_ms'], 'single p50', q['single_top10_p50_ms'], 'all-hits 16t', q['threads16_all_hits_qps'])"
