#!/bin/bash
# The short bench command (python3 bench.py --gpus 1 --steps 20 --warmup 5, here with --full) beside the default
# run (200 timed polls after 20 warmup, no extras), alternating on one box: ms per poll and chain.
set -u
OUT=${OUT:-bench_out}   # where the logs go
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
for r in 1 2 3; do
  timeout -k 10 200 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/drv$r.log 2>&1 || exit $?
  python3 - $OUT/drv$r.log <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][0])
print("steps20", round(d["ms_per_step"], 4), round(d["roofline"]["chain_ms"] * 1e3, 1), d.get("check_timed_poll_vs_scan"))
PY
  timeout -k 10 200 python3 bench.py --full --no-cpu --no-extras > $OUT/drvd$r.log 2>&1 || exit $?
  python3 - $OUT/drvd$r.log <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][0])
print("default", round(d["ms_per_step"], 4), round(d["roofline"]["chain_ms"] * 1e3, 1), d["steps"], d["warmup"])
PY
done
