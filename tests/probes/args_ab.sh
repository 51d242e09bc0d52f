#!/bin/bash
# Same-box comparison of bench argument sets (alternating, two rounds): tests/probes/args_ab.sh "common args" "args A" "args B" ...
source tests/probes/gpu_steps.sh
OUT=${OUT:-$(mktemp -d)}   # the bench line and log of the latest run
COMMON=$1; shift
for round in 1 2; do
  for extra in "$@"; do
    step 400 python bench.py --full --no-cpu-baseline --no-api-concurrent --no-config4-full --no-latency $COMMON $extra > "$OUT/ab.json" 2> "$OUT/ab.err"
    python - "$extra" "$OUT/ab.json" <<'PY'
import json, sys
d = [json.loads(l) for l in open(sys.argv[2]) if l.startswith("{")][0]
print(repr(sys.argv[1]), round(d["value"]), round(d["ms_per_step"], 4), d["kernel_ms"], d.get("finishing_alone", {}).get("finish_us"), d["all_lists_proven_exact"])
PY
  done
done
