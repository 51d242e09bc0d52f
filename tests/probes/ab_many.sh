#!/bin/bash
# Same-box comparison of several builds of the library on a bench line: tests/probes/ab_many.sh "bench args" LIB...
source tests/probes/gpu_steps.sh
OUT=${OUT:-$(mktemp -d)}   # the bench line and log of the latest run
ARGS=$1; shift
for round in 1 2; do
  for lib in "$@"; do
    export HBMRAG_LIB=$lib
    step 400 python bench.py --full --no-cpu-baseline --no-api-concurrent --no-config4-full --no-latency $ARGS > "$OUT/ab.json" 2> "$OUT/ab.err"
    python - "$lib" "$OUT/ab.json" <<'PY'
import json, sys
d = [json.loads(l) for l in open(sys.argv[2]) if l.startswith("{")][0]
print(sys.argv[1].split("/")[-1], round(d["value"]), round(d["ms_per_step"], 4), d["kernel_ms"], d.get("finishing_alone", {}).get("finish_us"), d["all_lists_proven_exact"])
PY
  done
done
