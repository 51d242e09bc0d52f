#!/bin/bash
# Same-box A/B of two builds of the library on the default bench line: tests/probes/ab_default.sh LIB_A LIB_B [extra bench args]
source tests/probes/gpu_steps.sh
OUT=${OUT:-$(mktemp -d)}   # the bench line and log of the latest run
A=$1; B=$2; shift 2
for round in 1 2; do
  for lib in "$A" "$B"; do
    export HBMRAG_LIB=$lib
    step 400 python bench.py --full --no-cpu-baseline --no-api-concurrent --no-config4-full --no-latency --steps 50 "$@" > "$OUT/ab.json" 2> "$OUT/ab.err"
    python - "$lib" "$OUT/ab.json" <<'PY'
import json, sys
d = [json.loads(l) for l in open(sys.argv[2]) if l.startswith("{")][0]
print(sys.argv[1].split("/")[-1], round(d["value"]), round(d["ms_per_step"], 4), d["kernel_ms"], d.get("finishing_alone", {}).get("finish_us"), d["all_lists_proven_exact"])
PY
  done
done
