#!/bin/bash
# Quick bench: the PTA leg and the predicted strong scaling only (no grid / J0740 / C2 / CPU
# baseline / cold start); the JSON line to $OUT/benchq.json, a brief to stdout.
set -u
cd "$(dirname "$0")/.."
OUT=${PINT_OUT:-bench_out}  # where the records go
mkdir -p "$OUT"
timeout -k 10 400 python3 bench.py --full --steps ${STEPS:-100} --warmup ${WARM:-10} --grid 0 --j0740 0 --c2 0 --cpu-baseline 0 --cold-start 0 "$@" \
    > $OUT/benchq.json 2> $OUT/benchq.err || { tail -20 $OUT/benchq.err; exit 1; }
grep -v "^\[trace\]" $OUT/benchq.err | tail -12
python3 scripts/bench_brief.py $OUT/benchq.json
