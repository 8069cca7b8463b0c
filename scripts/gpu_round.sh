#!/bin/bash
# Round measurements on the GPU box: hardware probes (FP64 MFMA rate, FP64 VALU issue and
# latency, MFMA/VALU co-issue, HBM copy), the default bench line, then scripts/gpu_prof.sh.
# Every GPU step has its own time limit; any failure stops the script.
set -u
cd "$(dirname "$0")/.."
OUT=${PINT_OUT:-bench_out}  # where the records go
mkdir -p "$OUT"
timeout -k 10 60 ./build/peaks > $OUT/peaks.json || exit $?
timeout -k 10 60 ./build/mfma_probe > $OUT/mfma_probe.json || exit $?
timeout -k 10 60 ./build/valu_probe > $OUT/valu_probe.txt || exit $?
timeout -k 10 60 ./build/coissue_probe > $OUT/coissue_probe.txt || exit $?
timeout -k 10 400 python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || exit $?
bash scripts/gpu_prof.sh
