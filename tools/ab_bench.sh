#!/bin/bash
# A/B through bench.py (GPU box, repo root), alternated:
#   bash tools/ab_bench.sh <out log> VAR v1 v2 [rounds]        two values of a tuning environment variable
#   bash tools/ab_bench.sh <out log> TREE dir1 dir2 [rounds]   two built checkouts (e.g. the parent commit next to this one): each runs
#                                                              its own bench.py, package and library
# every run must succeed (set -e): a failing GPU step ends the script
set -e
J=$(mktemp)                   # the line of the current run
OUT=$1; VAR=$2; A=$3; B=$4; R=${5:-2}
for ((i = 0; i < R; ++i)); do
  for v in $A $B; do
    if [ "$VAR" = TREE ]; then BENCH=$v/bench.py; else export $VAR=$v; BENCH=bench.py; fi
    timeout -k 10 200 python3 $BENCH --full --no-cpu-baseline --no-parity-gate --steps 40 > $J 2>/dev/null
    python3 - <<EOF2 >> $OUT
import json; d = json.load(open("$J")); print("$VAR=$v", round(d["ms_per_step"], 3), [round(s["ms"], 3) for s in d["roofline"]["stages"]])
EOF2
  done
done
