#!/bin/bash
# One full bench line per workload (run from the repo root on a GPU host): $OUT/<name>.json
set -o pipefail
OUT=${OUT:-bench_out/sweep}
mkdir -p $OUT
for spec in "default|" "synthetic|--model synthetic" "qsize|--model qsize --no-edge-cut" "geant2|--topology geant2 --no-edge-cut" \
            "train|--train" "train_fresh|--train --fresh-batches"; do
  name=${spec%%|*}; args=${spec#*|}
  timeout -k 10 400 python -u bench.py --full $args > $OUT/$name.json 2> $OUT/$name.err || {
    echo "$name failed"; exit 1; }
  echo "$name done"
done
