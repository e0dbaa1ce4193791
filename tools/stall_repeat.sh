#!/bin/bash
# Round 3: run the benchmark's rows several times with STG_BENCH_DEBUG=1; every timed block prints its wall time, the device's
# own span and the container's cgroup cpu.stat delta (nr_throttled / throttled_usec) over the block.
set -o pipefail
# usage: tools/stall_repeat.sh <out dir> [runs] [NAME=value ...]   (NAME=value: settings for the runs, e.g. STG_HIP_LIBRARY=<build>)
OUT=${1:?usage: tools/stall_repeat.sh <out dir> [runs] [NAME=value ...]}; N=${2:-6}; shift $(( $# < 2 ? $# : 2 ))
mkdir -p "$OUT"
for i in $(seq 1 $N); do
  env STG_BENCH_DEBUG=1 "$@" python3 bench.py --full --cpu-baseline 0 --pmc off > $OUT/run$i.json 2> $OUT/run$i.err || { tail -5 $OUT/run$i.err; exit 1; }
  echo "run $i done"
done
