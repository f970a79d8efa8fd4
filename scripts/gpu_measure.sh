#!/bin/bash
# GPU box: the round's measurements. For every "<config> <precision>" spec: kernel trace + PMC passes
# (scripts/prof_pmc.sh) whose summaries are copied into profiles/ on the box; then one full bench line per
# config (bench.py --full: fp64 headline + fp32 alt line, CPU baseline and full-size parity rows), which
# reads those summaries for its rooflines.
#   scripts/gpu_measure.sh <tag> "<config> <precision>" ... -- <config> ...
# Output under $RT_MEASURE_OUT/<tag>/ (default measure_out/). Each GPU step has its own time limit and
# the chain stops at the first failure.
set -e
tag=$1; shift
export TMPDIR=/tmp
out=${RT_MEASURE_OUT:-measure_out}/$tag
mkdir -p $out profiles
while [ $# -gt 0 ] && [ "$1" != "--" ]; do
  set -- $1 "${@:2}"
  cfg=$1; prec=$2; shift 2
  bash scripts/prof_pmc.sh $out/${cfg}_$prec ${tag}_${cfg}_$prec --config $cfg --precision $prec
  cp $out/${cfg}_$prec/summary/* profiles/
done
[ "$1" == "--" ] && shift
for cfg in "$@"; do
  timeout -k 10 600 python3 bench.py --full --config $cfg > $out/bench_$cfg.json 2> $out/bench_$cfg.err
  cut -c1-400 $out/bench_$cfg.json
done
