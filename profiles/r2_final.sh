#!/bin/bash
# End-of-round artifacts: GPU suite, default bench (with CPU baselines),
# warmup-60 bench, chess bench.  Usage: bash profiles/r2_final.sh <tag>
export OUT_ROOT=${OUT_ROOT:-bench_out}  # where the results go (the scripts called below use it too)
set -o pipefail
tag=${1:-r2v}
bash profiles/gpu_check.sh $tag || exit 1
timeout -k 10 300 python bench.py --full --game chess > $OUT_ROOT/$tag/bench_chess.json 2> $OUT_ROOT/$tag/bench_chess.err || { tail $OUT_ROOT/$tag/bench_chess.err; exit 1; }
tail -c 600 $OUT_ROOT/$tag/bench_chess.json
