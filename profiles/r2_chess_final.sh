#!/bin/bash
OUT_ROOT=${OUT_ROOT:-bench_out}  # where the results go
set -o pipefail
mkdir -p $OUT_ROOT/r2i
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT_ROOT/r2i/gpu_tests.log 2>&1 || { tail -30 $OUT_ROOT/r2i/gpu_tests.log; exit 1; }
tail -2 $OUT_ROOT/r2i/gpu_tests.log
timeout -k 10 300 python bench.py --full --game chess > $OUT_ROOT/r2i/bench_chess.json 2> $OUT_ROOT/r2i/bench_chess.err || { tail $OUT_ROOT/r2i/bench_chess.err; exit 1; }
python3 -c "
import json; d=json.loads(open('$OUT_ROOT/r2i/bench_chess.json').read().strip().splitlines()[-1]); print('chess', d['value'], d['roofline']['frac'], d.get('gpu_over_cpu'))"
