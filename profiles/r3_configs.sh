#!/bin/bash
# the other BASELINE configs + chess on the round-3 build (one MI355X)
export OUT_ROOT=${OUT_ROOT:-bench_out}  # where the results go (the scripts called below use it too)
set -o pipefail
bash profiles/bench_configs.sh || exit 1
timeout -k 10 300 python bench.py --full --game chess > $OUT_ROOT/configs/chess.json 2> $OUT_ROOT/configs/chess.err || { tail $OUT_ROOT/configs/chess.err; exit 1; }
for f in s400 s400_32k c5_9x9 chess; do
python3 -c "
import json; d=json.loads(open('$OUT_ROOT/configs/$f.json').read().strip().splitlines()[-1]); r=d['roofline']
print('$f', d['value'], d['unit'], 'exp/s', d.get('expansions_per_s'), 'frac', r['frac'], 'hit', (d.get('transposition_cache') or {}).get('hit_rate'))"
done
