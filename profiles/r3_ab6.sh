#!/bin/bash
# round 3 A/B 6: lagged activation reads (lag) and + buffer-load weight stream (lagbuf) vs base
set -o pipefail
out=gpurun_out/r3_ab6
mkdir -p $out
for v in lag lagbuf; do
  AZ_LIB_PATH=$PWD/profiles/ab_libs/$v/libaz.so timeout -k 10 400 python -u -m pytest tests/test_engine_gpu.py -x -q --timeout 120 --timeout-method thread -k "tower or keras or batch_invariant or replays" \
    > $out/tests_$v.log 2>&1 || { tail -30 $out/tests_$v.log; exit 1; }
  tail -1 $out/tests_$v.log
done
for v in base lag lagbuf base lag lagbuf; do
  bash profiles/tower_ab.sh run $v 2>&1 | grep -v amdgpu.ids | tee -a $out/times.txt || exit 1
done
i=0
for v in base lag lagbuf base lag lagbuf; do
  i=$((i+1))
  if [ $v = base ]; then lib=custom-alphazero_amd/custom_alphazero/_lib/libaz.so; else lib=profiles/ab_libs/$v/libaz.so; fi
  AZ_LIB_PATH=$PWD/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-cache-window > $out/b${v}_$i.json 2> $out/b${v}_$i.err || { tail -5 $out/b${v}_$i.err; exit 1; }
  python3 -c "
import json,sys; d=json.loads(open('$out/b${v}_$i.json').read().strip().splitlines()[-1]); r=d['roofline']
print('$v', d['value'], d['ms_per_step'], 'tower', r['avg_launch_ms'], 'frac', r['frac'], 'iso', r['isolated']['avg_launch_ms'], 'busy_union', r['busy_union']['frac'])" | tee -a $out/bench.txt
done
