#!/bin/bash
# A/B of the two-files-in-flight region of bench.py (two contexts / streams / host threads) with alternative builds.
out=bench_out/ab
mkdir -p $out
i=0
for lib in "$@"; do
  i=$((i+1)); name=ov_$(basename $lib .so)_$i
  PGW_LIB=$PWD/$lib python bench.py --full --no-cpu-baseline --no-extras --overlap-streams ${OV:-2} --steps 12 --warmup 2 > $out/$name.json 2> $out/$name.err || echo "$name failed"
  python - <<PY
import json
d=json.load(open('$out/$name.json'))
print('$lib', d['ms_per_step'], d['overlap'], {k:v['avg_ms'] for k,v in d['kernels'].items()})
PY
done
