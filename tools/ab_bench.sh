#!/bin/bash
# A/B: bench.py's timed region with alternative builds of the library (PGW_LIB), same box, back to back.
# usage: bash tools/ab_bench.sh [ENV=VALUE:]lib_a.so lib_b.so ...   (paths relative to the repo root; results in bench_out/ab/)
out=bench_out/ab
mkdir -p $out
i=0
for spec in "$@"; do
  i=$((i+1))
  envs=""; lib=$spec
  if [[ "$spec" == *:* ]]; then envs="${spec%%:*}"; lib="${spec#*:}"; fi
  name=$(basename $lib .so)_$i
  env $envs PGW_LIB=$PWD/$lib python bench.py --full --no-cpu-baseline --no-extras --overlap-streams 0 --steps 10 --warmup 2 ${AB_ARGS} > $out/$name.json 2> $out/$name.err || echo "$name failed"
  python - <<PY
import json
d=json.load(open('$out/$name.json'))
print('$spec', d['ms_per_step'], {k:v['avg_ms'] for k,v in d['kernels'].items()})
PY
done
