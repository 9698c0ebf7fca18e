#!/bin/bash
# The full bench line (--full: its parity checks) with the library's pools poisoned (LEGKILO_POISON_POOLS=1).   usage: tools/gpu_poison_bench.sh <out dir>
OUT=${1:?usage: tools/gpu_poison_bench.sh <out dir>}/poison
mkdir -p $OUT
LEGKILO_POISON_POOLS=1 timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc $?"
python - $OUT/bench.json <<'PY'
import json, sys
j=json.load(open(sys.argv[1]))
print(j['value'], j['parity_check'].get('ok'), {k:(v.get('counts_equal'),v.get('n')) for k,v in j['parity_check'].items() if isinstance(v,dict)}, j['parity_check'].get('counts_equal'), j.get('warnings'))
PY
