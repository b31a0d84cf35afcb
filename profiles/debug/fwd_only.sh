#!/bin/bash
# forward-only entry: tests + the inference probe of bench.py --full:  bash profiles/debug/fwd_only.sh <out dir>
[ -n "$1" ] || { echo "usage: fwd_only.sh <out dir>" >&2; exit 2; }
O=$(mkdir -p "$1" && cd "$1" && pwd)
cd $(dirname $0)/../..
timeout 900 python -m pytest tests/test_gpu_step_plan.py tests/test_gpu_predict.py tests/test_gpu_train_entry.py -x -q -m gpu 2>&1 | tail -15 > $O/fwd_tests.log
timeout 900 python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline --no-cfg3 --no-split-probe > $O/fwd_bench.json 2> $O/fwd_bench.err
python - $O/fwd_bench.json <<'PY' > $O/fwd_inf.txt
import json, sys
l=[x for x in open(sys.argv[1]) if x.startswith('{')][-1]
d=json.loads(l)
print(d['value'], d['ms_per_step'])
for k,v in d.get('inference',{}).items(): print(k, v)
PY
