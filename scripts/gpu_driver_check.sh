#!/bin/bash
# What the driver runs at round end, minus the test suite: smoke(), then the default bench line
# (its PMC fields must bind to profiles/<round>_pmc).  Usage: bash scripts/gpu_driver_check.sh TAG
set -o pipefail
T=${1:-drv}
O=${ORBX_OUT_DIR:-bench_out}/$T
mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.txt 2>&1 || { tail -20 $O/smoke.txt; exit 1; }
tail -1 $O/smoke.txt
timeout -k 10 600 python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 2; }
python - <<PY
import json
d = json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
r = d["roofline"]
print(d["value"], r["kernel"], r["frac"], r.get("traffic"), r["issue_roofline"].get("frac"), r.get("traffic_note", "")[:120])
PY
