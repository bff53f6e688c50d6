#!/bin/bash
# Full iteration: the whole -m gpu suite, then the C2 / C5 bench lines and the one-thread
# drop-in line.  Usage: bash scripts/gpu_all_iter.sh TAG
set -o pipefail
T=${1:-iter}
O=${ORBX_OUT_DIR:-bench_out}/$T
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread \
  > $O/tests.txt 2>&1 || { tail -30 $O/tests.txt; exit 1; }
tail -1 $O/tests.txt
timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-upload > $O/c2.jsonl 2> $O/c2.err || exit 2
timeout -k 10 200 python bench.py --dropin --threads 1 --dropin-frames 400 > $O/d1.json 2> $O/d1.err || exit 4
timeout -k 10 200 python bench.py --dropin --threads 8 --dropin-frames 300 > $O/d8.json 2> $O/d8.err || exit 5
python - <<PY
import json
d = json.loads(open("$O/c2.jsonl").read())
st = d["roofline"]["stages_ms_per_step"]
print("c2", d["value"], {k: v for k, v in st.items() if v})
for t in ("d1", "d8"):
    d = json.loads(open("$O/%s.json" % t).read())
    print("dropin", t, d["value"], {k: v for k, v in d["dropin"].items() if "median" in k})
PY
