#!/bin/bash
# FAST iteration: the extraction and pipeline parity tests (every batch plan runs k_fast_pairs),
# then the C2 / C5 bench lines (stage times).  Usage: bash scripts/gpu_fast_iter.sh TAG
set -o pipefail
T=${1:-fast}
O=${ORBX_OUT_DIR:-bench_out}/$T
mkdir -p $O
timeout -k 10 500 python -u -m pytest tests/test_extract_gpu.py tests/test_pipeline_gpu.py -m gpu -q -x \
  --timeout 240 --timeout-method thread > $O/tests.txt 2>&1 || { tail -30 $O/tests.txt; exit 1; }
tail -1 $O/tests.txt
timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-upload > $O/c2.jsonl 2> $O/c2.err || exit 2
timeout -k 10 300 python bench.py --full --config C5 --steps 10 --warmup 2 --no-cpu-baseline --no-upload > $O/c5.jsonl 2> $O/c5.err || exit 3
python - <<PY
import json
for c in ("c2", "c5"):
    d = json.loads(open("$O/%s.jsonl" % c).read())
    st = d["roofline"]["stages_ms_per_step"]
    print(c, d["value"], {k: v for k, v in st.items() if v})
PY
