#!/bin/bash
# ab.sh <workload> [env assignment for the B run] -- GPU box: one bench line per variant (value M frames/s, kernel, kernel ms)
w=${1:-imbe_mixed}; shift
cd "$(dirname "$0")/.."
export T=$(mktemp -d); trap 'rm -rf "$T"' EXIT   # the two bench lines, read back below
python bench.py --workload $w --no-cpu-baseline --no-extras > $T/ab_a.log 2>&1
env "$@" python bench.py --workload $w --no-cpu-baseline --no-extras > $T/ab_b.log 2>&1
python - <<'PY'
import json, os
for f in ("ab_a.log", "ab_b.log"):
    try:
        d = json.loads(open(os.path.join(os.environ["T"], f)).read().strip().splitlines()[-1])
        print(f, round(d["value"] / 1e6, 1), d["roofline"]["kernel"], round(d["roofline"]["kernel_ms"], 4))
    except Exception as e:
        print(f, "FAILED", e, open(os.path.join(os.environ["T"], f)).read()[-400:])
PY
