#!/bin/bash
cd $GRAFT_REPO_ROOT
timeout 1200 python -m pytest tests -m gpu -x -q 2>&1 | tail -4
python bench.py --full --steps 20 --warmup 5 --no-train-step --no-gather --no-scale-workload --no-robustness --no-config-legs --no-cpu-baseline 2>/dev/null | tail -1 | python -c '
import json, sys
d=json.loads(sys.stdin.read())
print("headline ms", d["ms_per_step"], "median", d.get("step_ms_median"), "filter ms", d["roofline"]["avg_launch_ms"])
print({k:v for k,v in d["legs"].items() if k.startswith("streaming")})
'
