"""Kernel split of ONE ScaNN call, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/profile_scann.py --batch 1
    python tools/profile_scann.py --summarize OUT

The first form indexes the clustered 1 M x 64 corpus of tools/bench_scann.py at (1000 leaves, 100 searched,
1000 re-ordered), warms the call up, idles 0.3 s and makes one eager call of --batch queries.  The second reads the
kernel trace under OUT, keeps the dispatches after the last idle gap of more than 0.1 s (the profiled call alone) and
prints one line per kernel: dispatches, total microseconds, share of the call's kernel time, and the call's span from
the first dispatch start to the last dispatch end."""
import argparse
import collections
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(batch: int) -> None:
  import torch
  from recommenders_amd.layers import factorized_top_k as ftk
  sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
  from bench_scann import corpus
  dev = torch.device("cuda", 0)
  g = torch.Generator(device=dev).manual_seed(1)
  cand, queries = corpus(1_000_000, 64, True, g, dev, 8192)
  layer = ftk.ScaNN(k=10, num_leaves=1000, num_leaves_to_search=100, num_reordering_candidates=1000).index(cand)
  q = queries[:batch].contiguous()
  for _ in range(3):
    layer(q)
  torch.cuda.synchronize()
  time.sleep(0.3)
  layer(q)
  torch.cuda.synchronize()


def summarize(out_dir: str) -> None:
  paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
  if not paths:
    raise SystemExit(f"no kernel trace under {out_dir}")
  rows = []
  for path in paths:
    with open(path) as f:
      for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
  rows.sort()
  cut, last_end = 0, rows[0][1]
  for i in range(1, len(rows)):
    if rows[i][0] - last_end > 100_000_000:     # idle for more than 0.1 s before this dispatch
      cut = i
    last_end = max(last_end, rows[i][1])
  call = rows[cut:]
  total = sum(e - s for s, e, _ in call)
  per = collections.defaultdict(lambda: [0, 0])
  for s, e, name in call:
    short = name.split("(")[0]
    per[short][0] += 1
    per[short][1] += e - s
  print(f"dispatches {len(call)}, kernel time {total / 1e3:.1f} us, span {(call[-1][1] - call[0][0]) / 1e3:.1f} us")
  for name, (count, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
    print(f"{ns / 1e3:10.1f} us {100.0 * ns / total:5.1f} %  x{count:<4d} {name}")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=1)
  ap.add_argument("--summarize", default=None)
  args = ap.parse_args()
  if args.summarize:
    summarize(args.summarize)
  else:
    run(args.batch)


if __name__ == "__main__":
  main()
