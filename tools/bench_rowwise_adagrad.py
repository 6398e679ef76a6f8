"""RowWiseAdagrad's sparse update against the fused sparse Adagrad of the same build, on one GPU, one JSON line per shape:

  large   the `sparse_adagrad` shape of bench_legs.py: a 26 M x 128 table, 65536 * 26 uniform ids (the sorted route)
  small   a 3000 x 64 table, 4096 ids (the row scan)

Timing: device events around every call, the two sides alternated call by call in the same process after warm-up,
median and p10 / p90 over the calls.  Bytes are the algorithmic ones, computed from the shapes as bench_legs.py counts
them (n ids, uniq touched rows, width d):

  Adagrad    n d 4 + 4 uniq d 4 + n 8                  gradient rows; table and accumulator rows read and written; ids
  row-wise   n d 4 + 2 uniq d 4 + uniq 8 + n 8         gradient rows; table rows read and written; one float per row
                                                       read and written; ids

and the optimizer state bytes are vocab d 4 against vocab 4.

    python tools/bench_rowwise_adagrad.py [--only large,small] [--iters N] [--out profiles/rowwise_adagrad.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd import optimizers as own
from recommenders_amd.layers import embedding as emb

HBM_PEAK = 8e12

SHAPES = {"large": (26_000_000, 128, 65536 * 26), "small": (3000, 64, 4096)}


def alternate(fns, iters, warmup=3):
  """{name: sorted ms} of the calls of every fn, alternated round by round."""
  for _ in range(warmup):
    for fn in fns.values():
      fn()
  events = {k: [] for k in fns}
  for _ in range(iters):
    for k, fn in fns.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      fn()
      b.record()
      events[k].append((a, b))
  torch.cuda.synchronize()
  return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in events.items()}


def stats(ts):
  return {"ms_median": ts[len(ts) // 2], "ms_p10": ts[len(ts) // 10], "ms_p90": ts[(len(ts) * 9) // 10], "calls": len(ts)}


def bench_shape(name, dev, iters):
  vocab, d, n = SHAPES[name]
  g = torch.Generator(device=dev).manual_seed(0)
  ids = torch.randint(0, vocab, (n,), generator=g, device=dev)
  go = torch.randn((n, d), generator=g, device=dev) * 1e-3
  uniq = int(torch.unique(ids).numel())
  table_a = torch.empty((vocab, d), device=dev).uniform_(-0.05, 0.05)
  acc_a = torch.full_like(table_a, 0.1)
  table_r = torch.nn.Parameter(table_a.clone())
  table_r._tfrs_embedding = True
  opt = own.RowWiseAdagrad([table_r], learning_rate=0.5)

  def rowwise():
    table_r._tfrs_slices.append((ids, go))
    opt.step()

  ts = alternate({"adagrad": lambda: emb.adagrad_sparse_update_(table_a, acc_a, go, ids, 0.5), "rowwise": rowwise}, iters)
  st = {k: stats(v) for k, v in ts.items()}
  nbytes = {"adagrad": n * d * 4 + 4 * uniq * d * 4 + n * 8, "rowwise": n * d * 4 + 2 * uniq * d * 4 + uniq * 8 + n * 8}
  state = {"adagrad": vocab * d * 4, "rowwise": int(opt.state[table_r]["accumulator"].numel()) * 4}
  rec = {"op": "sparse update, uniform ids", "shape": name, "route": "row scan" if emb._use_rowscan(vocab, n, d) else "sorted",
         "vocab": vocab, "dim": d, "rows": n, "unique": uniq}
  for k in ("adagrad", "rowwise"):
    med = st[k]["ms_median"]
    rec[k] = {**st[k], "algorithmic_bytes": nbytes[k], "gbps": nbytes[k] / (med * 1e-3) / 1e9,
              "frac_hbm_peak": nbytes[k] / (med * 1e-3) / HBM_PEAK, "optimizer_state_bytes": state[k]}
  rec["rowwise_over_adagrad_ms"] = st["rowwise"]["ms_median"] / st["adagrad"]["ms_median"]
  rec["rowwise_over_adagrad_bytes"] = nbytes["rowwise"] / nbytes["adagrad"]
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--only", default="large,small")
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_rowwise_adagrad: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  lines = []
  for name in SHAPES:
    if name in args.only.split(","):
      lines.append(bench_shape(name, dev, args.iters))
      print(json.dumps(lines[-1]), flush=True)
      torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for rec in lines:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
  main()
