"""Discretization / Normalization against the torch composition a user writes today, on one GPU, one JSON line per
shape and operation:

  bucketize   Discretization(boundaries)(ts)          vs  torch.bucketize(ts, boundaries_f64, right=True)
  normalize   Normalization(mean, variance)(x)        vs  (x.float() - m) / s
  moments     reset_state + update_state + finalize   vs  torch.var_mean(x.double(), unbiased=False)

Shapes: 8 192 and 1 048 576 int64 unix timestamps with 1000 boundaries (bucketize, normalize with axis=None, moments),
and f32 [65 536, 13] for the per-feature normalisation and moments.

Timing, two ways, the two sides alternated sample by sample in one process after warm-up:
  eager   device events around C back-to-back calls issued to an idle queue, divided by C: launch and host overhead
          included
  graph   the same C calls captured once in a HIP graph, device events around one replay: device time alone
Every call of a sample reads an input of its own and keeps an output of its own, and C is chosen so that one sample
moves at least 512 MiB, twice the 256 MiB cache: the 1 M and [65 536, 13] shapes are read from memory, not from cache.
Medians (p10, p90) over the samples; the whole measurement runs twice (pass 1, pass 2) to show repeatability.

Bytes are algorithmic (input read once, output written once; the moments read only).  For the layer's graph timing the
record states the fraction of the in-process copy ceiling (tfrs_calibrate_copy, the one bench.py reports) -- for the
8 192 shape no such fraction is stated: it is launch-bound.

    python tools/bench_numeric_features.py [--samples N] [--out profiles/numeric_features.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommenders_amd.layers import Discretization, Normalization

SAMPLE_BYTES = 512 << 20
MAX_CALLS = 256


def stats(ts):
  ts = sorted(ts)
  return {"ms_median": ts[len(ts) // 2], "ms_p10": ts[len(ts) // 10], "ms_p90": ts[(len(ts) * 9) // 10], "samples": len(ts)}


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  return a, b


def alternate(fns, calls, samples, warmup=3, drain=False):
  """{name: ms per call} of every fn (each runs ``calls`` calls), alternated sample by sample.  ``drain``: the queue is
  empty when a sample starts, so its events bracket the host's enqueueing too."""
  for _ in range(warmup):
    for fn in fns.values():
      fn()
  events = {k: [] for k in fns}
  for _ in range(samples):
    for k, fn in fns.items():
      if drain:
        torch.cuda.synchronize()
      events[k].append(timed(fn))
  torch.cuda.synchronize()
  return {k: [a.elapsed_time(b) / calls for a, b in v] for k, v in events.items()}


def many(fn, calls):
  keep = [None] * calls                 # every call keeps an output of its own

  def run():
    for c in range(calls):
      keep[c] = fn(c)
  return run


def graphed(fn, calls):
  run = many(fn, calls)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    run()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    run()
  return graph.replay


def compare(op, shape, dtype, layer_fn, torch_fn, bytes_per_call, calls, samples, copy_gbs, roofline):
  eager = alternate({"layer": many(layer_fn, calls), "composition": many(torch_fn, calls)}, calls, samples, drain=True)
  graph = alternate({"layer": graphed(layer_fn, calls), "composition": graphed(torch_fn, calls)}, calls, samples)
  rec = {"op": op, "shape": list(shape), "dtype": dtype, "calls_per_sample": calls,
         "algorithmic_bytes_per_call": bytes_per_call}
  for mode, ts in (("eager", eager), ("graph", graph)):
    rec[mode] = {k: stats(v) for k, v in ts.items()}
    rec[mode]["layer_over_composition"] = rec[mode]["layer"]["ms_median"] / rec[mode]["composition"]["ms_median"]
  gbs = bytes_per_call / (rec["graph"]["layer"]["ms_median"] * 1e-3) / 1e9
  rec["graph"]["layer_gbs"] = gbs
  if roofline:
    rec["measured_copy_gbs"] = copy_gbs
    rec["graph"]["layer_frac_of_copy_ceiling"] = gbs / copy_gbs
  else:
    rec["roofline"] = "none stated: launch-bound at this size"
  return rec


def calls_for(bytes_per_call):
  return int(min(MAX_CALLS, max(8, -(-SAMPLE_BYTES // bytes_per_call))))


def timestamp_records(n, samples, copy_gbs, dev, g):
  boundaries = np.linspace(875_000_000, 893_000_000, 1000).astype(np.float32)
  roofline = n >= 1 << 20
  calls = calls_for(16 * n)
  ts = torch.randint(875_000_000, 893_000_001, (calls, n), generator=g, device=dev)
  buckets = Discretization(bin_boundaries=boundaries, device=dev)
  b64 = buckets.bin_boundaries.double()             # what an all-torch user compares int64 seconds against
  same = float((buckets(ts[0]) == torch.bucketize(ts[0], b64, right=True)).float().mean())
  rec = compare("Discretization.forward vs torch.bucketize(right=True)", (n,), "int64", lambda c: buckets(ts[c]),
                lambda c: torch.bucketize(ts[c], b64, right=True), 16 * n, calls, samples, copy_gbs, roofline)
  rec["boundaries"] = 1000
  rec["share_equal_to_f64_bucketize"] = same        # the f32 rule moves a few timestamps by one bucket
  yield rec

  norm = Normalization(axis=None, device=dev)
  norm.adapt(ts[0])
  m, s = norm.mean.clone(), norm._scale.clone()
  same = float((norm(ts[0]) == (ts[0].float() - m) / s).float().mean())
  rec = compare("Normalization(axis=None).forward vs (x.float() - m) / s", (n,), "int64", lambda c: norm(ts[c]),
                lambda c: (ts[c].float() - m) / s, 12 * n, calls, samples, copy_gbs, roofline)
  rec["share_equal_to_composition"] = same
  yield rec

  def layer_moments(c):
    norm.reset_state()
    norm.update_state(ts[c])
    norm.finalize_state()
    return norm.mean

  yield compare("Normalization reset + update_state + finalize_state vs torch.var_mean(x.double())", (n,), "int64",
                layer_moments, lambda c: torch.var_mean(ts[c].double(), unbiased=False), 8 * n, calls, samples,
                copy_gbs, roofline)


def feature_records(rows, f, samples, copy_gbs, dev, g):
  n = rows * f
  calls = calls_for(8 * n)
  x = torch.randn((calls, rows, f), generator=g, device=dev) * 3 + 1
  norm = Normalization(device=dev)
  norm.adapt(x[0])
  m, s = norm.mean.clone(), norm._scale.clone()
  same = float((norm(x[0]) == (x[0] - m) / s).float().mean())
  rec = compare("Normalization(axis=-1).forward vs (x - m) / s", (rows, f), "float32", lambda c: norm(x[c]),
                lambda c: (x[c] - m) / s, 8 * n, calls, samples, copy_gbs, True)
  rec["share_equal_to_composition"] = same
  yield rec

  def layer_moments(c):
    norm.reset_state()
    norm.update_state(x[c])
    norm.finalize_state()
    return norm.mean

  yield compare("Normalization reset + update_state + finalize_state vs torch.var_mean(x.double(), dim=0)", (rows, f),
                "float32", layer_moments, lambda c: torch.var_mean(x[c].double(), dim=0, unbiased=False), 4 * n, calls,
                samples, copy_gbs, True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--samples", type=int, default=30)
  ap.add_argument("--out", default=os.path.join("profiles", "numeric_features.jsonl"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_numeric_features: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  g = torch.Generator(device=dev).manual_seed(0)
  import bench_legs
  copy_gbs = bench_legs.measure_ceilings(dev)["copy_gbs"]
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "a") as f:
    for pass_no in (1, 2):
      for n in (8_192, 1 << 20):
        for rec in timestamp_records(n, args.samples, copy_gbs, dev, g):
          rec["pass"] = pass_no
          print(json.dumps(rec), flush=True)
          f.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()
      for rec in feature_records(65_536, 13, args.samples, copy_gbs, dev, g):
        rec["pass"] = pass_no
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")
      torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
