"""LayerNormalization against the torch composition a user writes today, on one GPU, one JSON line per shape and
operation:

  forward            layer(x)                                   vs  F.layer_norm(x, (D,), gamma, beta, eps)
  forward_backward   layer(x) and its gradients of x, gamma,    vs  the same through F.layer_norm
                     beta for a given dy
  fused_add          layer(x, residual=r, return_sum=True)      vs  s = x + r; F.layer_norm(s, ...)

Shapes [N, D]: (81 920, 32), (409 600, 64), (262 144, 256), (65 536, 1024) and (8 192, 4096).

Timing as tools/bench_numeric_features.py does it (its helpers are used): both sides alternated sample by sample in one
process after warm-up; `eager` is device events around C back-to-back calls issued to an idle queue, divided by C;
`graph` is the LAYER ALONE, the same C calls captured once and replayed (the torch side is not captured).  Every call
of a sample reads inputs of its own and keeps outputs of its own, and C is chosen so that a sample moves at least
512 MiB.  Medians (p10, p90); the whole measurement runs twice (pass 1, pass 2).

Bytes are algorithmic, in row images of 4 N D bytes: forward 2 (read x, write y), forward_backward 5 (+ read x and dy,
write dx; mean / rstd and the parameter slabs are not counted), fused_add 4 (read x and r, write s and y).  The record
states TB/s and the fraction of the in-process copy ceiling (bench_legs.measure_ceilings) for the eager and the graph
timing of the layer.

    python tools/bench_layer_norm.py [--samples N] [--out profiles/layer_norm.jsonl]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from bench_numeric_features import alternate, calls_for, graphed, many, stats
from recommenders_amd.layers import LayerNormalization

SHAPES = ((8192 * 10, 32), (8192 * 50, 64), (2048 * 128, 256), (65536, 1024), (8192, 4096))
EPSILON = 1e-3


def records(n, d, samples, copy_gbs, dev, g):
  image = 4 * n * d
  calls = calls_for(2 * image)
  layer = LayerNormalization(epsilon=EPSILON, device=dev)
  layer.build(d, dev)
  with torch.no_grad():
    layer.gamma.copy_(torch.randn(d, generator=g, device=dev) * 0.5 + 1.0)
    layer.beta.copy_(torch.randn(d, generator=g, device=dev) * 0.25)
  x = torch.randn((calls, n, d), generator=g, device=dev)
  r = torch.randn((calls, n, d), generator=g, device=dev)
  dy = torch.randn((n, d), generator=g, device=dev)
  xg = [x[c].clone().requires_grad_(True) for c in range(calls)]          # a leaf per call
  params = [layer.gamma, layer.beta]
  torch_ln = lambda t: F.layer_norm(t, (d,), layer.gamma, layer.beta, EPSILON)

  def no_grad(fn):
    def run(c):
      with torch.no_grad():
        return fn(c)
    return run

  def torch_fused(c):
    s = x[c] + r[c]
    return torch_ln(s), s

  sides = {
      "forward": (2, no_grad(lambda c: layer(x[c])), no_grad(lambda c: torch_ln(x[c]))),
      "forward_backward": (5, lambda c: torch.autograd.grad(layer(xg[c]), [xg[c]] + params, dy),
                           lambda c: torch.autograd.grad(torch_ln(xg[c]), [xg[c]] + params, dy)),
      "fused_add": (4, no_grad(lambda c: layer(x[c], residual=r[c], return_sum=True)), no_grad(torch_fused)),
  }
  for op, (images, layer_fn, torch_fn) in sides.items():
    eager = alternate({"layer": many(layer_fn, calls), "torch": many(torch_fn, calls)}, calls, samples, drain=True)
    graph = alternate({"layer": graphed(layer_fn, calls)}, calls, samples)
    rec = {"op": op, "shape": [n, d], "calls_per_sample": calls, "algorithmic_bytes_per_call": images * image,
           "measured_copy_gbs": copy_gbs, "eager": {k: stats(v) for k, v in eager.items()},
           "graph": {"layer": stats(graph["layer"])}}
    rec["eager"]["layer_over_torch"] = rec["eager"]["layer"]["ms_median"] / rec["eager"]["torch"]["ms_median"]
    for mode in ("eager", "graph"):
      tbs = images * image / (rec[mode]["layer"]["ms_median"] * 1e-3) / 1e12
      rec[mode]["layer_tbs"] = tbs
      rec[mode]["layer_frac_of_copy_ceiling"] = tbs * 1e3 / copy_gbs
    yield rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--samples", type=int, default=20)
  ap.add_argument("--out", default=os.path.join("profiles", "layer_norm.jsonl"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_layer_norm: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  g = torch.Generator(device=dev).manual_seed(0)
  import bench_legs
  copy_gbs = bench_legs.measure_ceilings(dev)["copy_gbs"]
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "a") as f:
    for pass_no in (1, 2):
      for n, d in SHAPES:
        for rec in records(n, d, args.samples, copy_gbs, dev, g):
          rec["pass"] = pass_no
          print(json.dumps(rec), flush=True)
          f.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
