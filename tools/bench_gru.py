"""``layers.GRU`` (one projection GEMM + ONE recurrence launch forward, one recurrence launch + two
``dense_backward`` calls backward) against what a user had before it, in one process on one GPU, one JSON line per
(shape, direction, issue mode, pass):

  (B, T, E, U) in {(8192, 10, 32, 32): the sequential-retrieval tutorial's tower at the README batch,
                   (8192, 50, 64, 64)}, x ~ N(0, 1), no mask (the layer holds at most 64 units)

  fused      the layer
  per_step   a Python loop over T of the project's ``Dense`` (input side and recurrent side, 3U wide each) plus torch
             gate arithmetic: the composition the layer replaces
  torch_gru  ``torch.nn.GRU(batch_first=True)`` on the same device (the vendor library's kernels; another gate order
             and weight layout, no Keras mask) -- if it runs there; a failure is recorded, not hidden

Directions: forward (no grad) and forward + backward (loss = sum of the last state).  Issue modes: eager, and replayed
from a captured graph (``torch.cuda.graph``).  Timing: device events around every call, the sides alternated call by
call after warm-up, median and p10 / p90 over the calls; the whole sweep runs ``--passes`` times (default 2) so that the
medians can be compared between passes.  It is a latency chain per 32-row tile: no roofline is claimed.

    python tools/bench_gru.py [--shapes 8192x10x32x32,...] [--iters N] [--passes N] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd.layers import GRU
from recommenders_amd.layers.blocks import Dense

SHAPES = ((8192, 10, 32, 32), (8192, 50, 64, 64))


class PerStep(torch.nn.Module):
  """The per-step composition: 2 ``Dense`` launches + torch gate arithmetic per time step."""

  def __init__(self, E, U):
    super().__init__()
    self.units = U
    self.inp, self.rec = Dense(3 * U), Dense(3 * U)
    self.inp.build(E, torch.device("cuda"))
    self.rec.build(U, torch.device("cuda"))

  def forward(self, x):
    U = self.units
    h = torch.zeros((x.shape[0], U), dtype=torch.float32, device=x.device)
    for t in range(x.shape[1]):
      a, q = self.inp(x[:, t]), self.rec(h)
      z = torch.sigmoid(a[:, :U] + q[:, :U])
      r = torch.sigmoid(a[:, U:2 * U] + q[:, U:2 * U])
      hh = torch.tanh(a[:, 2 * U:] + r * q[:, 2 * U:])
      h = z * h + (1.0 - z) * hh
    return h


def alternate(fns, iters, warmup=2):
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


def captured(fn):
  """`fn` captured after a warm-up on a side stream; returns the replay callable."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(3):
      fn()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    fn()
  return graph.replay


def make_sides(B, T, E, U, with_torch_gru):
  g = torch.Generator(device="cuda").manual_seed(T)
  x = torch.randn((B, T, E), generator=g, device="cuda")
  fused = GRU(U)
  fused.build(E, "cuda")
  modules = {"fused": fused, "per_step": PerStep(E, U)}
  skipped = {}
  if with_torch_gru:
    try:
      net = torch.nn.GRU(E, U, batch_first=True).cuda()
      with torch.no_grad():
        net(x[:64])
      torch.cuda.synchronize()
      modules["torch_gru"] = net
    except Exception as e:          # the vendor route is optional: say why it is absent
      skipped["torch_gru"] = f"torch.nn.GRU did not run: {type(e).__name__}: {str(e)[:200]}"

  def last(name, y):
    return y[1][0] if name == "torch_gru" else y

  def forward(name):
    def fn():
      with torch.no_grad():
        last(name, modules[name](x))
    return fn

  def train(name):
    params = list(modules[name].parameters())

    def fn():
      for p in params:
        p.grad = None
      last(name, modules[name](x)).sum().backward()
    return fn

  return modules, skipped, forward, train


def bench(shape, iters, pass_no, with_torch_gru, graph_torch_gru):
  B, T, E, U = shape
  modules, skipped, forward, train = make_sides(B, T, E, U, with_torch_gru)
  recs = []
  for direction, make in (("forward", forward), ("forward + backward", train)):
    eager = {k: make(k) for k in modules}
    for mode in ("eager", "graph"):
      rec = {"op": "gru", "batch": B, "steps": T, "input_dim": E, "units": U, "direction": direction, "mode": mode,
             "pass": pass_no}
      rec.update(skipped)
      fns = {}
      for k, fn in eager.items():
        if mode == "eager":
          fns[k] = fn
          continue
        if k == "torch_gru" and not graph_torch_gru:
          rec[k] = "not captured (pass --graph-torch-gru)"
          continue
        try:
          fns[k] = captured(fn)
        except Exception as e:
          torch.cuda.synchronize()
          rec[k] = f"capture failed: {type(e).__name__}: {str(e)[:200]}"
      for k, v in alternate(fns, iters).items():
        rec[k] = stats(v)
      for k in ("per_step", "torch_gru"):
        if isinstance(rec.get(k), dict):
          rec[f"fused_over_{k}_ms"] = rec["fused"]["ms_median"] / rec[k]["ms_median"]
      recs.append(rec)
      print(json.dumps(rec), flush=True)
      del fns
  return recs


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default=",".join("x".join(str(v) for v in sh) for sh in SHAPES))
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--passes", type=int, default=2)
  ap.add_argument("--no-torch-gru", action="store_true")
  ap.add_argument("--graph-torch-gru", action="store_true", help="also capture torch.nn.GRU (the vendor route)")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_gru: needs a GPU (no CPU fallback for a measurement)")
  out = None
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
  for p in range(args.passes):
    for sh in args.shapes.split(","):
      for rec in bench(tuple(int(v) for v in sh.split("x")), args.iters, p + 1, not args.no_torch_gru,
                       args.graph_torch_gru):
        if out:                       # line by line: a run that is cut short keeps what it measured
          out.write(json.dumps(rec) + "\n")
          out.flush()
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == "__main__":
  main()
