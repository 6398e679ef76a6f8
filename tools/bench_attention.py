"""``layers.MultiHeadAttention`` (three projection GEMMs, ONE ``tfrs_attention_fwd`` launch and the output
projection forward; one ``tfrs_attention_bwd`` launch plus ``dense_backward`` calls backward) against what a user had
before it, in one process on one GPU, one JSON line per (shape, direction, issue mode, pass):

  (B, T, H, key_dim) in {(8192, 10, 1, 32): the sequential tower at the README batch, (8192, 50, 2, 32),
                         (2048, 128, 4, 64)}, self-attention over x ~ N(0, 1) [B, T, H key_dim], causal, with a
                         right-padded mask (lengths 1 .. T) on queries and keys

  fused        the layer
  composition  the same projections through the project's ``dense`` (with gradients) and the attention core in torch:
               ``matmul``, ``masked_fill``, ``softmax``, ``matmul`` -- it stores the [B, H, T, T] scores
  sdpa         the same projections and ``torch.nn.functional.scaled_dot_product_attention`` with a boolean mask (rows
               with nothing allowed are given their own position, so that no route computes a NaN) -- if it runs
               there; a failure is recorded, not hidden

Directions: forward (no grad) and forward + backward (loss = sum of the output).  Issue modes: eager, and replayed from
a captured graph (``torch.cuda.graph``).  Only the layer is captured.  The torch sides (batched ``matmul`` /
``scaled_dot_product_attention`` of the vendor libraries) are timed eagerly only, as ``bench_lstm.py`` times
``torch.nn.LSTM``: capturing and replaying them beside the layer faulted on the GPU, so this tool has no
path that does, and their graph rows say "not measured".  Timing: device events around every call, the sides alternated
call by call after warm-up, median and p10 / p90 over the calls; the whole sweep runs ``--passes`` times (default 2) so
that the medians can be compared between passes.  ``peak_bytes`` is ``torch.cuda.max_memory_allocated`` over one eager
forward + backward above what was allocated before it.  It is a latency chain per (b, h): no roofline is claimed.

    python tools/bench_attention.py [--shapes 8192x10x1x32,...] [--iters N] [--passes N] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd.layers import MultiHeadAttention
from recommenders_amd.layers.feature_interaction.dcn import dense_act

SHAPES = ((8192, 10, 1, 32), (8192, 50, 2, 32), (2048, 128, 4, 64))


class TorchCore(torch.nn.Module):
  """The layer's weights and projections, the attention core in torch (``sdpa=False``: the explicit composition)."""

  def __init__(self, layer, sdpa):
    super().__init__()
    self.layer, self.sdpa = layer, sdpa

  def forward(self, x, allow):
    m, (b, t, _) = self.layer, x.shape
    h, dk, dv = m.num_heads, m.key_dim, m.value_dim
    x2 = x.reshape(b * t, -1)
    proj = lambda w, bias, d: dense_act(x2, w.reshape(-1, h * d), bias.reshape(-1), 0).reshape(b, t, h, d).transpose(1, 2)
    q, k, v = proj(m.query_kernel, m.query_bias, dk), proj(m.key_kernel, m.key_bias, dk), proj(m.value_kernel,
                                                                                              m.value_bias, dv)
    if self.sdpa:
      o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=allow[:, None])
    else:
      s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(dk))
      o = torch.matmul(torch.softmax(s.masked_fill(~allow[:, None], float("-inf")), dim=-1), v)
    o = o.transpose(1, 2).reshape(b * t, h * dv)
    return dense_act(o, m.output_kernel.reshape(h * dv, -1), m.output_bias, 0).reshape(b, t, -1)


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


def make_sides(B, T, H, dk):
  g = torch.Generator(device="cuda").manual_seed(T)
  x = torch.randn((B, T, H * dk), generator=g, device="cuda")
  lengths = 1 + torch.arange(B, device="cuda") % T
  live = torch.arange(T, device="cuda")[None, :] < lengths[:, None]                      # right-padded
  allow = live[:, :, None] & live[:, None, :] & torch.ones((T, T), dtype=torch.bool, device="cuda").tril()[None]
  allow = allow | (torch.eye(T, dtype=torch.bool, device="cuda")[None] & ~live[:, :, None])   # padded rows: no NaN
  layer = MultiHeadAttention(H, dk)
  layer.build(H * dk, device="cuda")
  modules = {"fused": layer, "composition": TorchCore(layer, False), "sdpa": TorchCore(layer, True)}
  skipped = {}
  try:
    with torch.no_grad():
      modules["sdpa"](x[:64], allow[:64])
    torch.cuda.synchronize()
  except Exception as e:          # the vendor route is optional: say why it is absent
    del modules["sdpa"]
    skipped["sdpa"] = f"scaled_dot_product_attention did not run: {type(e).__name__}: {str(e)[:200]}"

  def call(name):
    if name == "fused":
      return layer(x, x, query_mask=live, value_mask=live, use_causal_mask=True)
    return modules[name](x, allow)

  def forward(name):
    def fn():
      with torch.no_grad():
        call(name)
    return fn

  def train(name):
    params = list(layer.parameters())

    def fn():
      for p in params:
        p.grad = None
      call(name).sum().backward()
    return fn

  return modules, skipped, forward, train


def peak_bytes(fn):
  fn()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  fn()
  torch.cuda.synchronize()
  return torch.cuda.max_memory_allocated() - before


def bench(shape, iters, pass_no):
  B, T, H, dk = shape
  modules, skipped, forward, train = make_sides(B, T, H, dk)
  recs = []
  for direction, make in (("forward", forward), ("forward + backward", train)):
    eager = {k: make(k) for k in modules}
    for mode in ("eager", "graph"):
      rec = {"op": "attention", "batch": B, "steps": T, "heads": H, "key_dim": dk, "direction": direction,
             "mode": mode, "pass": pass_no}
      rec.update(skipped)
      fns = {}
      for k, fn in eager.items():
        if mode == "eager":
          fns[k] = fn
          continue
        if k != "fused":
          rec[k] = "not measured"
          continue
        fns[k] = captured(fn)
      for k, v in alternate(fns, iters).items():
        rec[k] = stats(v)
      for k in ("composition", "sdpa"):
        if isinstance(rec.get(k), dict):
          rec[f"fused_over_{k}_ms"] = rec["fused"]["ms_median"] / rec[k]["ms_median"]
      del fns
      if direction != "forward" and mode == "eager":
        rec["peak_bytes"] = {k: peak_bytes(fn) for k, fn in eager.items()}
      recs.append(rec)
      print(json.dumps(rec), flush=True)
  return recs


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default=",".join("x".join(str(v) for v in sh) for sh in SHAPES))
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--passes", type=int, default=2)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_attention: needs a GPU (no CPU fallback for a measurement)")
  out = None
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
  for p in range(args.passes):
    for sh in args.shapes.split(","):
      for rec in bench(tuple(int(v) for v in sh.split("x")), args.iters, p + 1):
        if out:                       # line by line: a run that is cut short keeps what it measured
          out.write(json.dumps(rec) + "\n")
          out.flush()
      torch.cuda.empty_cache()
  if out:
    out.close()


if __name__ == "__main__":
  main()
