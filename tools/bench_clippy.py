"""ClippyAdagrad's kernels against what they stand beside, on one GPU, one JSON line per measurement:

  dense    tfrs_clippy_dense_multi vs tfrs_adagrad_dense_multi on the dense parameter set of the configs[3] DCN-v2 model
           (bottom MLP 13-512-256-128, three full-rank Cross layers of width 3456, top MLP 3584-1024-512-1), and vs the
           same formula in torch ops on the same GPU tensors (what a user would write without the kernels)
  sparse   tfrs_clippy_sparse vs the fused sparse Adagrad on the 26 M x 128 table of tools/bench_scatter.py, uniform ids
  sparse_zipf  the same with Zipf ids: one id occurs ~10^5 times; ClippyAdagrad sums such a run as one sequential chain
  step     the configs[3] DCN-v2 train step with CompositeOptimizer([ClippyAdagrad(tables), Adagrad(dense)]) vs Adagrad

Timing: device events around every call, the two sides of a comparison alternated call by call in the same process
after warm-up, median and p10 / p90 over the calls.  Bytes are the algorithmic ones, computed from the shapes.

    python tools/bench_clippy.py [--only dense,sparse,sparse_zipf,step] [--iters N] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import recommenders_amd as tfrs
from recommenders_amd import optimizers as own
from recommenders_amd.experimental.optimizers import ClippyAdagrad, CompositeOptimizer
from recommenders_amd.experimental.optimizers.clippy_adagrad import clippy_update
from recommenders_amd.layers import embedding as emb

HBM_PEAK = 8e12


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


def dcn_dense_shapes():
  width, dim = 27 * 128, 128
  shapes = []
  for a, b in ((13, 512), (512, 256), (256, dim)):                      # bottom MLP
    shapes += [(a, b), (b,)]
  shapes += [(width, width), (width,)] * 3                              # Cross kernels and biases
  for a, b in ((dim + width, 1024), (1024, 512), (512, 1)):             # top MLP
    shapes += [(a, b), (b,)]
  return shapes


def bench_dense(dev, iters, emit):
  g = torch.Generator(device=dev).manual_seed(1)
  shapes = dcn_dense_shapes()
  mk = lambda: [torch.nn.Parameter(torch.empty(s, device=dev).uniform_(-0.05, 0.05, generator=g)) for s in shapes]
  grads = [torch.randn(s, generator=g, device=dev) * 1e-3 for s in shapes]
  elements = sum(t.numel() for t in grads)
  sides = {}
  for name, opt_of in (("adagrad", lambda p: own.Adagrad(p, learning_rate=0.01)),
                       ("clippy", lambda p: ClippyAdagrad(p, learning_rate=0.01, export_clipping_factors=True))):
    params = mk()
    for p, gr in zip(params, grads):
      p.grad = gr
    sides[name] = opt_of(params)
  # the same formula in torch ops on the same kind of tensors: ClippyAdagrad's own fallback route, forced
  params = mk()
  group = sides["clippy"].param_groups[0]
  accs = [torch.full_like(p, 0.1) for p in params]
  factors = torch.ones((len(params),), device=dev)

  @torch.no_grad()
  def torch_ops():
    for i, (p, a, gr) in enumerate(zip(params, accs, grads)):
      w, a2, f = clippy_update(p.data, a, gr, group)
      p.data.copy_(w)
      a.copy_(a2)
      factors[i].copy_(f)

  ts = alternate({"adagrad": sides["adagrad"].step, "clippy": sides["clippy"].step, "torch_ops": torch_ops}, iters)
  med = {k: stats(v)["ms_median"] for k, v in ts.items()}
  for name, per_element in (("adagrad", 20), ("clippy", 32)):
    nbytes = per_element * elements
    emit({"op": "dense " + name, "tensors": len(shapes), "elements": elements, **stats(ts[name]),
          "algorithmic_bytes": nbytes, "gbps": nbytes / (med[name] * 1e-3) / 1e9,
          "frac_hbm_peak": nbytes / (med[name] * 1e-3) / HBM_PEAK})
  emit({"op": "dense clippy formula in torch ops", "tensors": len(shapes), "elements": elements, **stats(ts["torch_ops"])})
  emit({"op": "dense ratios", "clippy_over_adagrad": med["clippy"] / med["adagrad"], "byte_model": 32 / 20,
        "torch_ops_over_clippy": med["torch_ops"] / med["clippy"],
        "factors_below_one": int((sides["clippy"]._factors < 1).sum())})
  if not med["clippy"] < med["torch_ops"]:
    raise SystemExit("bench_clippy: the kernels (%.3f ms) are not faster than the torch-op formula (%.3f ms)"
                     % (med["clippy"], med["torch_ops"]))


def zipf_ids(n, vocab, exponent, g, dev):
  """n ids of a Zipf law (rank r with weight r^-exponent), the ranks scattered over [0, vocab) by an affine bijection."""
  cdf = torch.cumsum(torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** -exponent, 0)
  ranks = torch.searchsorted(cdf, torch.rand((n,), generator=g, device=dev, dtype=torch.float64) * cdf[-1]).clamp_(max=vocab - 1)
  return (ranks * 7_654_321 + 12345) % vocab          # (7 654 321 is odd and not a multiple of 5 or 13: coprime to 26 M)


def bench_sparse(dev, iters, emit, zipf=False):
  """Uniform ids (every run of equal ids is short), or Zipf ids with exponent 1.05: the hottest id then occurs ~10^5
  times, which the sparse Adagrad sums in parallel pieces and ClippyAdagrad as ONE occurrence-order chain per column
  group, in both passes -- the price of a factor that is exact against the sequential sum."""
  g = torch.Generator(device=dev).manual_seed(0)
  vocab, d, n = 26_000_000, 128, 65536 * 26
  ids = zipf_ids(n, vocab, 1.05, g, dev) if zipf else torch.randint(0, vocab, (n,), generator=g, device=dev)
  kind = "Zipf(1.05) ids, longest run %d" % int(torch.bincount(ids).max()) if zipf else "uniform ids"
  go = torch.randn((n, d), generator=g, device=dev) * 1e-3
  uniq = int(torch.unique(ids).numel())
  table_a = torch.empty((vocab, d), device=dev).uniform_(-0.05, 0.05)
  acc_a = torch.full_like(table_a, 0.1)
  table_c = torch.nn.Parameter(table_a.clone())
  table_c._tfrs_embedding = True
  opt = ClippyAdagrad([table_c], learning_rate=0.5, export_clipping_factors=True)

  def clippy():
    table_c._tfrs_slices.append((ids, go))
    opt.step()

  ts = alternate({"adagrad": lambda: emb.adagrad_sparse_update_(table_a, acc_a, go, ids, 0.5), "clippy": clippy}, iters)
  med = {k: stats(v)["ms_median"] for k, v in ts.items()}
  rows = uniq * d * 4
  model = {"adagrad": n * d * 4 + 4 * rows + n * 8,          # gradient rows + table / accumulator rows read and written + ids
           "clippy": 2 * n * d * 4 + 6 * rows + n * 8}        # ... gradient rows and table / accumulator rows read twice
  for name in ("adagrad", "clippy"):
    emit({"op": "sparse " + name + " (radix sort + segmented update), " + kind, "rows": n, "unique": uniq, "dim": d, "vocab": vocab,
          **stats(ts[name]), "algorithmic_bytes": model[name], "gbps": model[name] / (med[name] * 1e-3) / 1e9,
          "frac_hbm_peak": model[name] / (med[name] * 1e-3) / HBM_PEAK})
  emit({"op": "sparse ratios, " + kind, "clippy_over_adagrad": med["clippy"] / med["adagrad"],
        "byte_model": model["clippy"] / model["adagrad"], "factor": float(opt.clipping_factors[0])})


def bench_step(dev, iters, emit):
  from recommenders_amd.experimental.models import ranking as rk
  n_tables, vocab, dim, batch = 26, 1_000_000, 128, 65536
  g = torch.Generator(device=dev).manual_seed(34)
  feats = {"dense_features": torch.rand((batch, 13), generator=g, device=dev),
           "sparse_features": {str(i): torch.randint(0, vocab, (batch,), generator=g, device=dev) for i in range(n_tables)}}
  labels = torch.randint(0, 2, (batch,), generator=g, device=dev)

  def build(kind):
    torch.manual_seed(7)
    model = rk.Ranking(rk.EmbeddingDict({str(i): vocab for i in range(n_tables)}, dim),
                       bottom_stack=tfrs.layers.blocks.MLP(units=[512, 256, dim], final_activation="relu"),
                       feature_interaction=rk.ConcatCross(num_layers=3),
                       top_stack=tfrs.layers.blocks.MLP(units=[1024, 512, 1], final_activation="sigmoid"),
                       task=tfrs.tasks.Ranking(loss=tfrs.losses.BinaryCrossentropy(reduction="none")))
    with torch.no_grad():
      model(feats)
    if kind == "adagrad":
      model.compile(optimizer=own.Adagrad(model.parameters(), learning_rate=0.01))
    else:
      tables = [p for p in model.parameters() if getattr(p, "_tfrs_embedding", False)]
      dense = [p for p in model.parameters() if not getattr(p, "_tfrs_embedding", False)]
      model.compile(optimizer=CompositeOptimizer([(ClippyAdagrad(tables, learning_rate=0.01), lambda: tables),
                                                  (own.Adagrad(dense, learning_rate=0.01), lambda: dense)]))
    return model

  models = {"adagrad": build("adagrad"), "composite": build("composite")}
  ts = alternate({k: (lambda m=m: m.train_step((feats, labels))) for k, m in models.items()}, iters, warmup=2)
  med = {k: stats(v)["ms_median"] for k, v in ts.items()}
  for k in models:
    emit({"op": "dcn_v2 train step, " + ("Adagrad" if k == "adagrad" else "CompositeOptimizer(ClippyAdagrad tables, Adagrad dense)"),
          "batch": batch, **stats(ts[k]), "examples_per_s": batch / (med[k] * 1e-3)})
  emit({"op": "dcn_v2 step ratio", "composite_over_adagrad": med["composite"] / med["adagrad"]})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--only", default="dense,sparse,sparse_zipf,step")
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_clippy: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  lines = []

  def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)

  for name, fn in (("dense", bench_dense), ("sparse", bench_sparse),
                   ("sparse_zipf", lambda dev, iters, emit: bench_sparse(dev, max(5, iters // 3), emit, zipf=True)),
                   ("step", bench_step)):
    if name in args.only.split(","):
      fn(dev, args.iters if name != "step" else max(5, args.iters // 3), emit)
      torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for rec in lines:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
  main()
