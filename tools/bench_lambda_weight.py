"""What the lambda weights cost: forward + backward of ``PairwiseLogisticLoss`` in one process on one
GPU, one JSON line per list length:

  B = 8192 lists of L in {5, 32, 128, 512} items, labels in {-1, 0, .., 4} (one position in six padded), scores N(0, 2)

alternated call by call between
  unweighted   the fused loss without ``lambda_weight``
  ndcg         the fused loss with ``NDCGLambdaWeight()`` (smooth_fraction 0: the kernels without the u table)
  ndcg_smooth  the fused loss with ``NDCGLambdaWeight(smooth_fraction=0.25)``
  torch        a torch composition of the weighted formulas (smooth_fraction 0.25): two stable sorts for the ranks and
               IDCG, then ``[B, L, L]`` tensors for the weights and the pair terms.  Skipped, with a message in the
               line, where its temporaries (estimated as sixteen ``[B, L, L]`` float32 tensors) exceed
               ``--torch-max-gib`` or the allocation fails.

Timing: device events around every call (loss forward and ``backward()``), after warm-up, median and p10 / p90 over the
calls.  ``agreement`` is (fused ndcg_smooth loss, torch loss, largest gradient difference / largest gradient).

    python tools/bench_lambda_weight.py [--lengths 5,32] [--kind pairwise_hinge] [--iters N] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd import losses

BATCH = 8192
LENGTHS = (5, 32, 128, 512)
FUSED = {"pairwise_logistic": losses.PairwiseLogisticLoss, "pairwise_hinge": losses.PairwiseHingeLoss}
NEG_INF = float("-inf")


def torch_lambda_pairwise(y, s, hinge, mu):
  """Per-list NDCG-weighted pairwise loss [B]; the weights are detached (constants of the backward)."""
  B, L = y.shape
  valid = y >= 0
  with torch.no_grad():
    pos = torch.arange(L, device=y.device, dtype=torch.float32)
    d0 = 1.0 / torch.log2(pos + 2.0)                                     # d0[r - 1] = D0(r)
    order = torch.sort(torch.where(valid, s, torch.full_like(s, NEG_INF)), dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(L, device=y.device).expand(B, L))      # 0-based
    gain = torch.where(valid, torch.exp2(y) - 1.0, torch.zeros_like(y))
    ideal = torch.sort(torch.where(valid, y, torch.full_like(y, NEG_INF)), dim=1, descending=True, stable=True).indices
    idcg = (torch.gather(gain, 1, ideal) * d0).sum(dim=1, keepdim=True)
    g = torch.where(idcg > 0, gain / torch.where(idcg > 0, idcg, torch.ones_like(idcg)), torch.zeros_like(gain))
    disc = d0[rank]
    delta = (rank[:, :, None] - rank[:, None, :]).abs()
    u = (d0[(delta - 1).clamp(min=0)] - d0[delta.clamp(max=L - 1)]).abs()
    w = (g[:, :, None] - g[:, None, :]).abs() * ((1.0 - mu) * (disc[:, :, None] - disc[:, None, :]).abs() + mu * u)
    pair = valid[:, :, None] & valid[:, None, :] & (y[:, :, None] > y[:, None, :])
    w = torch.where(pair, w, torch.zeros_like(w))
  x = s[:, :, None] - s[:, None, :]
  phi = torch.clamp(1.0 - x, min=0.0) if hinge else torch.clamp(-x, min=0.0) + torch.log1p(torch.exp(-x.abs()))
  return (w * torch.where(pair, phi, torch.zeros_like(phi))).sum(dim=(1, 2))


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


def bench(kind, L, dev, iters, torch_max_gib, mu=0.25):
  g = torch.Generator(device=dev).manual_seed(L)
  y = torch.randint(-1, 5, (BATCH, L), generator=g, device=dev).to(torch.float32)
  s = (torch.randn((BATCH, L), generator=g, device=dev) * 2.0).requires_grad_(True)
  rec = {"op": kind, "batch": BATCH, "list_len": L, "direction": "forward + backward", "smooth_fraction": mu}
  out = {}

  def fused(name, loss_fn):
    def call():
      s.grad = None
      out[name] = loss_fn(y, s)
      out[name].backward()
      out[name + "_grad"] = s.grad
    return call

  def composed():
    s.grad = None
    out["torch"] = torch_lambda_pairwise(y, s, kind == "pairwise_hinge", mu).sum() / BATCH
    out["torch"].backward()
    out["torch_grad"] = s.grad

  fns = {"unweighted": fused("unweighted", FUSED[kind]()),
         "ndcg": fused("ndcg", FUSED[kind](lambda_weight=losses.NDCGLambdaWeight())),
         "ndcg_smooth": fused("ndcg_smooth", FUSED[kind](lambda_weight=losses.NDCGLambdaWeight(smooth_fraction=mu)))}
  torch_bytes = 16 * BATCH * L * L * 4
  skip = None if torch_bytes <= torch_max_gib * 2 ** 30 else (
      f"torch side skipped: about {torch_bytes / 2 ** 30:.0f} GiB of [B, L, L] temporaries (limit {torch_max_gib} GiB)")
  if skip is None:
    try:
      composed()
      torch.cuda.synchronize()
      fns["torch"] = composed
    except torch.cuda.OutOfMemoryError:
      skip = "torch side skipped: its temporaries did not fit in device memory"
      out.pop("torch", None)
      s.grad = None
      torch.cuda.empty_cache()
  ts = alternate(fns, iters)
  for k, v in ts.items():
    rec[k] = stats(v)
  base = rec["unweighted"]["ms_median"]
  rec["ndcg_over_unweighted_ms"] = rec["ndcg"]["ms_median"] / base
  rec["ndcg_smooth_over_unweighted_ms"] = rec["ndcg_smooth"]["ms_median"] / base
  if "torch" in ts:
    tg = torch.nan_to_num(out["torch_grad"], nan=0.0)
    rec["ndcg_smooth_over_torch_ms"] = rec["ndcg_smooth"]["ms_median"] / rec["torch"]["ms_median"]
    rec["agreement"] = (float(out["ndcg_smooth"]), float(out["torch"]),
                        float((out["ndcg_smooth_grad"] - tg).abs().max()) / max(float(tg.abs().max()), 1e-30))
  else:
    rec["torch"] = skip
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--kind", default="pairwise_logistic", choices=sorted(FUSED))
  ap.add_argument("--lengths", default=",".join(str(l) for l in LENGTHS))
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--torch-max-gib", type=float, default=160.0)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_lambda_weight: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  lines = []
  for L in (int(v) for v in args.lengths.split(",")):
    lines.append(bench(args.kind, L, dev, args.iters, args.torch_max_gib))
    print(json.dumps(lines[-1]), flush=True)
    torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for rec in lines:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
  main()
