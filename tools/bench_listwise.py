"""The fused listwise losses (forward + backward) and NDCGMetric against a torch composition of the same formulas
(DESIGN 4.24), in one process on one GPU, one JSON line per (op, list length):

  B = 8192 lists of L in {5, 32, 128, 512} items, labels in {-1, 0, .., 4} (one position in six padded), scores N(0, 2)

The torch side is what a user could write without the kernels: a masked logsumexp for the softmax loss, a
``[B, L, L]`` difference tensor for the pairwise losses (several temporaries of that size live through the backward),
a stable sort + ``logcumsumexp`` for ListMLE, two sorts for NDCG.  Where its temporaries (estimated as ten ``[B, L, L]``
float32 tensors for the pairwise losses) exceed ``--torch-max-gib``, or the allocation fails, the torch side is skipped
and the line says so.

Timing: device events around every call (loss forward, ``backward()`` included; for the metric one ``update_state``),
the two sides alternated call by call after warm-up, median and p10 / p90 over the calls.  ``pair_rate`` is the number
of (i, j) position pairs a pairwise loss walks (B L L, forward and backward each) over the fused median.

    python tools/bench_listwise.py [--only softmax,pairwise_logistic,...] [--lengths 5,32] [--iters N] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd import losses, metrics

BATCH = 8192
LENGTHS = (5, 32, 128, 512)
OPS = ("softmax", "pairwise_logistic", "pairwise_hinge", "list_mle", "ndcg")
FUSED = {"softmax": losses.SoftmaxLoss, "pairwise_logistic": losses.PairwiseLogisticLoss,
         "pairwise_hinge": losses.PairwiseHingeLoss, "list_mle": losses.ListMLELoss}
NEG_INF = float("-inf")


# ---- the torch composition (per-list values [B]) -----------------------------------------------------------------------
def torch_softmax(y, s):
  valid = y >= 0
  lse = torch.logsumexp(torch.where(valid, s, torch.full_like(s, NEG_INF)), dim=1, keepdim=True)
  return torch.where(valid, y * (lse - s), torch.zeros_like(s)).sum(dim=1)


def torch_pairwise(y, s, hinge):
  valid = y >= 0
  x = s[:, :, None] - s[:, None, :]
  pair = valid[:, :, None] & valid[:, None, :] & (y[:, :, None] > y[:, None, :])
  phi = torch.clamp(1.0 - x, min=0.0) if hinge else torch.clamp(-x, min=0.0) + torch.log1p(torch.exp(-x.abs()))
  return torch.where(pair, phi, torch.zeros_like(phi)).sum(dim=(1, 2))


def torch_list_mle(y, s):
  valid = y >= 0
  order = torch.sort(torch.where(valid, y, torch.full_like(y, NEG_INF)), dim=1, descending=True, stable=True).indices
  ss = torch.gather(torch.where(valid, s, torch.full_like(s, NEG_INF)), 1, order)      # invalid items last, at -inf
  ok = torch.gather(valid, 1, order)
  lse = torch.logcumsumexp(ss.flip(1), dim=1).flip(1)
  return torch.where(ok, lse - torch.where(ok, ss, torch.zeros_like(ss)), torch.zeros_like(ss)).sum(dim=1)


def torch_ndcg(y, s, topn):
  valid = y >= 0
  disc = 1.0 / torch.log2(torch.arange(y.shape[1], device=y.device, dtype=torch.float32) + 2.0)
  disc = torch.where(torch.arange(y.shape[1], device=y.device) < topn, disc, torch.zeros_like(disc))
  gain = torch.where(valid, torch.exp2(y) - 1.0, torch.zeros_like(y))

  def dcg(keys):
    order = torch.sort(torch.where(valid, keys, torch.full_like(keys, NEG_INF)), dim=1, descending=True, stable=True).indices
    return (torch.gather(gain, 1, order) * disc).sum(dim=1)

  d, i = dcg(s), dcg(y)
  counted = i > 0
  return torch.where(counted, d / torch.where(counted, i, torch.ones_like(i)), torch.zeros_like(d)), counted


TORCH = {"softmax": torch_softmax, "pairwise_logistic": lambda y, s: torch_pairwise(y, s, False),
         "pairwise_hinge": lambda y, s: torch_pairwise(y, s, True), "list_mle": torch_list_mle}


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


def bench(op, L, dev, iters, torch_max_gib):
  g = torch.Generator(device=dev).manual_seed(L)
  y = torch.randint(-1, 5, (BATCH, L), generator=g, device=dev).to(torch.float32)
  s = (torch.randn((BATCH, L), generator=g, device=dev) * 2.0).requires_grad_(True)
  rec = {"op": op, "batch": BATCH, "list_len": L, "direction": "update_state" if op == "ndcg" else "forward + backward"}
  torch_bytes = 10 * BATCH * L * L * 4 if op.startswith("pairwise") else 12 * BATCH * L * 4
  skip = None if torch_bytes <= torch_max_gib * 2 ** 30 else (
      f"torch side skipped: about {torch_bytes / 2 ** 30:.0f} GiB of [B, L, L] temporaries (limit {torch_max_gib} GiB)")

  if op == "ndcg":
    metric = metrics.NDCGMetric(topn=10)
    sd = s.detach()
    state = {"total": torch.zeros((), device=dev), "count": torch.zeros((), device=dev)}

    def fused():
      metric.update_state(y, sd)

    def composed():
      v, c = torch_ndcg(y, sd, 10)
      state["total"].add_((v * c).sum())
      state["count"].add_(c.sum())

    check = lambda: (float(metric.result()), float(state["total"] / state["count"]))
  else:
    loss_fn = FUSED[op]()
    out = {}

    def fused():
      s.grad = None
      out["fused"] = loss_fn(y, s)
      out["fused"].backward()
      out["fused_grad"] = s.grad

    def composed():
      s.grad = None
      out["torch"] = TORCH[op](y, s).sum() / BATCH
      out["torch"].backward()
      out["torch_grad"] = s.grad

    def check():      # (an all-padding list gives the torch composition NaN gradients; the fused kernels give zeros)
      tg = torch.nan_to_num(out["torch_grad"], nan=0.0)
      return (float(out["fused"]), float(out["torch"]),
              float((out["fused_grad"] - tg).abs().max()) / max(float(tg.abs().max()), 1e-30))

  fns = {"fused": fused}
  if skip is None:
    try:
      composed()
      torch.cuda.synchronize()
      fns["torch"] = composed
    except torch.cuda.OutOfMemoryError:
      skip = "torch side skipped: its temporaries did not fit in device memory"
      torch.cuda.empty_cache()
  ts = alternate(fns, iters)
  for k, v in ts.items():
    rec[k] = stats(v)
  if "torch" in ts:
    rec["fused_over_torch_ms"] = rec["fused"]["ms_median"] / rec["torch"]["ms_median"]
    rec["agreement"] = check()       # losses: (fused, torch, max gradient difference / max gradient); ndcg: the two results
  else:
    rec["torch"] = skip
  if op.startswith("pairwise"):
    rec["pair_rate"] = 2.0 * BATCH * L * L / (rec["fused"]["ms_median"] * 1e-3)
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--only", default=",".join(OPS))
  ap.add_argument("--lengths", default=",".join(str(l) for l in LENGTHS))
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--torch-max-gib", type=float, default=96.0)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_listwise: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  lines = []
  for op in OPS:
    if op not in args.only.split(","):
      continue
    for L in (int(v) for v in args.lengths.split(",")):
      lines.append(bench(op, L, dev, args.iters, args.torch_max_gib))
      print(json.dumps(lines[-1]), flush=True)
      torch.cuda.empty_cache()
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for rec in lines:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
  main()
