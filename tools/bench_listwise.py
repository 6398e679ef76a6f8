"""The fused listwise losses (forward + backward) and the list metrics against a torch composition of the same formulas
(DESIGN 4.24, 4.26), in one process on one GPU, one JSON line per (op, list length):

  B = 8192 lists of L in {5, 32, 128, 512} items, labels in {-1, 0, .., 4} (one position in six padded), scores N(0, 2)

The torch side is what a user could write without the kernels: a masked logsumexp for the softmax loss, a
``[B, L, L]`` difference tensor for the pairwise losses (several temporaries of that size live through the backward),
a stable sort + ``logcumsumexp`` for ListMLE, two sorts for NDCG, one sort + gather + cumsum for the rank metrics (MRR,
hits, precision, recall, MAP, DCG, ARP) and ``[B, L, L]`` boolean tensors for OPA.  Where its temporaries (estimated as
ten ``[B, L, L]`` float32 tensors for the pairwise losses and OPA) exceed ``--torch-max-gib``, or the allocation fails, the
torch side is skipped and the line says so.

``metric_group`` is the six-metric set NDCG@10, MRR, MAP, Precision@10, Recall@10, OPA of one step, three sides: ``torch``
(the composition, ONE score sort shared by the rank metrics), ``separate`` (six fused ``update_state`` calls) and
``grouped`` (one ``metrics.update_listwise_metrics`` call: one launch).

Timing: device events around every call (loss forward, ``backward()`` included; for the metric one ``update_state``),
the two sides alternated call by call after warm-up, median and p10 / p90 over the calls.  ``pair_rate`` is the number
of (i, j) position pairs a pairwise loss walks (B L L, forward and backward each) over the fused median.

``--other-lib PATH`` adds the op ``ndcg_entry``: the C entry ``tfrs_listwise_ndcg`` alone (no torch reduction, ``topn`` 10)
of this tree's library against the library at PATH -- another build of ``libtfrs_hip.so``, such as the parent commit's --
loaded into the same process and alternated (this, other, other, this) call by call; before the timing one record
says on how many cases (67 lists at every length on both sides of a switch of the work mapping x ``topn`` in
{none, 1, 10, 2000} x continuous and grid scores) the two libraries returned identical bits, and the tool stops if any
differs.

    python tools/bench_listwise.py [--only softmax,pairwise_logistic,...] [--lengths 5,32] [--iters N] [--out FILE]
                                   [--other-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recommenders_amd import _lib, losses, metrics

BATCH = 8192
LENGTHS = (5, 32, 128, 512)
METRIC_OPS = ("ndcg", "dcg", "mrr", "hits", "precision", "recall", "map", "arp", "opa")
OPS = ("softmax", "pairwise_logistic", "pairwise_hinge", "list_mle") + METRIC_OPS + ("metric_group",)
GROUP = ("ndcg", "mrr", "map", "precision", "recall", "opa")
TOPN = {"ndcg": 10, "dcg": 10, "mrr": None, "hits": 10, "precision": 10, "recall": 10, "map": None}      # arp, opa: none
METRIC = {"ndcg": metrics.NDCGMetric, "dcg": metrics.DCGMetric, "mrr": metrics.MRRMetric, "hits": metrics.HitsMetric,
          "precision": metrics.PrecisionMetric, "recall": metrics.RecallMetric, "map": metrics.MeanAveragePrecisionMetric,
          "arp": metrics.ARPMetric, "opa": metrics.OPAMetric}
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


def torch_by_score(y, s):
  """Labels in score order (descending, ties by position), invalid positions last as -1."""
  valid = y >= 0
  order = torch.sort(torch.where(valid, s, torch.full_like(s, NEG_INF)), dim=1, descending=True, stable=True).indices
  return torch.gather(torch.where(valid, y, torch.full_like(y, -1.0)), 1, order)


def torch_rank_metric(name, ys, topn):
  """(value, weight) per list of one rank metric from the labels in score order."""
  L = ys.shape[1]
  ranks = torch.arange(L, device=ys.device, dtype=torch.float32)
  cut = (ranks < (L if topn is None else topn)).to(torch.float32)
  ok = ys >= 0
  yv = torch.where(ok, ys, torch.zeros_like(ys))
  if name == "dcg":
    return ((torch.exp2(yv) - 1.0) / torch.log2(ranks + 2.0) * cut).sum(dim=1), (yv > 0).any(dim=1).to(torch.float32)
  if name == "arp":
    den = yv.sum(dim=1)
    return torch.where(den > 0, (yv * (ranks + 1.0)).sum(dim=1) / den.clamp_min(1e-30), torch.zeros_like(den)), den
  rel = (ys >= 1).to(torch.float32)
  total = rel.sum(dim=1)
  has = (total > 0).to(torch.float32)
  relc = rel * cut
  ck = relc.sum(dim=1)
  if name == "mrr":
    return (relc / (ranks + 1.0)).max(dim=1).values, has
  if name == "hits":
    return (ck > 0).to(torch.float32), has
  if name == "precision":
    return ck / float(L if topn is None else min(topn, L)), has
  if name == "recall":
    return ck / total.clamp_min(1.0), has
  if name == "map":
    return (relc * torch.cumsum(rel, dim=1) / (ranks + 1.0)).sum(dim=1) / total.clamp_min(1.0), has
  raise ValueError(name)


def torch_opa(y, s):
  valid = y >= 0
  pair = valid[:, :, None] & valid[:, None, :] & (y[:, :, None] > y[:, None, :])
  right = pair & (s[:, :, None] > s[:, None, :])
  p = pair.sum(dim=(1, 2)).to(torch.float32)
  return right.sum(dim=(1, 2)).to(torch.float32) / p.clamp_min(1.0), p


def torch_metrics(names, y, s):
  """{name: (value, weight)}: one score sort for all the rank metrics among ``names``."""
  out, ys = {}, None
  for name in names:
    if name == "ndcg":
      v, c = torch_ndcg(y, s, TOPN["ndcg"])
      out[name] = (v, c.to(torch.float32))
    elif name == "opa":
      out[name] = torch_opa(y, s)
    else:
      ys = torch_by_score(y, s) if ys is None else ys
      out[name] = torch_rank_metric(name, ys, TOPN.get(name))
  return out


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
  is_metric = op in METRIC_OPS or op == "metric_group"
  rec = {"op": op, "batch": BATCH, "list_len": L, "direction": "update_state" if is_metric else "forward + backward"}
  pairs = op.startswith("pairwise") or op in ("opa", "metric_group")
  torch_bytes = 10 * BATCH * L * L * 4 if pairs else 12 * BATCH * L * 4
  skip = None if torch_bytes <= torch_max_gib * 2 ** 30 else (
      f"torch side skipped: about {torch_bytes / 2 ** 30:.0f} GiB of [B, L, L] temporaries (limit {torch_max_gib} GiB)")

  fns = {}
  if is_metric:
    names = GROUP if op == "metric_group" else (op,)
    make = lambda: [METRIC[n]() if n in ("arp", "opa") else METRIC[n](topn=TOPN[n]) for n in names]
    sd = s.detach()
    state = {n: {"total": torch.zeros((), device=dev), "count": torch.zeros((), device=dev)} for n in names}
    separate = make()

    def fused():
      for m in separate:
        m.update_state(y, sd)

    def composed():
      for n, (v, w) in torch_metrics(names, y, sd).items():
        state[n]["total"].add_((v * w).sum())
        state[n]["count"].add_(w.sum())

    check_pairs = [separate]
    if op == "metric_group":
      rec["metrics"] = ["%s@%s" % (n, TOPN.get(n)) for n in names]
      grouped = make()
      fns["grouped"] = lambda: metrics.update_listwise_metrics(grouped, y, sd)
      check_pairs.append(grouped)

    # per metric: the fused result(s), then the torch result
    check = lambda: {n: [float(ms[i].result()) for ms in check_pairs] + [float(state[n]["total"] / state[n]["count"])]
                     for i, n in enumerate(names)}
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

  fns = {"separate" if op == "metric_group" else "fused": fused, **fns}
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
    rec["fused_over_torch_ms"] = rec["grouped" if op == "metric_group" else "fused"]["ms_median"] / rec["torch"]["ms_median"]
    # losses: (fused, torch, max gradient difference / max gradient); metrics: per metric the fused result(s), then torch's
    rec["agreement"] = check()
  else:
    rec["torch"] = skip
  if op == "metric_group":
    rec["grouped_over_separate_ms"] = rec["grouped"]["ms_median"] / rec["separate"]["ms_median"]
  if op.startswith("pairwise"):
    rec["pair_rate"] = 2.0 * BATCH * L * L / (rec["fused"]["ms_median"] * 1e-3)
  return rec


EDGE_LENGTHS = (1, 2, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 256, 257, 1024)


def _ndcg_entry(lib, y, s, topn, out):
  rc = lib.tfrs_listwise_ndcg(_lib.ptr(y), _lib.ptr(s), y.shape[0], y.shape[1], topn, _lib.ptr(out[0]), _lib.ptr(out[1]),
                              _lib.current_stream())
  if rc != 0:
    raise SystemExit(f"bench_listwise: tfrs_listwise_ndcg returned {rc}")


def _other_library(path):
  other = ctypes.CDLL(os.path.abspath(path))
  p = ctypes.c_void_p
  other.tfrs_listwise_ndcg.restype = ctypes.c_int
  other.tfrs_listwise_ndcg.argtypes = [p, p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, p, p, p]
  return other


def ndcg_entry_bits(other, path, dev):
  """One record: the cases on which the two libraries' ndcg and counted outputs have identical bits (all, or exit)."""
  this = _lib.load()
  cases = lists = 0
  for L in EDGE_LENGTHS:
    for grid in (False, True):
      g = torch.Generator(device=dev).manual_seed(7 * L + grid)
      y = torch.randint(-1, 5, (67, L), generator=g, device=dev).to(torch.float32)
      s = torch.randn((67, L), generator=g, device=dev) * 2.0
      s = torch.round(s * 2.0) / 2.0 if grid else s
      for topn in (0, 1, 10, 2000):
        a, b = torch.full((2, 67), -7.0, device=dev), torch.full((2, 67), -9.0, device=dev)
        _ndcg_entry(this, y, s, topn, a)
        _ndcg_entry(other, y, s, topn, b)
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
          raise SystemExit(f"bench_listwise: tfrs_listwise_ndcg differs from {path} at L={L} topn={topn} grid={grid}")
        cases += 1
        lists += 67
  return {"op": "ndcg_entry", "other_lib": os.path.basename(path), "bit_equal_cases": cases, "bit_equal_lists": lists}


def bench_ndcg_entry(other, path, L, dev, iters):
  this = _lib.load()
  g = torch.Generator(device=dev).manual_seed(L)
  y = torch.randint(-1, 5, (BATCH, L), generator=g, device=dev).to(torch.float32)
  s = torch.randn((BATCH, L), generator=g, device=dev) * 2.0
  out = torch.zeros((2, BATCH), device=dev)
  ts = alternate({"this_first": lambda: _ndcg_entry(this, y, s, 10, out), "other": lambda: _ndcg_entry(other, y, s, 10, out),
                  "other_again": lambda: _ndcg_entry(other, y, s, 10, out), "this": lambda: _ndcg_entry(this, y, s, 10, out)},
                 iters)
  rec = {"op": "ndcg_entry", "other_lib": os.path.basename(path), "batch": BATCH, "list_len": L, "direction": "tfrs_listwise_ndcg alone"}
  for k, v in ts.items():
    rec[k] = stats(v)
  rec["this_over_other_ms"] = ((rec["this_first"]["ms_median"] + rec["this"]["ms_median"]) /
                               (rec["other"]["ms_median"] + rec["other_again"]["ms_median"]))
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--only", default=",".join(OPS))
  ap.add_argument("--lengths", default=",".join(str(l) for l in LENGTHS))
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--torch-max-gib", type=float, default=96.0)
  ap.add_argument("--out", default=None)
  ap.add_argument("--other-lib", default=None, help="another build of libtfrs_hip.so: adds the op ndcg_entry")
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
  if args.other_lib:
    other = _other_library(args.other_lib)
    lines.append(ndcg_entry_bits(other, args.other_lib, dev))
    print(json.dumps(lines[-1]), flush=True)
    for L in (int(v) for v in args.lengths.split(",")):
      lines.append(bench_ndcg_entry(other, args.other_lib, L, dev, args.iters))
      print(json.dumps(lines[-1]), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      for rec in lines:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
  main()
