"""ScaNN (partitioned, 4-bit product-quantized top-K) against BruteForce on the same corpus, in one process.

    python tools/bench_scann.py [--configs iid-1m,clustered-1m,clustered-12m,clustered-100m] [--batches 1,64,8192]

One JSON line per (corpus, ScaNN setting): index build seconds, device bytes held by the index, recall@10 against
BruteForce on 1000 queries, and ms per call (device events over warm windows of >= 0.5 s) at each batch, eager and
graphed; plus one line per corpus for BruteForce timed the same way.  Corpora: i.i.d. Gaussian, and the clustered
mixture of tools/bench_clustered.py (Gaussian centres, Zipf(1) popularity, 0.35 spread).  Settings: the reference
tutorial's (num_leaves, num_leaves_to_search, num_reordering_candidates): defaults (100, 10, None), (1000, 100,
1000), (1000, 70, 400); 10 000 leaves for the 100 M corpus."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from recommenders_amd.layers import factorized_top_k as ftk  # noqa: E402

K = 10
SETTINGS_1M = [dict(num_leaves=100, num_leaves_to_search=10, num_reordering_candidates=None),
               dict(num_leaves=1000, num_leaves_to_search=100, num_reordering_candidates=1000),
               dict(num_leaves=1000, num_leaves_to_search=70, num_reordering_candidates=400)]
CONFIGS = {
    "iid-1m": (1_000_000, 64, False, SETTINGS_1M),
    "clustered-1m": (1_000_000, 64, True, SETTINGS_1M),
    "clustered-12m": (12_500_000, 128, True, [dict(num_leaves=1000, num_leaves_to_search=100,
                                                   num_reordering_candidates=1000)]),
    "clustered-100m": (100_000_000, 64, True, [dict(num_leaves=10_000, num_leaves_to_search=100,
                                                    num_reordering_candidates=1000)]),
}


def corpus(n, d, clustered, g, dev, nq):
  if not clustered:
    return (torch.randn((n, d), generator=g, device=dev) / d ** 0.5,
            torch.randn((nq, d), generator=g, device=dev) / d ** 0.5)
  c = max(1000, n // 1000)
  centres = torch.randn((c, d), generator=g, device=dev) / d ** 0.5
  pop = 1.0 / torch.arange(1, c + 1, device=dev, dtype=torch.float32)
  pop = pop / pop.sum()

  def draw(m):
    out = torch.empty((m, d), device=dev)
    for lo in range(0, m, 1 << 22):
      hi = min(m, lo + (1 << 22))
      cl = torch.multinomial(pop, hi - lo, replacement=True, generator=g)
      out[lo:hi] = centres[cl] + 0.35 * torch.randn((hi - lo, d), generator=g, device=dev) / d ** 0.5
    return out

  return draw(n), draw(nq)


def ms_per_call(fn, min_seconds=0.5):
  """Device time per call over a warm window of >= min_seconds (events around the window)."""
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  iters = 1
  while True:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
      fn()
    end.record()
    end.synchronize()
    ms = start.elapsed_time(end)
    if ms >= min_seconds * 1e3:
      return ms / iters
    iters = max(iters * 2, int(iters * min_seconds * 1.2e3 / max(ms, 1e-3)))


def timings(layer, queries, batches):
  out = {}
  for b in batches:
    q = queries[:b].contiguous() if b <= queries.shape[0] else queries.repeat((b + queries.shape[0] - 1)
                                                                              // queries.shape[0], 1)[:b].contiguous()
    out[f"eager_ms_b{b}"] = round(ms_per_call(lambda: layer(q)), 4)
    print(f"  batch {b}: eager {out[f'eager_ms_b{b}']} ms", file=sys.stderr, flush=True)
    graphed = layer.make_graphed_call(q)
    out[f"graphed_ms_b{b}"] = round(ms_per_call(lambda: graphed(q)), 4)
    del graphed
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--configs", default="iid-1m,clustered-1m")
  ap.add_argument("--batches", default="1,64,8192")
  args = ap.parse_args()
  dev = torch.device("cuda", 0)
  batches = [int(b) for b in args.batches.split(",")]
  for name in args.configs.split(","):
    n, d, clustered, settings = CONFIGS[name]
    g = torch.Generator(device=dev).manual_seed(1)
    cand, queries = corpus(n, d, clustered, g, dev, 8192)
    bf = ftk.BruteForce(k=K).index(cand)
    _, truth = bf(queries[:1000])
    truth = truth.cpu().numpy()
    line = {"op": "BruteForce top-10", "corpus": name, "n": n, "d": d}
    line.update(timings(bf, queries, batches))
    print(json.dumps(line), flush=True)
    del bf
    for s in settings:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      layer = ftk.ScaNN(k=K, **s).index(cand)
      torch.cuda.synchronize()
      build_s = time.perf_counter() - t0
      print(f"{name} {s}: index built in {build_s:.1f} s", file=sys.stderr, flush=True)
      _, got = layer(queries[:1000])
      got = got.cpu().numpy()
      recall = sum(len(set(got[i].tolist()) & set(truth[i].tolist())) for i in range(1000)) / (10.0 * 1000)
      l_eff, p_max = layer.probe_plan()
      line = {"op": "ScaNN top-10", "corpus": name, "n": n, "d": d, **s, "l_eff": l_eff, "p_max": p_max,
              "index_build_s": round(build_s, 2), "index_bytes": layer.index_bytes(), "recall_at_10": recall}
      line.update(timings(layer, queries, batches))
      print(json.dumps(line), flush=True)
      del layer
      torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
