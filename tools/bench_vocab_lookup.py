"""IntegerLookup.forward against the composition a torch user writes today, on one GPU, one JSON line per shape:

  layer        IntegerLookup(vocabulary=v)(ids): one launch of the hash-table lookup (csrc/vocab.hip)
  composition  pos = searchsorted(v_sorted, ids); hit = v_sorted[pos] == ids; where(hit, 1 + pos, 0)

The vocabulary is n sorted distinct random 64-bit ids, so both sides give the same indices (checked before anything is
timed).  Shapes: vocabulary 1 700, 1 M, 26 M; 8 192 and 65 536 ids per call; 0 % and 50 % of the ids unknown.  Then
StringLookup on 8 192 titles over a 1 700-title vocabulary (its host-side packing included: that is what a call costs).

Timing, two ways, the two sides alternated sample by sample in one process after warm-up:
  eager   device events around C back-to-back calls issued to an idle queue, divided by C: what a Python loop pays,
          launch and host overhead included
  graph   the same C calls captured once in a HIP graph, device events around one replay: device time alone
Every call of a sample looks up ids of its own, C = 2^22 / ids per call: one sample touches 2^22 table lines of 128 B,
twice the 256 MiB cache, so a table that is larger than the cache is not read from it.
Median, p10 and p90 over the samples.  Bytes are algorithmic: 8 B read and 8 B written per id, 16 B per probe.

    python tools/bench_vocab_lookup.py [--vocab 1700,1000000,26000000] [--samples N] [--out profiles/vocab_lookup.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommenders_amd.layers import preprocessing

IDS_PER_SAMPLE = 1 << 22    # distinct ids per sample: their table lines (128 B each, 512 MiB) do not fit the 256 MiB cache
VOCABS = (1_700, 1_000_000, 26_000_000)
BATCHES = (8_192, 65_536)
UNKNOWN = (0.0, 0.5)


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
  empty when a sample starts, so its events bracket the host's enqueueing too, not only work queued behind the other
  side's."""
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


def graphed(fn, calls):
  """fn(0) .. fn(calls - 1) captured in one graph on one stream; returns the replay."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for c in range(2):
      fn(c)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    for c in range(calls):
      fn(c)
  return graph.replay


def make_vocabulary(n, dev, g):
  v = torch.unique(torch.randint(-(1 << 62), 1 << 62, (n + n // 64 + 64,), generator=g, device=dev))
  assert v.numel() >= n
  return v[:n].contiguous()      # sorted, distinct


def make_ids(vocab, n, unknown, g):
  known = vocab[torch.randint(0, vocab.numel(), (n,), generator=g, device=vocab.device)]
  far = torch.randint(-(1 << 62), 1 << 62, (n,), generator=g, device=vocab.device)   # a token with chance < 2^-37
  pick = torch.rand((n,), generator=g, device=vocab.device) < unknown
  return torch.where(pick, far, known).contiguous()


def bench_integer(vocab, layer, n, unknown, samples, g):
  calls = IDS_PER_SAMPLE // n
  ids = make_ids(vocab, n * calls, unknown, g).reshape(calls, n)     # every call of a sample looks up ids of its own
  last = vocab.numel() - 1

  def composition(c):
    pos = torch.searchsorted(vocab, ids[c]).clamp_(max=last)
    return torch.where(vocab[pos] == ids[c], pos + 1, 0)

  def run_layer(c):
    return layer(ids[c])

  share = 0.0
  for c in (0, calls - 1):
    got, want = run_layer(c), composition(c)
    assert torch.equal(got, want), "the layer and the composition disagree"
    share = float((got == 0).float().mean())

  def many(fn):
    def run():
      for c in range(calls):
        fn(c)
    return run

  eager = alternate({"layer": many(run_layer), "composition": many(composition)}, calls, samples, drain=True)
  graph = alternate({"layer": graphed(run_layer, calls), "composition": graphed(composition, calls)}, calls, samples)
  rec = {"op": "IntegerLookup.forward vs searchsorted + eq + where", "vocabulary": vocab.numel(),
         "table_slots": int(layer._table.shape[0]), "ids": n, "unknown_share": share, "calls_per_sample": calls}
  for mode, ts in (("eager", eager), ("graph", graph)):
    rec[mode] = {k: stats(v) for k, v in ts.items()}
    rec[mode]["layer_over_composition"] = rec[mode]["layer"]["ms_median"] / rec[mode]["composition"]["ms_median"]
    rec[mode]["layer_ids_per_s"] = n / (rec[mode]["layer"]["ms_median"] * 1e-3)
  return rec


def bench_strings(samples, dev):
  titles = ["Movie number %d, The (19%02d)" % (i, i % 100) for i in range(1_700)]
  layer = preprocessing.StringLookup(vocabulary=titles, device=dev)
  rng = np.random.default_rng(0)
  queries = np.array(titles, dtype=object)[rng.integers(0, len(titles), size=8_192)]
  want = 1 + np.array([titles.index(q) for q in queries[:256]])
  assert np.array_equal(layer(queries[:256]).cpu().numpy(), want)
  for _ in range(3):
    layer(queries)
  torch.cuda.synchronize()
  ts = []
  for _ in range(samples):
    t0 = time.perf_counter()
    layer(queries)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  return {"op": "StringLookup.forward (host packing + fingerprint + lookup), host clock to synchronise",
          "vocabulary": len(titles), "ids": int(queries.size), "bytes_per_title": sum(map(len, queries)) / queries.size,
          "call": stats(ts)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--vocab", default=",".join(str(v) for v in VOCABS))
  ap.add_argument("--samples", type=int, default=40)
  ap.add_argument("--out", default=os.path.join("profiles", "vocab_lookup.jsonl"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_vocab_lookup: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  g = torch.Generator(device=dev).manual_seed(0)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "a") as f:
    def emit(rec):
      print(json.dumps(rec), flush=True)
      f.write(json.dumps(rec) + "\n")
      f.flush()

    preprocessing.IntegerLookup(vocabulary=[1, 2, 3], device=dev)(torch.tensor([1], device=dev))   # loads the library
    for n_vocab in (int(v) for v in args.vocab.split(",")):
      vocab = make_vocabulary(n_vocab, dev, g)
      t0 = time.perf_counter()
      layer = preprocessing.IntegerLookup(vocabulary=vocab, device=dev)
      torch.cuda.synchronize()
      build_ms = (time.perf_counter() - t0) * 1e3
      for n in BATCHES:
        for unknown in UNKNOWN:
          rec = bench_integer(vocab, layer, n, unknown, args.samples, g)
          rec["set_vocabulary_ms"] = build_ms
          emit(rec)
      del layer, vocab
      torch.cuda.empty_cache()
    emit(bench_strings(args.samples, dev))


if __name__ == "__main__":
  main()
