"""TextVectorization.forward on one GPU against what a user had before the layer, one JSON line per shape:

  graph.window / graph.direct  the layer on a device-resident PackedStrings with a fixed output_sequence_length, 64 calls
               (over 8 batches in turn) captured once in a HIP graph, device events around one replay: device time
               alone, for the kernel's two byte routes (TFRS_TEXT_VARIANT = window / direct), alternated sample by sample
  list         the layer called with a Python list: host packing, copy, one launch; host clock to synchronise
  baseline     Python lower / translate / split per string, StringLookup over the flat tokens, padding on the device;
               host clock to synchronise

Text: synthetic, seeded, from a fixed list of 12 000 words of which the first 9 998 are the vocabulary (10 000 entries
with the two special ones), so a sixth of the words and every year are unknown; random case, punctuation and a year in brackets, as
movie titles have.  Shapes: 8 192 and 65 536 strings of about 28 bytes (output_sequence_length 8), 8 192 strings of
about 200 bytes (32).  All four ways give the same indices (checked before anything is timed).

Every figure is a median with its p10 / p90 over the samples, and the whole measurement of a shape is REPEATED
(``run2``) so that the spread between two runs stands next to every difference read off one of them.  The last line
names each shape's winner (a variant wins only when it wins in both runs) and the default that follows from them.

    python tools/bench_text_vectorization.py [--samples N] [--out profiles/text_vectorization.jsonl]
"""
import argparse
import json
import os
import string
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from recommenders_amd import _lib
from recommenders_amd.layers import preprocessing
from recommenders_amd.layers.hashing import PackedStrings

SHAPES = ((8_192, 28, 8), (65_536, 28, 8), (8_192, 200, 32))     # strings, about this many bytes each, sequence length
BATCHES = 8                                                      # distinct batches per shape
CALLS = 64                                                       # calls captured in one graph: every batch 8 times
VOCABULARY = 10_000
_STRIP = str.maketrans("", "", string.punctuation)


def word_list(n):
  """n distinct lower-case words of 3 to 9 letters, the same on every run."""
  rng = np.random.default_rng(1234)
  words = set()
  while len(words) < n:
    words.add("".join(chr(97 + c) for c in rng.integers(0, 26, size=int(rng.integers(3, 10)))))
  return sorted(words)


def make_text(rng, words, n, target_bytes):
  k = max(1, round((target_bytes - 7) / 7.5))                  # a word and its space: 7.5 bytes on average; "(1995)": 6
  pick = rng.integers(len(words), size=(n, k)).tolist()
  upper = (rng.integers(3, size=(n, k)) > 0).tolist()
  mark = rng.integers(24, size=(n, k)).tolist()                # one word in six carries punctuation
  years = rng.integers(1930, 2025, size=n).tolist()
  marks = (":", ",", "'s", "!")
  out = []
  for row, caps, ms, year in zip(pick, upper, mark, years):
    parts = [(words[w].capitalize() if c else words[w]) + (marks[m] if m < 4 else "") for w, c, m in zip(row, caps, ms)]
    out.append(" ".join(parts) + " (%d)" % year)
  return out


def stats(ts):
  ts = sorted(ts)
  return {"ms_median": ts[len(ts) // 2], "ms_p10": ts[len(ts) // 10], "ms_p90": ts[(len(ts) * 9) // 10], "samples": len(ts)}


def graphed(layer, batches, variant):
  _lib.set_option("TFRS_TEXT_VARIANT", variant)
  try:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for b in batches[:2]:
        layer(b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      outs = [layer(batches[c % len(batches)]) for c in range(CALLS)]
  finally:
    _lib.set_option("TFRS_TEXT_VARIANT", None)
  return graph, outs


def device_times(graphs, samples, warmup=3):
  """{name: [ms per call]}: the replays alternated sample by sample, device events around each."""
  for _ in range(warmup):
    for g in graphs.values():
      g.replay()
  events = {k: [] for k in graphs}
  for _ in range(samples):
    for k, g in graphs.items():
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      g.replay()
      b.record()
      events[k].append((a, b))
  torch.cuda.synchronize()
  return {k: [a.elapsed_time(b) / CALLS for a, b in v] for k, v in events.items()}


def host_times(fn, samples, warmup=2):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(samples):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  return ts


def baseline(lookup, seq_len, dev):
  """What a user wrote before the layer: tokens on the host, StringLookup over the flat list, padding."""
  def run(strings):
    rows = [s.lower().translate(_STRIP).split() for s in strings]
    flat = [t for r in rows for t in r[:seq_len]]
    ids = lookup(flat)
    lengths = torch.as_tensor([min(len(r), seq_len) for r in rows], device=dev)
    out = torch.zeros((len(rows), seq_len), dtype=torch.int64, device=dev)
    out[torch.arange(seq_len, device=dev)[None, :] < lengths[:, None]] = ids
    return out
  return run


def bench_shape(words, n, target_bytes, seq_len, samples, dev):
  rng = np.random.default_rng(n + target_bytes)
  vocab = words[:VOCABULARY - 2]
  layer = preprocessing.TextVectorization(vocabulary=vocab, output_sequence_length=seq_len, device=dev)
  lookup = preprocessing.StringLookup(vocabulary=vocab, mask_token="", device=dev)     # the same index layout
  texts = [make_text(rng, words, n, target_bytes) for _ in range(BATCHES)]
  batches = [PackedStrings.from_strings(t, dev) for t in texts]
  user = baseline(lookup, seq_len, dev)
  want = user(texts[0])
  assert torch.equal(layer(texts[0]), want), "the layer and the host baseline disagree"
  graphs = {}
  for variant in ("window", "direct"):
    graphs[variant], outs = graphed(layer, batches, variant)
    graphs[variant].replay()
    assert torch.equal(outs[0], want), f"the {variant} variant and the host baseline disagree"
  rec = {"op": "TextVectorization.forward", "strings": n, "bytes_per_string": float(np.mean([len(s) for s in texts[0]])),
         "tokens_per_string": float((want != 0).sum()) / n, "unknown_share": float((want == 1).sum()) / float((want != 0).sum()),
         "output_sequence_length": seq_len, "vocabulary": VOCABULARY, "calls_per_replay": CALLS}
  for run in ("run1", "run2"):
    dev_ts = device_times(graphs, samples)
    r = {"graph": {k: stats(v) for k, v in dev_ts.items()},
         "list": stats(host_times(lambda: layer(texts[1]), max(samples // 4, 5))),
         "baseline": stats(host_times(lambda: user(texts[1]), max(samples // 8, 3)))}
    r["graph"]["window_over_direct"] = r["graph"]["window"]["ms_median"] / r["graph"]["direct"]["ms_median"]
    r["strings_per_s_device"] = n / (min(r["graph"][k]["ms_median"] for k in ("window", "direct")) * 1e-3)
    r["baseline_over_list"] = r["baseline"]["ms_median"] / r["list"]["ms_median"]
    rec[run] = r
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--samples", type=int, default=40)
  ap.add_argument("--out", default=os.path.join("profiles", "text_vectorization.jsonl"))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("bench_text_vectorization: needs a GPU (no CPU fallback for a measurement)")
  dev = torch.device("cuda", 0)
  words = word_list(12_000)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "a") as f:
    def emit(rec):
      print(json.dumps(rec), flush=True)
      f.write(json.dumps(rec) + "\n")
      f.flush()

    shapes = []
    for n, target_bytes, seq_len in SHAPES:
      rec = bench_shape(words, n, target_bytes, seq_len, args.samples, dev)
      ratios = [rec[run]["graph"]["window_over_direct"] for run in ("run1", "run2")]
      # a variant wins a shape only when it wins in BOTH runs
      winner = "window" if max(ratios) < 1.0 else "direct" if min(ratios) > 1.0 else "neither"
      shapes.append({"strings": n, "bytes_per_string": rec["bytes_per_string"], "window_over_direct": ratios,
                     "winner": winner, "workgroup_span_over_window": rec["bytes_per_string"] * 256 /
                     preprocessing.TEXT_WINDOW_BYTES})
      emit(rec)
    won = {s["winner"] for s in shapes}
    if "window" not in won:
      follows = "direct"
    elif "direct" not in won:
      follows = "window"
    else:    # the library's rule: the window while the 256 strings of a workgroup fit one window on average
      fits = all((s["winner"] == "window") == (s["workgroup_span_over_window"] <= 1.0) for s in shapes
                 if s["winner"] != "neither")
      follows = "window while a workgroup's span fits one window, direct beyond" if fits else "mixed: see the shapes"
    emit({"op": "TextVectorization default variant", "shapes": shapes, "default_that_follows": follows})

if __name__ == "__main__":
  main()
