"""Forward + backward time and peak memory of ``Retrieval`` with hard negatives over adjusted logits: the mined route
(``csrc/softmax_mined.hip``: radix select + keep predicate inside the streaming kernels, no ``[B, C]`` tensor) against
the explicit route (``TFRS_RETRIEVAL_EXPLICIT=1``: dense GEMM, element-wise passes, paged top-k, row-wise
cross-entropy on the matrix).

    python tools/bench_hard_negatives.py [--out profiles/hard_negatives.jsonl] [--iters 20]

One JSON line per (shape, options, route): median / min milliseconds of a step over ``--iters`` timed steps after
warm-up (device events around forward + backward, queue drained before each), and ``torch.cuda.max_memory_allocated``
above the level before the step (inputs excluded)."""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import recommenders_amd as tfrs

SHAPES = [  # (B, C, d, n), each with the sampling correction and accidental-hit removal
    (4096, 4096, 64, 100), (8192, 8192, 64, 100), (2048, 16384, 64, 100), (8192, 8192, 64, 1000),
]


def measure(b, c_rows, d, n, explicit, iters, warmup=3):
  gen = torch.Generator(device="cuda").manual_seed(b + c_rows + n)
  q = (torch.randn((b, d), device="cuda", generator=gen) / d ** 0.25).requires_grad_(True)
  c = (torch.randn((c_rows, d), device="cuda", generator=gen) / d ** 0.25).requires_grad_(True)
  call = dict(compute_metrics=False,
              candidate_sampling_probability=torch.rand((c_rows,), device="cuda", generator=gen),
              candidate_ids=torch.randint(0, c_rows // 2, (c_rows,), device="cuda", generator=gen))
  task = tfrs.tasks.Retrieval(num_hard_negatives=n, remove_accidental_hits=True)
  if explicit:
    os.environ["TFRS_RETRIEVAL_EXPLICIT"] = "1"
  else:
    os.environ.pop("TFRS_RETRIEVAL_EXPLICIT", None)

  def step():
    q.grad = c.grad = None
    loss = task(q, c, **call)
    loss.backward()
    return loss

  for _ in range(warmup):
    loss = step()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  step()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - before
  times = []
  for _ in range(iters):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    step()
    t1.record()
    t1.synchronize()
    times.append(t0.elapsed_time(t1))
  os.environ.pop("TFRS_RETRIEVAL_EXPLICIT", None)
  return dict(B=b, C=c_rows, d=d, n=n, options="correction+accidental_hits",
              route="explicit" if explicit else "mined", ms_median=round(statistics.median(times), 4),
              ms_min=round(min(times), 4), peak_mb=round(peak / 2 ** 20, 1), loss=float(loss.detach()), iters=iters)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join("profiles", "hard_negatives.jsonl"))
  ap.add_argument("--iters", type=int, default=20)
  args = ap.parse_args()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    for shape in SHAPES:
      for explicit in (False, True):
        line = measure(*shape, explicit=explicit, iters=args.iters)
        line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
  main()
