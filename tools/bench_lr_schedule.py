"""What a learning-rate schedule costs in the captured quickstart train step (evidence tool, one GPU).

Two quickstart two-tower models (MovieLens-100K tables, dim 64, batch 8192 by default, no metrics) in ONE process:
``Adagrad(0.5)`` and ``Adagrad(ExponentialDecay(0.5, 1000, 0.96))``.  Each train step is captured once
(``Model.make_graphed_train_step``); the two graphs are then replayed alternately, replay by replay, each replay timed
with device events.  Expected difference: the one-thread ``tfrs_lr_tick`` kernel at the head of the scheduled step.
``--optimizer adam`` times ``Adam``, whose existing tick kernel takes the schedule in (no extra kernel).

Prints and appends one JSON line (median and p10 / p90 in microseconds per variant) to ``--out``.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import recommenders_amd as tfrs
from recommenders_amd import schedules


def quickstart(make_optimizer, seed=5):
  class TwoTower(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.user_model = tfrs.layers.embedding.Embedding(943, 64)
      self.item_model = tfrs.layers.embedding.Embedding(1682, 64)
      self.task = tfrs.tasks.Retrieval()

    def compute_loss(self, features, training=False):
      return self.task(self.user_model(features["user_id"]), self.item_model(features["movie_id"]),
                       compute_metrics=False)

  torch.manual_seed(seed)
  m = TwoTower()
  m.compile(optimizer=make_optimizer(m.parameters()))
  return m


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=8192)
  ap.add_argument("--replays", type=int, default=300)
  ap.add_argument("--warmup", type=int, default=20)
  ap.add_argument("--optimizer", choices=["adagrad", "adam"], default="adagrad")
  ap.add_argument("--out", default=os.path.join("profiles", "lr_schedule.jsonl"))
  args = ap.parse_args()
  cls, lr0 = (tfrs.optimizers.Adagrad, 0.5) if args.optimizer == "adagrad" else (tfrs.optimizers.Adam, 0.01)
  rng = np.random.default_rng(0)
  batch = {"user_id": torch.as_tensor(rng.integers(0, 943, size=args.batch)).cuda(),
           "movie_id": torch.as_tensor(rng.integers(0, 1682, size=args.batch)).cuda()}
  variants = {
      "constant": quickstart(lambda ps: cls(ps, learning_rate=lr0)),
      "scheduled": quickstart(lambda ps: cls(ps, learning_rate=schedules.ExponentialDecay(lr0, 1000, 0.96))),
  }
  steps = {name: m.make_graphed_train_step(batch) for name, m in variants.items()}
  times = {name: [] for name in steps}
  for i in range(args.warmup + args.replays):
    for name, step in steps.items():      # alternated replay by replay
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      step.graph.replay()
      stop.record()
      stop.synchronize()
      if i >= args.warmup:
        times[name].append(start.elapsed_time(stop) * 1e3)
  result = {"tool": "bench_lr_schedule", "optimizer": args.optimizer, "batch": args.batch, "replays": args.replays,
            "device": torch.cuda.get_device_name(0)}
  for name, ts in times.items():
    p10, p50, p90 = np.percentile(ts, [10, 50, 90])
    result[name] = {"median_us": round(float(p50), 3), "p10_us": round(float(p10), 3), "p90_us": round(float(p90), 3)}
  result["scheduled_minus_constant_us"] = round(result["scheduled"]["median_us"] - result["constant"]["median_us"], 3)
  result["iterations"] = int(variants["scheduled"].optimizer.iterations)
  line = json.dumps(result)
  print(line)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "a") as f:
    f.write(line + "\n")


if __name__ == "__main__":
  main()
