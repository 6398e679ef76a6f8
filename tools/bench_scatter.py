"""Large-vocabulary scatter-add / fused sparse Adagrad at BASELINE configs[3] shapes (1.7M looked-up
rows of dim 128 from 26 x 1M-row tables): time incl. the library's own radix sort, vs HBM.

``--rule sgd|adam|ftrl`` times that rule's sparse update (``tfrs_table_update_sparse``) in the same process as the
Adagrad update, alternating the two in windows of at least 0.5 s after a warm-up, with the device-to-device copy ceiling
measured in the same process, and the non-temporal row streams on and off (``TFRS_SCATTER_NT``); ``--out FILE`` appends
the result lines to a text file (profiles/table_optimizers.txt)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from recommenders_amd import _lib
from recommenders_amd.layers import embedding as emb

ap = argparse.ArgumentParser()
ap.add_argument("--rule", choices=["adagrad", "sgd", "adam", "ftrl"], nargs="+", default=["adagrad"])
ap.add_argument("--vocab", type=int, default=26_000_000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--ids", type=int, default=65536 * 26)
ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
ap.add_argument("--rounds", type=int, default=3, help="alternations of every variant")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
vocab, d, n = args.vocab, args.dim, args.ids
table = torch.empty((vocab, d), device=dev).uniform_(-0.05, 0.05)
acc = torch.full_like(table, 0.1)
ids = torch.randint(0, vocab, (n,), generator=g, device=dev)
go = torch.randn((n, d), generator=g, device=dev)
uniq = int(torch.unique(ids).numel())


def emit(record):
  line = json.dumps(record)
  print(line, flush=True)
  if args.out:
    with open(args.out, "a") as f:
      f.write(line + "\n")


def timeit(fn, iters=10):
  for _ in range(2): fn()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
  for a, b in ev:
    a.record(); fn(); b.record()
  torch.cuda.synchronize()
  ts = sorted(a.elapsed_time(b) for a, b in ev)
  return ts[len(ts) // 2] * 1e-3


def window(fn, seconds):
  """Mean time per call over one window of at least ``seconds`` (device events around the whole window)."""
  iters = max(3, int(seconds / max(timeit(fn, 3), 1e-6)) + 1)
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters): fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) * 1e-3 / iters


def algorithmic_bytes(streams_per_row):
  """Gradient rows read + ``streams_per_row`` reads and writes of a touched row + ids."""
  return n * d * 4 + streams_per_row * uniq * d * 4 + n * 8


adagrad = lambda: emb.adagrad_sparse_update_(table, acc, go, ids, 0.5)

if args.rule == ["adagrad"]:
  t = timeit(adagrad)
  byts = algorithmic_bytes(4)
  emit({"op": "sparse_adagrad (own radix sort + fused segmented update)", "rows": n, "unique": uniq,
        "dim": d, "ms": t * 1e3, "gbps": byts / t / 1e9, "frac_hbm_peak": byts / t / 8e12,
        "algorithmic_bytes": byts})
  sys.exit(0)

from recommenders_amd import optimizers

# the copy ceiling of this device, in this process: a device-to-device copy moves 2 bytes per byte copied
src = torch.empty((1 << 30,), dtype=torch.uint8, device=dev)
dst = torch.empty_like(src)
t_copy = min(window(lambda: dst.copy_(src), args.window) for _ in range(3))
ceiling = 2 * src.numel() / t_copy
del src, dst
emit({"op": "copy ceiling (1 GiB device-to-device, read + write)", "gbps": ceiling / 1e9})

builders = {"sgd": lambda p: optimizers.SGD([p], learning_rate=0.01), "adam": lambda p: optimizers.Adam([p]),
            "ftrl": lambda p: optimizers.Ftrl([p], learning_rate=0.05)}
slots = {"sgd": 0, "adam": 2, "ftrl": 2}
for rule in [r for r in args.rule if r != "adagrad"]:
  p = torch.nn.Parameter(table.clone())
  p._tfrs_embedding = True
  opt = builders[rule](p)

  def update():
    p._tfrs_slices.append((ids, go))
    opt.step()

  update()
  times = {"adagrad": [], rule + " nt": [], rule + " no-nt": []}
  for _ in range(args.rounds):        # alternating: the three variants see the same neighbours on the machine
    times["adagrad"].append(window(adagrad, args.window))
    _lib.set_option("TFRS_SCATTER_NT", None)
    times[rule + " nt"].append(window(update, args.window))
    _lib.set_option("TFRS_SCATTER_NT", "0")
    times[rule + " no-nt"].append(window(update, args.window))
    _lib.set_option("TFRS_SCATTER_NT", None)
  t_ada = min(times["adagrad"])
  byts_ada = algorithmic_bytes(4)
  emit({"op": "sparse adagrad", "rows": n, "unique": uniq, "dim": d, "ms_windows": [round(t * 1e3, 4) for t in times["adagrad"]],
        "ms": t_ada * 1e3, "algorithmic_bytes": byts_ada, "frac_copy_ceiling": byts_ada / t_ada / ceiling})
  byts = algorithmic_bytes(2 * (1 + slots[rule]))
  for variant in (rule + " nt", rule + " no-nt"):
    t = min(times[variant])
    emit({"op": "sparse " + variant, "rows": n, "unique": uniq, "dim": d, "ms_windows": [round(x * 1e3, 4) for x in times[variant]],
          "ms": t * 1e3, "algorithmic_bytes": byts, "frac_copy_ceiling": byts / t / ceiling, "ratio_to_adagrad": t / t_ada})
  opt.close()
  del opt, p
  torch.cuda.empty_cache()
