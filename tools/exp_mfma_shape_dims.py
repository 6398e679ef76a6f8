"""The two MFMA shapes of the fp16 scan kernels (TFRS_SCAN16_MFMA = 32x32 | 16x16) at dims 128 / 32 / 64, alternating
inside one process on one index: whole-call time (HIP events around each call: median, p10, p90 of 50 calls after 10
warm-up calls, three alternations) and the filter pass per launch.  Decides the per-dim default of
scan16_default_mfma() in csrc/topk_scan16.hip (profiles/scan16_mfma_shape_ab.txt).  `--series` also prints every
call's time in order (how the clock settles within a run)."""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from recommenders_amd import _lib
from recommenders_amd.layers import factorized_top_k as ftk
dev = torch.device("cuda", 0)
lib = _lib.load()
series = "--series" in sys.argv
dims = [int(a) for a in sys.argv[1:] if a.isdigit()] or [128, 32, 64]
rows, nq = 1_000_000, 8192
g = torch.Generator(device=dev).manual_seed(1)
for d in dims:
  corpus = torch.randn((rows, d), generator=g, device=dev) / d ** 0.5
  index = ftk.BruteForce(k=100).index(corpus)
  q = torch.randn((nq, d), generator=g, device=dev) / d ** 0.5
  ref = None
  for rep in range(3):
    for arm in ("32x32", "16x16"):
      _lib.set_option("TFRS_SCAN16_MFMA", arm)
      for _ in range(10):
        out = index(q)
      torch.cuda.synchronize()
      if ref is None:
        ref = (out[0].clone(), out[1].clone())
      same = bool(torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]))
      ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
      lib.tfrs_profile_read(None, None, None)
      lib.tfrs_profile_enable(1)
      for a, b in ev:
        a.record()
        index(q)
        b.record()
      torch.cuda.synchronize()
      kinds = {}
      for kind in (1, 2):
        ms, n, fl = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        lib.tfrs_profile_read_kind(kind, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
        kinds[kind] = ms.value / max(n.value, 1)
      lib.tfrs_profile_read(None, None, None)
      lib.tfrs_profile_enable(0)
      _lib.set_option("TFRS_SCAN16_MFMA", None)
      t = [a.elapsed_time(b) for a, b in ev]
      s = sorted(t)
      line = {"dim": d, "rows": rows, "nq": nq, "mfma": arm, "rep": rep, "call_ms_median": round(s[25], 4),
              "call_ms_p10": round(s[5], 4), "call_ms_p90": round(s[44], 4), "filter_ms": round(kinds[1], 4),
              "threshold_ms": round(kinds[2], 4), "redo": index.last_redo_count(), "same": same}
      if series:
        line["series"] = [round(x, 3) for x in t]
      print(json.dumps(line), flush=True)
  del index, corpus
  torch.cuda.empty_cache()
