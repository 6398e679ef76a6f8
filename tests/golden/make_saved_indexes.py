"""Writes tests/golden/saved_*.npz: indexes saved by ``BruteForce.save`` / ``ScaNN.save`` next to the queries and
the ``(scores, identifiers)`` the saving layer returned for them.  Needs an MI355X.

The committed files were written at commit ae8dfb5, the last one in which ``factorized_top_k`` was a single module:
``test_saved_indexes_load_across_versions`` (tests/test_topk_gpu.py) loads them with the current code, so they are
NOT to be regenerated when the layers change -- a file format change has to keep them readable.

Run:  python tests/golden/make_saved_indexes.py [output directory]
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(out):
  from recommenders_amd.layers import factorized_top_k as ftk
  rng = np.random.default_rng(2026)
  d = 16
  q = rng.normal(size=(8, d)).astype(np.float32)
  c = rng.normal(size=(300, d)).astype(np.float32)
  cases = {
      "bruteforce": ftk.BruteForce(k=10).index(c, np.array([f"item-{i}" for i in range(len(c))])),
      "scann": ftk.ScaNN(k=10, num_leaves=8, num_leaves_to_search=3, num_reordering_candidates=50,
                         seed=3).index(c, (np.arange(len(c)) * 7 + 1).astype(np.int64)),
      "scann_noreorder": ftk.ScaNN(k=5, num_leaves=6, num_leaves_to_search=2, dimensions_per_block=3).index(c),
  }
  expected = {"queries": q}
  for name, layer in cases.items():
    layer.save(os.path.join(out, f"saved_{name}.npz"))
    scores, ids = layer(q)
    expected[f"{name}_scores"] = scores.cpu().numpy()
    expected[f"{name}_identifiers"] = ids.cpu().numpy() if hasattr(ids, "cpu") else np.asarray(ids)
  np.savez(os.path.join(out, "saved_expected.npz"), **expected)


if __name__ == "__main__":
  main(sys.argv[1] if len(sys.argv) > 1 else HERE)
