"""Fuzz: ScaNN on hand-built indexes (tests/scann_handbuilt.py: leaf sizes around the scan's 32 / 128 / 4096-row
boundaries, empty leaves, any dim and block width) against the float64 restatement (tests/scann_restatement.py) within
the bound of include/tfrs_hip.h; with every leaf searched and every probed row re-ordered also exact equality with
BruteForce.  The search runs on the whole batch; the host restatement on as many of its queries as fit a budget.

    python tools/fuzz_scann.py [seed] [cases] [only_case]     (a bad case prints the line that rebuilds it)"""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from recommenders_amd.layers import factorized_top_k as ftk
from tests import scann_handbuilt as hb, scann_restatement as rs

LEAF_SIZES = [0, 1, 31, 33, 127, 128, 129, 1000, 4096, 4097, 12289]
HOST_BUDGET = 2e8      # probed rows x dims x queries the float64 restatement is evaluated on per case


def draw(seed: int, case: int) -> dict:
  rng = np.random.default_rng([seed, case])
  sizes = [int(rng.choice(LEAF_SIZES)) for _ in range(int(rng.integers(2, 41)))]
  k = int(rng.choice([1, 10, 100]))
  while sum(sizes) < k:
    sizes.append(1000)
  reorder = None if rng.integers(0, 2) == 0 else max(k, int(rng.choice([k, 200, 1024])))
  n = sum(sizes)
  planted = sorted({int(p): int(kind) for p, kind in zip(rng.integers(0, n, size=int(rng.integers(0, 2 * k + 9))),
                                                         rng.choice([14, 15], size=2 * k + 9))}.items())
  return dict(seed=seed, case=case, sizes=sizes, d=int(rng.integers(1, 129)), dpb=int(rng.integers(1, 9)),
              nq=int(rng.choice([1, 31, 33, 64, 300])), nls=int(rng.integers(1, len(sizes) + 1)), k=k, reorder=reorder,
              planted=planted, garbage=bool(rng.integers(0, 2)), build_seed=int(rng.integers(1 << 30)))


def run(p: dict) -> dict:
  """One case; raises AssertionError on a mismatch.  Returns what it measured."""
  built = hb.build_state(p["sizes"], p["d"], p["dpb"], p["build_seed"], p["planted"], rows=p["reorder"] is not None,
                         garbage=p["garbage"])
  state, c = built if p["reorder"] is not None else (built, None)
  q, _ = hb.queries(p["nq"], p["d"], p["dpb"], p["build_seed"] + 1)
  k, nls = p["k"], p["nls"]
  layer = hb.make_layer(state, k, nls, p["reorder"])
  l_eff, p_max = layer.probe_plan(k)
  s, rows = layer(q)
  s, rows = s.cpu().numpy(), rows.cpu().numpy()
  checked = int(min(p["nq"], max(1, HOST_BUDGET // (p_max * p["d"]))))
  sel = np.sort(np.random.default_rng(p["build_seed"]).permutation(p["nq"])[:checked])
  share = hb.check_against_restatement(layer, state, q[sel], k, nls, p["reorder"], s[sel], rows[sel], corpus=c)
  exact = l_eff == len(p["sizes"]) and p["reorder"] is not None and p["reorder"] >= p_max
  if exact:
    bs, bi = ftk.BruteForce(k=k).index(c)(q)
    np.testing.assert_array_equal(rows, bi.cpu().numpy())
    np.testing.assert_array_equal(s, bs.cpu().numpy())
  return dict(l_eff=l_eff, p_max=p_max, checked=checked, decided=round(share, 3), bruteforce=exact)


def main(seed: int = 0, cases: int = 30, only: int = -1) -> int:
  bad = 0
  for case in range(cases) if only < 0 else [only]:
    p = draw(seed, case)
    brief = {key: p[key] for key in ("case", "d", "dpb", "nq", "nls", "k", "reorder", "garbage")}
    brief.update(leaves=len(p["sizes"]), rows=sum(p["sizes"]), planted=len(p["planted"]))
    try:
      brief.update(run(p), ok=True)
    except AssertionError as e:
      bad += 1
      brief.update(ok=False, error=str(e)[:400], sizes=p["sizes"],
                   rebuild=f"python tools/fuzz_scann.py {seed} {cases} {case}")
    print(json.dumps(brief), flush=True)
  print("MISMATCHES", bad)
  return bad


if __name__ == "__main__":
  args = [int(a) for a in sys.argv[1:]]
  sys.exit(1 if main(*args) else 0)
