"""The in-batch softmax kernels (csrc/softmax.hip, csrc/softmax16.hip) where a wave streams SEVERAL tiles: the in-wave
rescale of the online softmax, the one-tile-ahead prefetch, the slab / ring rewrite between tiles, the per-row scale of
the split-fp16 backward and the batched finalize, on the hand-built batches of tests/softmax_handbuilt.py (every planted
property and every claimed split geometry is proved on the host by tests/test_softmax_handbuilt_host.py).  The split
geometry is steered in-process through ``_lib.set_option`` (the planners read their targets on every call); the kernels
are called through the C entry points, which also return the per-row ``lse`` and ``pos``.

Gates, all the project's own: loss 1e-5 relative; dq / dc of the f32 kernels GATE_SOFTMAX_GRAD["f32"] and of the
split-fp16 kernels GATE_SOFTMAX_MIXED, both in units of the oracle's own-terms yardsticks with no floor; the per-row loss
``lse - pos`` 3.5e-6 of 1 + A_bb + sum_c p_bc A_bc, A = |q| |c|^T / |T| (the ``cond`` of oracle/retrieval.py).  Observed
maxima on MI355X over every case of this file, in gate units (every check prints its own): f32 kernels loss 1.1e-7, row
loss 9.9e-7, dq 3.6e-7, dc 1.2e-6; split-fp16 kernels loss 1.3e-6, row loss 6.1e-7, dq 2.3e-7, dc 6.1e-7.

The staircase and ladder batches draw their noise from the grid WITHOUT 0 (softmax_handbuilt.nonzero_grid): the
split-fp16 backward keeps T under one scale per owned row over ~27 binades, so a gradient entry whose
large terms meet an exact 0 coordinate and whose only nonzero terms are 2^-80 of the row's largest is flushed (observed:
0 for 1e-27, 1e-2 of that entry's own yardstick) -- a documented limit, not what these cases are about."""

import numpy as np
import pytest

from oracle import retrieval as o_ret
from tests import multihead_restatement as mh
from tests import softmax_handbuilt as hb
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GATE_F32 = 3.5e-6       # tests/test_ops_gpu.py GATE_SOFTMAX_GRAD["f32"]
GATE_F16 = 4e-6         # tests/test_ops_gpu.py GATE_SOFTMAX_MIXED (own-terms yardstick, no floor)
GATE_ROW = 3.5e-6
LOSS_RTOL = 1e-5
ONE_SPLIT_F32 = {"TFRS_SOFTMAX_WAVES": "1"}
ONE_SPLIT_F16 = {"TFRS_SOFTMAX_WGS": "1", "TFRS_SOFTMAX_WGS_BWD": "1"}


def test_the_gates_are_the_projects():
  from tests import test_ops_gpu as ops
  assert (GATE_F32, GATE_F16) == (ops.GATE_SOFTMAX_GRAD["f32"], ops.GATE_SOFTMAX_MIXED)


def run(q, c, kw, mode, opts=None, reuse=1):
  """(loss, lse, dq, dc, pos) through the C entry points under ``opts``; ``mode`` "f32" forces the f32-MFMA kernels."""
  from recommenders_amd import _lib
  opts = dict(opts or {})
  if mode == "f32":
    opts["TFRS_SOFTMAX_MODE"] = "f32"
  try:
    for k, v in opts.items():
      _lib.set_option(k, v)
    return hb.entry_point_outputs(q, c, kw, multi_head=np.ndim(q) == 3, reuse=reuse, with_pos=True)
  finally:
    for k in opts:
      _lib.set_option(k, None)


def _oracle_kw(kw):
  return dict(kw, remove_accidental_hits_flag=True) if "candidate_ids" in kw else kw


_REFS = {}


def reference(key, q, c, kw):
  """(loss, dq, dc, dq yardstick, dc yardstick, per-row loss, its yardstick) of the float64 oracle, computed once per
  ``key`` and shared."""
  if key not in _REFS:
    if np.ndim(q) == 3:
      rows = (None, None)
      ref = (mh.loss(q, c, **kw),) + tuple(mh.loss_grads(q, c, return_yardsticks=True, **kw))
    else:
      rows = hb.row_losses(q, c, **kw)
      ref = (float(o_ret.loss(q, c, **_oracle_kw(kw))),) + tuple(
          o_ret.loss_grads(q, c, return_yardsticks=True, **_oracle_kw(kw)))
    _REFS[key] = ref + rows
  return _REFS[key]


def check(tag, q, c, kw, out, mode, key=None, row_check=True):
  """Holds one run to the gates; returns the observed (loss, row, dq, dc) errors."""
  loss, lse, dq, dc, pos = out
  ref, dq_ref, dc_ref, dq_y, dc_y, row_ref, row_y = reference(key or tag, q, c, kw)
  assert np.all(np.isfinite(dq)) and np.all(np.isfinite(dc)) and np.all(np.isfinite(lse)), tag
  e_loss = abs(float(loss) - ref) / max(abs(ref), 1e-30)
  e_row = 0.0
  if row_ref is not None and row_check:
    rows = np.flatnonzero(pos > hb.MIN_FLOAT / 2)       # a masked positive: lse and pos are both MIN_FLOAT (see F)
    e_row = float_gate("softmax_handbuilt.row_loss", lse[rows].astype(np.float64) - pos[rows].astype(np.float64),
                       row_ref[rows], row_y[rows], GATE_ROW)
  gate = GATE_F32 if mode == "f32" else GATE_F16
  e_dq = float_gate(f"softmax_handbuilt.{mode}.dq", dq, dq_ref, dq_y, gate)
  e_dc = float_gate(f"softmax_handbuilt.{mode}.dc", dc, dc_ref, dc_y, gate)
  print(f"{tag} [{mode}]: loss rel {e_loss:.3e}, row loss {e_row:.3e}, dq {e_dq:.3e}, dc {e_dc:.3e} (gate units)")
  assert e_loss <= LOSS_RTOL, (tag, float(loss), ref)
  return e_loss, e_row, e_dq, e_dc


# ------------------------------------------------------------------------------------------ A. streaming depth, f32
@pytest.mark.parametrize("waves,heads,shape", [case[:3] for case in hb.F32_DEPTH_CASES],
                         ids=lambda v: str(v).replace(" ", ""))
def test_f32_kernels_stream_several_tiles(waves, heads, shape):
  nq, nc, d = shape
  rng = np.random.default_rng([nq, nc, d, heads])
  q = hb.grid(rng, (nq, d) if heads == 1 else (nq, heads, d))
  c = hb.grid(rng, (nc, d))
  variants = hb.option_variants(rng, nq, nc)
  names = list(variants) if shape == (33, 70, 20) and heads == 1 else ["plain", "all"]
  opts = {} if waves is None else {"TFRS_SOFTMAX_WAVES": waves}
  for name in names:
    check(f"depth{shape}x{heads}/{name}", q, c, variants[name], run(q, c, variants[name], "f32", opts), "f32")


# ------------------------------------------------------------------------------------------ B. order of the maxima
@pytest.mark.parametrize("step", hb.STAIR_STEPS)
@pytest.mark.parametrize("kind", hb.STAIR_KINDS)
def test_staircases_within_one_split_and_across_splits(kind, step):
  nq, nc, d = hb.STAIR_SHAPE
  q, c, _, t = hb.staircase(nq, nc, d, kind, step)
  kw = dict(temperature=t)
  key = f"stair/{kind}/{step}"
  check(key + "/one split", q, c, kw, run(q, c, kw, "f32", ONE_SPLIT_F32), "f32", key)
  check(key + "/one split", q, c, kw, run(q, c, kw, "f16", ONE_SPLIT_F16), "f16", key)
  check(key + "/per-tile splits", q, c, kw, run(q, c, kw, "f32"), "f32", key)
  check(key + "/per-tile splits", q, c, kw, run(q, c, kw, "f16"), "f16", key)


# ------------------------------------------------------------------------------------------ C. streaming depth, fp16
@pytest.mark.parametrize("d", hb.F16_DEPTH_DIMS)
@pytest.mark.parametrize("shape", list(hb.F16_DEPTH_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_f16_kernels_stream_every_ring_residue(shape, d):
  nq, nc = shape
  rng = np.random.default_rng([nq, nc, d])
  q, c = hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))
  w = rng.uniform(0.1, 2.0, size=nq).astype(np.float32)
  for name, kw in (("plain", dict()), ("weights", dict(sample_weight=w, temperature=0.5))):
    for nw in ("4", "8"):
      out = run(q, c, kw, "f16", dict(ONE_SPLIT_F16, TFRS_SOFTMAX_NW=nw))
      check(f"ring{shape}x{d}/{name}/nw{nw}", q, c, kw, out, "f16", f"ring{shape}x{d}/{name}")


@pytest.mark.parametrize("shape", list(hb.F16_TWO_SPLIT_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_f16_kernels_with_two_splits(shape):
  nq, nc = shape
  d = 20
  rng = np.random.default_rng([nq, nc, d, 2])
  q, c = hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))
  kw = dict(sample_weight=rng.uniform(0.1, 2.0, size=nq).astype(np.float32), temperature=0.5)
  two = {"TFRS_SOFTMAX_WGS": "2", "TFRS_SOFTMAX_WGS_BWD": "2"}
  check(f"two splits{shape}", q, c, kw, run(q, c, kw, "f16", two), "f16")
  if shape == (70, 97):         # the backward rebuilds the operand records (what TFRS_SOFTMAX_NO_REUSE=1 asks for)
    check(f"two splits{shape}/no reuse", q, c, kw, run(q, c, kw, "f16", two, reuse=0), "f16", f"two splits{shape}")
    check(f"one split{shape}/no reuse", q, c, kw, run(q, c, kw, "f16", ONE_SPLIT_F16, reuse=0), "f16",
          f"two splits{shape}")


# ------------------------------------------------------------------------------------------ D. finalize in batches of 16
@pytest.mark.parametrize("shape", list(hb.FINALIZE_SHAPES), ids=lambda v: str(v).replace(" ", ""))
def test_finalize_with_the_maximum_on_either_side_of_a_batch_boundary(shape):
  nq, nc, d = shape
  for at in hb.finalize_plants(hb.FINALIZE_SHAPES[shape]):
    q, c, _, t = hb.staircase(nq, nc, d, at, hb.FINALIZE_GAP)
    kw = dict(temperature=t)
    check(f"finalize{shape}/max in split {at}", q, c, kw, run(q, c, kw, "f16"), "f16")


# ------------------------------------------------------------------------------------------ E. numeric edges, fp16
EDGE_SHAPES = ((70, 97, 20), (40, 225, 64))


def _edge_batch(shape):
  nq, nc, d = shape
  rng = np.random.default_rng([nq, nc, d, 5])
  return rng, hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_power_of_two_shifts_leave_the_forward_bit_identical(shape):
  rng, q, c = _edge_batch(shape)
  kw = dict(sample_weight=rng.uniform(0.1, 2.0, size=shape[0]).astype(np.float32))
  for mode in ("f16", "f32"):
    base = run(q, c, kw, mode)
    check(f"shift{shape}/0", q, c, kw, base, mode, f"shift{shape}/0")
    for k in (-60, -20, 20, 60):
      qk, ck = q * np.float32(2.0 ** k), c * np.float32(2.0 ** -k)
      out = run(qk, ck, kw, mode)
      for what, a, b in zip(("loss", "lse", "pos"), (out[0], out[1], out[4]), (base[0], base[1], base[4])):
        np.testing.assert_array_equal(a, b, err_msg=f"{shape}/{mode}/2^{k}/{what}")
      check(f"shift{shape}/{k}", qk, ck, kw, out, mode)


@pytest.mark.parametrize("side", ("q", "c"))
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_scale_ladder_inside_one_record(shape, side):
  """Row r of the second 32-row record is scaled by 2^-r; sample weights of 10^4 and 10^-4 sit in the same record."""
  rng, q, c = _edge_batch(shape)
  ladder = np.float32(2.0) ** -np.arange(32, dtype=np.float32)
  x = q if side == "q" else c
  x[32:64] *= ladder[:len(x[32:64]), None]                # (40 queries: the record's 8 rows)
  w = np.ones(shape[0], np.float32)
  w[33:shape[0]:5] = 1e4
  w[35:shape[0]:5] = 1e-4
  kw = dict(sample_weight=w)
  check(f"ladder{shape}/{side}", q, c, kw, run(q, c, kw, "f16"), "f16")


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_weights_over_eighty_binades_and_zero_weights(shape):
  rng, q, c = _edge_batch(shape)
  nq = shape[0]
  values = np.array([0.0, 2.0 ** -40, 2.0 ** -13, 1.0, 3.0, 2.0 ** 13, 1.5 * 2.0 ** 40], np.float32)
  w = np.ones(nq, np.float32)
  w[:32] = values[np.arange(32) % len(values)]            # the whole range within the first record
  kw = dict(sample_weight=w)
  out = run(q, c, kw, "f16")
  check(f"weights{shape}/range", q, c, kw, out, "f16")
  assert np.all(out[2][w == 0.0] == 0.0)
  w = rng.uniform(0.5, 2.0, size=nq).astype(np.float32)
  w[32:64] = 0.0                                          # a whole record of zero weights
  kw = dict(sample_weight=w, temperature=0.5)
  out = run(q, c, kw, "f16")
  check(f"weights{shape}/zero record", q, c, kw, out, "f16")
  assert np.all(out[2][32:64] == 0.0) and np.abs(out[2][:32]).sum() > 0


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_zero_rows_zero_records_and_rows_below_the_flush(shape):
  nq, nc, d = shape
  for name in ("q record", "c record", "single rows", "all-zero q", "tiny rows"):
    _, q, c = _edge_batch(shape)
    if name == "q record":
      q[32:64] = 0.0
    elif name == "c record":
      c[32:64] = 0.0
    elif name == "single rows":
      q[3] = 0.0
      c[nc - 1] = 0.0
    elif name == "all-zero q":
      q[:] = 0.0
    else:       # below the 2^-100 under which the split-fp16 path takes a row as zero: the oracle's difference is 2^-110
      q[5] *= np.float32(2.0 ** -110)
      c[nc - 2] *= np.float32(2.0 ** -110)
    out = run(q, c, dict(), "f16")
    check(f"zeros{shape}/{name}", q, c, dict(), out, "f16")
    if name == "all-zero q":
      assert np.all(out[3] == 0.0)


def test_ladders_of_the_backwards_per_row_scale():
  """|G| of an owned row grows (shrinks) by at least 2^3 from one streamed tile to the next: the per-row scale of the
  T tile is lowered -- and the accumulators rescaled -- on every tile (only on the first)."""
  for kind in ("ascending", "descending"):
    q, c, _, t = hb.staircase(161, 161, 16, kind)
    for opts in (ONE_SPLIT_F16, {}):
      check(f"dq ladder/{kind}/{len(opts)}", q, c, dict(), run(q, c, dict(), "f16", opts), "f16", f"dq ladder/{kind}")
  for ascending in (True, False):
    q, c, _ = hb.column_ladder(129, 161, 16, ascending)
    for opts in (ONE_SPLIT_F16, {}):
      check(f"dc ladder/{ascending}/{len(opts)}", q, c, dict(), run(q, c, dict(), "f16", opts), "f16",
            f"dc ladder/{ascending}")


# ------------------------------------------------------------------------------------------ F. option semantics, f32
F_SHAPE = (33, 70, 20)


@pytest.mark.parametrize("weight", (0.0, 1.0))
def test_fully_masked_row(weight):
  """A query whose score_mask is all False: every logit is MIN_FLOAT, the softmax is uniform and the row's loss is
  log(nc) (the reference subtracts the row maximum first), its gradients are exactly 0.  ``lse`` and ``pos`` of that row
  are both MIN_FLOAT -- their difference says nothing -- so the row's loss is read from the loss under a one-hot
  weight."""
  nq, nc, d = F_SHAPE
  rng = np.random.default_rng([nq, nc, d, 6])
  q, c = hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))
  mask = rng.uniform(size=(nq, nc)) > 0.2
  mask[np.arange(nq), np.arange(nq)] = True
  masked_rows = (4, 32)                                 # one per row block
  w = rng.uniform(0.5, 2.0, size=nq).astype(np.float32)
  for r in masked_rows:
    mask[r] = False
    w[r] = weight
  kw = dict(score_mask=mask, sample_weight=w)
  out = run(q, c, kw, "f32", ONE_SPLIT_F32)
  check(f"masked row/w={weight}", q, c, kw, out, "f32")
  assert np.all(out[2][list(masked_rows)] == 0.0)
  row_ref, row_y = hb.row_losses(q, c, score_mask=mask)
  for r in masked_rows:
    assert row_ref[r] == pytest.approx(np.log(nc), rel=1e-12)
    one_hot = np.zeros(nq, np.float32)
    one_hot[r] = 1.0
    alone = run(q, c, dict(score_mask=mask, sample_weight=one_hot), "f32", ONE_SPLIT_F32)
    print(f"fully masked row {r}: loss under a one-hot weight {float(alone[0])!r}, oracle {row_ref[r]!r}")
    float_gate("softmax_handbuilt.row_loss", np.float64(alone[0]), row_ref[r], row_y[r], GATE_ROW)
    assert np.all(alone[3] == 0.0)                      # the only weighted row has G = 0


def test_all_negatives_removed():
  """Every candidate shares one id: each row's negatives are all accidental hits, its loss is 0 and G = 0."""
  nq, nc, d = F_SHAPE
  rng = np.random.default_rng([nq, nc, d, 7])
  q, c = hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))
  kw = dict(candidate_ids=np.full(nc, 7, np.int64), temperature=0.5)
  assert float(o_ret.loss(q, c, **_oracle_kw(kw))) == 0.0
  loss, lse, dq, dc, pos = run(q, c, kw, "f32", ONE_SPLIT_F32)
  assert float(loss) == 0.0 and np.array_equal(lse, pos)
  assert np.all(dq == 0.0) and np.all(dc == 0.0)


def test_duplicates_of_a_positives_id_in_other_tiles():
  nq, nc, d = F_SHAPE
  rng = np.random.default_rng([nq, nc, d, 8])
  q, c = hb.grid(rng, (nq, d)), hb.grid(rng, (nc, d))
  ids = np.arange(nc, dtype=np.int64) + 100
  ids[40:45] = ids[3]          # positive in tile 0, duplicates in tile 1
  ids[66:70] = ids[32]         # positive in tile 1, duplicates in the ragged tile 2
  ids[64] = ids[31]            # ... and one across two tile boundaries
  ids[10] = ids[33]            # row 10's positive takes the id of candidate 33, no query's positive, in tile 1
  assert all(ids[a] == ids[b] and a // 32 != b // 32 for a, b in ((40, 3), (66, 32), (64, 31), (10, 33)))
  kw = dict(candidate_ids=ids)
  check("duplicates across tiles", q, c, kw, run(q, c, kw, "f32", ONE_SPLIT_F32), "f32")
  kw = dict(candidate_ids=ids, sample_weight=rng.uniform(0.1, 2.0, size=nq).astype(np.float32), temperature=0.7)
  check("duplicates across tiles/weights", q, c, kw, run(q, c, kw, "f32", ONE_SPLIT_F32), "f32")
