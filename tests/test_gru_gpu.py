"""GPU tests of layers.GRU and the recurrence kernels of csrc/gru.hip against the float64 restatement
of tests/gru_restatement.py: values and gradients through float_gate, the bit-exact halving test, bitwise invariants,
training with capture, and the envelope."""

import functools

import numpy as np
import pytest
import torch

from tests import gru_restatement as G
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

_ids = lambda c: f"B{c.B}-T{c.T}-E{c.E}-U{c.U}-{c.mask}-{''.join('1' if o else '0' for o in c.opts)}"


def _t(a, grad=False):
  if a is None:
    return None
  t = torch.as_tensor(np.asarray(a)).cuda()
  return t.requires_grad_(True) if grad else t


def _np(t):
  return t.detach().cpu().numpy()


def _same_bits(a, b):
  a, b = _np(a), _np(b)
  return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _reference(case):
  d = G.make_inputs(case)
  return d, G.restate(case, d)


def _layer(case_or_units, d, **opts):
  from recommenders_amd.layers import GRU
  if isinstance(case_or_units, G.Case):
    seq, state, backwards, _, with_bias = case_or_units.opts
    layer = GRU(case_or_units.U, return_sequences=seq, return_state=state, go_backwards=backwards,
                use_bias=with_bias)
  else:
    layer = GRU(case_or_units, use_bias=d["bias"] is not None, **opts)
  layer.set_weights([d["kernel"], d["recurrent_kernel"]] + ([d["bias"]] if d["bias"] is not None else []))
  return layer


def _run(layer, d, x=None, h0=None):
  """The layer on the inputs of `d`: (seq or None, last or None) as the options return them."""
  x = _t(d["x"]) if x is None else x
  h0 = _t(d["h0"]) if h0 is None else h0
  out = layer(x, mask=_t(d["mask"]), initial_state=h0)
  if layer.return_sequences:
    return (out[0], out[1]) if layer.return_state else (out, None)
  return None, (out[1] if layer.return_state else out)


# ---- 1. values and gradients against the restatement ---------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=_ids)
def test_values_and_gradients_against_the_restatement(case):
  """Every returned tensor and every gradient of the loss sum(wseq * seq) + sum(wlast * last), entry by entry against
  float64 in the restatement's yardstick (the sum of |terms| of the entry, gru_restatement's docstring).  The limit of
  a gate is 4 x the ratio the float32 CPU recurrence shows for that gate on the inputs of THIS case, and never below
  4 x ALLOWANCE_FLOOR (G.limits(case)); tests/test_gru_host.py shows that a zeroed or 1 %-off result fails every case."""
  d, ref = _reference(case)
  limit = G.limits(case)
  layer = _layer(case, d)
  x, h0 = _t(d["x"], True), _t(d["h0"], True)
  seq, last = _run(layer, d, x, h0)
  seq_opt, state_opt = case.opts[0], case.opts[1]
  assert (seq is not None) == seq_opt and (last is not None) == (state_opt or not seq_opt)
  if seq_opt and state_opt:
    assert _same_bits(seq[:, -1], last)                    # the last state IS the last output
  loss = 0.0
  if seq is not None:
    assert tuple(seq.shape) == (case.B, case.T, case.U)
    loss = loss + (seq * _t(d["wseq"])).sum()
  if last is not None:
    assert tuple(last.shape) == (case.B, case.U)
    loss = loss + (last * _t(d["wlast"])).sum()
  loss.backward()
  got = {"seq": seq, "last": last, "dx": x.grad, "dh0": None if h0 is None else h0.grad,
         "dkernel": layer.kernel.grad, "drecurrent": layer.recurrent_kernel.grad,
         "dbias": None if layer.bias is None else layer.bias.grad}
  failures = []
  for key, value in got.items():
    if value is None:
      continue
    name = G.GATES[key]
    try:
      err = float_gate(name, _np(value), ref[key].value, ref[key].yard, limit[name], floor=G.FLOOR)
      print(f"{name}: observed {err / G.EPS:.2f} eps, limit {limit[name] / G.EPS:.2f} eps")
    except AssertionError as e:
      failures.append(str(e))
  assert not failures, failures


# ---- 2. the halving test ---------------------------------------------------------------------------------------------
def _guarded(shape, fill=float("nan")):
  """A tensor carved out of a NaN-filled buffer with 64 sentinel floats on either side: (view, buffer)."""
  n = int(np.prod(shape))
  buf = torch.full((n + 128,), fill, dtype=torch.float32, device="cuda")
  return buf[64:64 + n].view(*shape), buf


def _guards_intact(buf):
  return bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())


@pytest.mark.parametrize("U", G.UNITS)
@pytest.mark.parametrize("B", G.BATCHES)
def test_halving_counts_steps_masks_and_padding_bit_for_bit(B, U):
  """kernel, recurrent_kernel and bias all zero: z = 1/2 and hh = 0 exactly, h_t = h_{t-1} / 2 (proven step by step in
  tests/test_gru_host.py).  With small distinct integers as initial state the layer must return
  initial_state * 2^-(unmasked steps of the row so far) under ==, at every step of the sequence (a repeat at masked
  steps) and as last state, for every mask pattern and both directions: a miscounted loop, a mask read for the wrong
  row or step, or a padding lane / column leaking into a live one shows as a wrong bit.  The second half calls the two
  entry points on buffers with NaN sentinels around every output, which must stay untouched."""
  from recommenders_amd import _lib
  from recommenders_amd.layers import GRU
  T, E = 9, 3
  rng = np.random.default_rng(100 * B + U)
  x = _t(rng.normal(size=(B, T, E)).astype(np.float32))
  h0 = G.halving_state(B, U)
  zeros = [np.zeros((E, 3 * U), np.float32), np.zeros((U, 3 * U), np.float32), np.zeros((2, 3 * U), np.float32)]
  lib = _lib.load()
  for kind in G.MASKS:
    m = G.make_mask(kind, B, T, rng)
    for backwards in (False, True):
      want_seq, want_last = G.halving_expected(h0, m, T, backwards)
      layer = GRU(U, return_sequences=True, return_state=True, go_backwards=backwards)
      layer.set_weights(zeros)
      with torch.no_grad():
        seq, last = layer(x, mask=_t(m), initial_state=_t(h0))
      assert np.array_equal(_np(seq), want_seq), (kind, backwards)
      assert np.array_equal(_np(last), want_last), (kind, backwards)
      last_only = GRU(U, go_backwards=backwards)
      last_only.set_weights(zeros)
      with torch.no_grad():
        assert np.array_equal(_np(last_only(x, mask=_t(m), initial_state=_t(h0))), want_last), (kind, backwards)
      # the entry points on guarded buffers (xproj = x @ 0 + 0 = 0)
      xp = torch.zeros((B, T, 3 * U), dtype=torch.float32, device="cuda")
      rk = torch.zeros((U, 3 * U), dtype=torch.float32, device="cuda")
      mask_t, h0_t = _t(m), _t(h0)
      outs = [_guarded((B, T, U)), _guarded((B, U))] + [_guarded((B, T, U)) for _ in range(5)]
      _lib.check(lib.tfrs_gru_fwd(_lib.ptr(xp), _lib.ptr(rk), None, _lib.ptr(mask_t), _lib.ptr(h0_t), B, T, U,
                                  1 if backwards else 0, *[_lib.ptr(o[0]) for o in outs], _lib.current_stream()))
      assert np.array_equal(_np(outs[0][0]), want_seq) and np.array_equal(_np(outs[1][0]), want_last)
      assert all(_guards_intact(o[1]) for o in outs), (kind, backwards)
      assert not any(bool(torch.isnan(o[0]).any()) for o in outs)          # every live element was written
      dseq = _t(rng.normal(size=(B, T, U)).astype(np.float32))
      grads = [_guarded((B, T, 3 * U)), _guarded((B, T, 3 * U)), _guarded((B, U))]
      _lib.check(lib.tfrs_gru_bwd(_lib.ptr(rk), _lib.ptr(mask_t), *[_lib.ptr(o[0]) for o in outs[2:]],
                                  _lib.ptr(dseq), None, B, T, U, 1 if backwards else 0,
                                  *[_lib.ptr(g[0]) for g in grads], _lib.current_stream()))
      assert all(_guards_intact(g[1]) for g in grads), (kind, backwards)
      assert not any(bool(torch.isnan(g[0]).any()) for g in grads)
      if m is not None:                                                    # a masked step writes zeros to both
        dead = _t(~m)
        assert not bool(grads[0][0][dead].any()) and not bool(grads[1][0][dead].any())


# ---- 3. bitwise invariants on random weights -------------------------------------------------------------------------
def _random_case(B, T, E, U, mask, seed, opts=(True, True, False, True, True)):
  case = G.Case(B, T, E, U, mask, opts, seed)
  return case, G.make_inputs(case)


@pytest.mark.parametrize("U", (9, 33, 64))
def test_a_row_of_a_batch_equals_the_row_run_alone(U):
  case, d = _random_case(65, 9, 33, U, "holes", 7)
  layer = _layer(U, d, return_sequences=True, return_state=True)
  with torch.no_grad():
    seq, last = _run(layer, d)
    for b in (0, 31, 32, 64):
      one = {k: (v[b:b + 1] if k in ("x", "mask", "h0") else v) for k, v in d.items()}
      s1, l1 = _run(layer, one)
      assert _same_bits(seq[b:b + 1], s1) and _same_bits(last[b:b + 1], l1), b


@pytest.mark.parametrize("U", (9, 33, 64))
def test_go_backwards_equals_the_forward_layer_on_flipped_inputs(U):
  case, d = _random_case(33, 9, 33, U, "holes", 8)
  back = _layer(U, d, return_sequences=True, return_state=True, go_backwards=True)
  fwd = _layer(U, d, return_sequences=True, return_state=True)
  flipped = dict(d, x=d["x"][:, ::-1].copy(), mask=d["mask"][:, ::-1].copy())
  with torch.no_grad():
    sb, lb = _run(back, d)
    sf, lf = _run(fwd, flipped)
  assert _same_bits(sb, sf) and _same_bits(lb, lf)


@pytest.mark.parametrize("U", (9, 33, 64))
def test_a_right_padded_row_equals_the_row_truncated_to_its_length(U):
  case, d = _random_case(33, 9, 33, U, "right", 9)
  layer = _layer(U, d)
  lengths = d["mask"].sum(axis=1)
  with torch.no_grad():
    _, last = _run(layer, d)
    for b in (1, 2, 4, 32):
      n = int(lengths[b])
      assert 0 < n <= 9
      one = dict(d, x=d["x"][b:b + 1, :n], mask=None, h0=d["h0"][b:b + 1])
      _, l1 = _run(layer, one)
      assert _same_bits(last[b:b + 1], l1), (b, n)
    dead = np.nonzero(lengths == 0)[0]
    assert len(dead) and _same_bits(last[dead], _t(d["h0"][dead]))        # masked everywhere: the initial state


@pytest.mark.parametrize("U", (9, 33, 64))
def test_two_runs_are_identical_and_masked_steps_give_plus_zero(U):
  """No float atomics anywhere: forward and every gradient repeat bit for bit; the input gradient of a masked step
  is +0 exactly (da = +0 there, and a product's fma chain over zeros starting at +0 stays +0)."""
  case, d = _random_case(65, 9, 33, U, "holes", 10)
  runs = []
  for _ in range(2):
    layer = _layer(U, d, return_sequences=True, return_state=True)
    x, h0 = _t(d["x"], True), _t(d["h0"], True)
    seq, last = _run(layer, d, x, h0)
    ((seq * _t(d["wseq"])).sum() + (last * _t(d["wlast"])).sum()).backward()
    runs.append([seq, last, x.grad, h0.grad, layer.kernel.grad, layer.recurrent_kernel.grad, layer.bias.grad])
  for a, b in zip(*runs):
    assert _same_bits(a, b)
  dx = _np(runs[0][2])
  dead = ~d["mask"]
  assert dead.any() and np.all(dx[dead].view(np.uint32) == 0)
  assert np.any(dx[d["mask"]] != 0)


# ---- 4. training and capture -----------------------------------------------------------------------------------------
def _tower(tfrs, seed=3):
  class Sequential(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.embedding = tfrs.layers.Embedding(50, 16, mask_zero=True)
      self.gru = tfrs.layers.GRU(32)
      self.gru.build(16, "cuda")
      self.candidates = tfrs.layers.Embedding(40, 32)
      self.task = tfrs.tasks.Retrieval()

    def query(self, ids):
      e = self.embedding(ids)
      return self.gru(e, mask=self.embedding.compute_mask(ids))

    def compute_loss(self, features, training=False):
      return self.task(self.query(features["history"]), self.candidates(features["movie_id"]),
                       compute_metrics=False)

  torch.manual_seed(seed)
  m = Sequential()
  m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.5))
  return m


def _history_batch(rng, B=64, T=9):
  hist = rng.integers(1, 50, size=(B, T))
  lengths = rng.integers(1, T + 1, size=B)
  hist[np.arange(T)[None, :] >= lengths[:, None]] = 0                    # right-padded with the mask id
  return {"history": _t(hist), "movie_id": _t(rng.integers(0, 40, size=B))}


def test_tower_trains_and_the_captured_step_matches_the_eager_one():
  """Embedding(mask_zero=True) -> GRU(32) under tasks.Retrieval with the project's Adagrad at B = 64, T = 9: three
  steps lower the loss, and the same three steps replayed from a captured graph leave bitwise equal parameters."""
  import recommenders_amd as tfrs
  batch = _history_batch(np.random.default_rng(11))
  eager, graphed = _tower(tfrs), _tower(tfrs)
  for a, b in zip(eager.parameters(), graphed.parameters()):
    assert _same_bits(a, b)
  assert len(list(eager.parameters())) == 5
  step = graphed.make_graphed_train_step(batch)
  for a, b in zip(eager.parameters(), graphed.parameters()):               # the capture's warm-up is rolled back
    assert _same_bits(a, b)
  before = [p.detach().clone() for p in eager.parameters()]
  losses = []
  for _ in range(3):
    le = eager.train_step(batch)
    lg = step(batch)
    losses.append(float(le["loss"]))
    assert float(lg["loss"]) == losses[-1]
  assert losses[2] < losses[1] < losses[0], losses
  for a, b in zip(eager.parameters(), graphed.parameters()):
    assert _same_bits(a, b)
  assert all(not _same_bits(a, b) for a, b in zip(before, eager.parameters()))     # every weight was trained


def test_loaded_weights_reproduce_the_restatement():
  """The tutorial tower in three lines, on weights loaded with set_weights (Keras' order and shapes)."""
  import recommenders_amd as tfrs
  rng = np.random.default_rng(12)
  B, T, E, U = 33, 9, 16, 32
  table = rng.normal(size=(50, E)).astype(np.float32)
  ids = rng.integers(0, 50, size=(B, T))
  ids[:, 0] = 0
  case = G.Case(B, T, E, U, "none", G.OPTIONS[0], 12)
  d = G.make_inputs(case)
  emb = tfrs.layers.Embedding(50, E, mask_zero=True)
  with torch.no_grad():
    emb.embeddings.copy_(_t(table))
  gru = tfrs.layers.GRU(U)
  gru.set_weights([d["kernel"], d["recurrent_kernel"], d["bias"]])
  ids_t = _t(ids)
  with torch.no_grad():
    e = emb(ids_t)
    h = gru(e, mask=emb.compute_mask(ids_t))
  ref = G.gru(table[ids], d["kernel"], d["recurrent_kernel"], d["bias"], ids != 0)
  tower = dict(d, x=table[ids], mask=ids != 0, h0=None, wseq=None, wlast=None)
  cpu = G.ratio(G.torch_recurrence(tower, False, torch.float32)["last"], ref["last"])      # the allowance, same inputs
  float_gate("gru.fwd.last", _np(h), ref["last"].value, ref["last"].yard, 4.0 * max(cpu, G.ALLOWANCE_FLOOR),
             floor=G.FLOOR)
  for got, want in zip(gru.get_weights(), (d["kernel"], d["recurrent_kernel"], d["bias"])):
    assert np.array_equal(got, want)


# ---- 5. envelope -----------------------------------------------------------------------------------------------------
def test_units_above_the_envelope_raise_before_any_launch():
  from recommenders_amd import _lib
  from recommenders_amd.layers import GRU
  for units in (65, 129):
    with pytest.raises(NotImplementedError, match="units"):
      GRU(units)
  # ... and the entry points themselves refuse, pointers unread
  lib = _lib.load()
  with pytest.raises(NotImplementedError, match="units"):
    _lib.check(lib.tfrs_gru_fwd(None, None, None, None, None, 4, 3, 65, 0, None, None, None, None, None, None,
                                None, _lib.current_stream()))
  with pytest.raises(NotImplementedError, match="units"):
    _lib.check(lib.tfrs_gru_bwd(None, None, None, None, None, None, None, None, None, 4, 3, 65, 0, None, None,
                                None, _lib.current_stream()))
  torch.cuda.synchronize()


@pytest.mark.parametrize("B,T", [(0, 9), (4, 0), (0, 0)])
def test_empty_batches(B, T):
  """An empty batch (or no time steps) returns correctly shaped outputs without a launch; the weight gradients of an
  empty batch are zeros, and with no step the state is the initial one."""
  from recommenders_amd.layers import GRU
  E, U = 5, 9
  layer = GRU(U, return_sequences=True, return_state=True)
  layer.build(E, "cuda")
  x = torch.zeros((B, T, E), device="cuda", requires_grad=True)
  h0 = torch.full((B, U), 0.5, device="cuda", requires_grad=True)
  mask = torch.ones((B, T), dtype=torch.bool, device="cuda")
  seq, last = layer(x, mask=mask, initial_state=h0)
  assert tuple(seq.shape) == (B, T, U) and tuple(last.shape) == (B, U)
  assert _same_bits(last, h0)
  (seq.sum() + (2.0 * last).sum()).backward()
  assert tuple(x.grad.shape) == (B, T, E)
  for p in layer.parameters():
    assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape) and not bool(p.grad.any())
  assert np.array_equal(_np(h0.grad), np.full((B, U), 2.0, np.float32))
