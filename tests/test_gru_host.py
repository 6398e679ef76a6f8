"""Host-side tests of the GRU layer: the float64 restatement pinned against torch.nn.GRU, the layer's
constructor, initialisers and weight plumbing, and the exactness arguments the GPU tests rely on.  No GPU."""

import os

import numpy as np
import pytest
import torch

from tests import gru_restatement as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNMASKED = [c for c in G.CASES if c.mask in ("none", "all_true")]
MASKED = [c for c in G.CASES if c.mask not in ("none", "all_true")]


def _close(got, want, what):
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  err = float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if got.size else 0.0
  assert err <= 1e-12, (what, err)


def _torch_gru(d, U, E):
  """torch.nn.GRU in float64 carrying the Keras weights of `d`: gate blocks z, r, h -> r, z, n."""
  with_bias = d["bias"] is not None
  net = torch.nn.GRU(E, U, batch_first=True, bias=with_bias).double()
  perm = lambda a: np.concatenate([a[..., U:2 * U], a[..., :U], a[..., 2 * U:]], axis=-1)
  with torch.no_grad():
    net.weight_ih_l0.copy_(torch.tensor(perm(d["kernel"].astype(np.float64)).T))
    net.weight_hh_l0.copy_(torch.tensor(perm(d["recurrent_kernel"].astype(np.float64)).T))
    if with_bias:
      net.bias_ih_l0.copy_(torch.tensor(perm(d["bias"][0].astype(np.float64))))
      net.bias_hh_l0.copy_(torch.tensor(perm(d["bias"][1].astype(np.float64))))
  return net


def _unperm(a, U):
  """torch's r, z, n column blocks back to z, r, h."""
  return np.concatenate([a[..., U:2 * U], a[..., :U], a[..., 2 * U:]], axis=-1)


def _grad(t):
  """t.grad as an array; zeros where the loss does not depend on t (a batch masked everywhere)."""
  return np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()


def _torch_grads(net, U, with_bias):
  out = {"dkernel": _unperm(_grad(net.weight_ih_l0).T, U), "drecurrent": _unperm(_grad(net.weight_hh_l0).T, U)}
  if with_bias:
    out["dbias"] = np.stack([_unperm(_grad(net.bias_ih_l0), U), _unperm(_grad(net.bias_hh_l0), U)])
  return out


@pytest.mark.parametrize("case", UNMASKED, ids=lambda c: f"B{c.B}-T{c.T}-E{c.E}-U{c.U}-{c.mask}")
def test_restatement_equals_torch_gru_float64(case):
  d = G.make_inputs(case)
  ref = G.restate(case, d)
  B, T, E, U = case.B, case.T, case.E, case.U
  backwards = case.opts[2]
  net = _torch_gru(d, U, E)
  x = torch.tensor(d["x"].astype(np.float64), requires_grad=True)
  h0 = None if d["h0"] is None else torch.tensor(d["h0"].astype(np.float64), requires_grad=True)
  seq, last = net(x.flip(1) if backwards else x, None if h0 is None else h0[None])
  last = last[0]
  _close(seq.detach().numpy(), ref["seq"].value, "seq")
  _close(last.detach().numpy(), ref["last"].value, "last")
  loss = 0.0
  if d["wseq"] is not None:
    loss = loss + (seq * torch.tensor(d["wseq"].astype(np.float64))).sum()
  if d["wlast"] is not None:
    loss = loss + (last * torch.tensor(d["wlast"].astype(np.float64))).sum()
  loss.backward()
  _close(_grad(x), ref["dx"].value, "dx")
  if h0 is not None:
    _close(_grad(h0), ref["dh0"].value, "dh0")
  for k, v in _torch_grads(net, U, d["bias"] is not None).items():
    _close(v, ref[k].value, k)


@pytest.mark.parametrize("case", MASKED, ids=lambda c: f"B{c.B}-T{c.T}-E{c.E}-U{c.U}-{c.mask}")
def test_masked_restatement_equals_a_per_row_loop_over_the_valid_steps(case):
  """Row b of a masked batch is torch.nn.GRU on the valid steps of that row alone (in processing order); the output
  at a masked step repeats the one before (the initial state before the first valid step)."""
  d = G.make_inputs(case)
  ref = G.restate(case, d)
  B, T, E, U = case.B, case.T, case.E, case.U
  backwards = case.opts[2]
  net = _torch_gru(d, U, E)
  x = torch.tensor(d["x"].astype(np.float64), requires_grad=True)
  h0 = None if d["h0"] is None else torch.tensor(d["h0"].astype(np.float64), requires_grad=True)
  order = list(range(T - 1, -1, -1)) if backwards else list(range(T))
  rows_seq, rows_last = [], []
  for b in range(B):
    valid = [tt for tt in order if d["mask"][b, tt]]
    start = h0[b] if h0 is not None else torch.zeros(U, dtype=torch.float64)
    ys = None
    if valid:
      ys, _ = net(x[b, valid][None], start[None, None])
      ys = ys[0]
    cur, k, outs = start, 0, []
    for tt in order:
      if d["mask"][b, tt]:
        cur = ys[k]
        k += 1
      outs.append(cur)
    rows_seq.append(torch.stack(outs))
    rows_last.append(cur)
  seq, last = torch.stack(rows_seq), torch.stack(rows_last)
  _close(seq.detach().numpy(), ref["seq"].value, "seq")
  _close(last.detach().numpy(), ref["last"].value, "last")
  # a row masked everywhere returns its initial state
  dead = ~d["mask"].any(axis=1)
  assert dead.any() or case.mask not in ("row_all_false", "right", "left")
  want = d["h0"][dead] if d["h0"] is not None else np.zeros((int(dead.sum()), U))
  assert np.array_equal(ref["last"].value[dead], want)
  loss = torch.zeros((), dtype=torch.float64)
  if d["wseq"] is not None:
    loss = loss + (seq * torch.tensor(d["wseq"].astype(np.float64))).sum()
  if d["wlast"] is not None:
    loss = loss + (last * torch.tensor(d["wlast"].astype(np.float64))).sum()
  assert not np.any(ref["dx"].value[~d["mask"]]), "a masked step has a zero input gradient"
  if not loss.requires_grad:      # every row masked everywhere and no initial state: the loss depends on nothing
    assert not any(ref[k].value.any() for k in ("dx", "dkernel", "drecurrent"))
    return
  loss.backward()
  _close(_grad(x), ref["dx"].value, "dx")
  if h0 is not None:
    _close(_grad(h0), ref["dh0"].value, "dh0")
  for k, v in _torch_grads(net, U, d["bias"] is not None).items():
    _close(v, ref[k].value, k)


def test_the_float32_recurrence_of_the_allowance_is_the_restated_one():
  """torch_recurrence is what measures the allowance: in float64 it must be the restatement itself."""
  for case in (G.CASES[1], G.CASES[10], G.CASES[-2]):
    d = G.make_inputs(case)
    ref = G.restate(case, d)
    got = G.torch_recurrence(d, case.opts[2], torch.float64)
    for k in got:
      _close(got[k], ref[k].value, k)


def test_case_list_covers_what_the_issue_lists():
  assert {c.B for c in G.CASES} == set(G.BATCHES)
  assert {c.U for c in G.CASES} == set(G.UNITS)
  assert {c.U for c in G.CASES if c.B == 33} == set(G.UNITS)
  for U in (9, 33, 64):
    assert {c.B for c in G.CASES if c.U == U} >= set(G.BATCHES)
  assert {c.E for c in G.CASES} == {1, 33} and {c.T for c in G.CASES} == {1, 2, 9}
  assert {c.mask for c in G.CASES} == set(G.MASKS)
  assert all(c.T == 9 for c in G.CASES if c.mask != "none")
  assert {c.opts for c in G.CASES} == set(G.OPTIONS)
  for i in range(5):                      # every option on and off
    assert {o[i] for o in G.OPTIONS} == {True, False}
  rng = np.random.default_rng(0)
  right = G.make_mask("right", 33, 9, rng).sum(axis=1)
  assert 0 in right and 9 in right


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: f"B{c.B}-T{c.T}-E{c.E}-U{c.U}-{c.mask}")
def test_the_limits_have_teeth_in_every_case(case):
  """The limit of every gate of every case (4 x the float32 CPU ratio on the case's own inputs, floored) refuses a
  zeroed result and one that is 1 % off, and accepts the float32 CPU recurrence it was measured on; and no yard is
  far from its entry: the largest |value| / yard of a tensor is above 1e-2."""
  ref, lim = G.restate(case), G.limits(case)
  measured = G.float32_errors(case)
  for key, entry in ref.items():
    name = G.GATES[key]
    assert lim[name] >= 4.0 * G.ALLOWANCE_FLOOR
    if key in measured:
      assert measured[key] <= lim[name] / 4.0
    if not np.any(entry.value):
      continue                    # (a batch masked everywhere without initial state: exact zeros, yard 0)
    assert G.ratio(np.zeros_like(entry.value), entry) > 1e-2, key
    assert G.ratio(np.zeros_like(entry.value), entry) > 100.0 * lim[name], key
    assert G.ratio(entry.value * 1.01, entry) > lim[name], key
    assert G.ratio(entry.value * 0.99, entry) > lim[name], key
    assert np.all(entry.yard >= np.abs(entry.value) * (1.0 - 1e-12)), key      # a sum of |terms| is at least the entry


def test_constructor_validation():
  from recommenders_amd.layers import GRU
  for kwargs, word in (({"dropout": 0.1}, "dropout"), ({"recurrent_dropout": 0.1}, "recurrent_dropout"),
                       ({"stateful": True}, "stateful"), ({"unroll": True}, "unroll"),
                       ({"reset_after": False}, "reset_after"), ({"activation": "relu"}, "activation"),
                       ({"recurrent_activation": "hard_sigmoid"}, "recurrent_activation"),
                       ({"time_major": True}, "time_major")):
    with pytest.raises(NotImplementedError, match=word):
      GRU(8, **kwargs)
  for units in (65, 129):
    with pytest.raises(NotImplementedError, match="units"):
      GRU(units)
  with pytest.raises(ValueError):
    GRU(0)
  layer = GRU(64, return_sequences=True, return_state=True, go_backwards=True, use_bias=False)
  assert (layer.units, layer.return_sequences, layer.return_state, layer.go_backwards, layer.use_bias) == (
      64, True, True, True, False)
  assert not layer.built and layer.get_weights() == []
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    GRU(4)(torch.zeros(2, 3, 5))
  with pytest.raises(ValueError):
    GRU(4)(torch.zeros(2, 3))


def test_initialisers():
  from recommenders_amd.layers import GRU
  torch.manual_seed(7)
  U, E = 24, 40
  layer = GRU(U, device="cpu")
  layer.build(E)
  assert tuple(layer.kernel.shape) == (E, 3 * U) and tuple(layer.recurrent_kernel.shape) == (U, 3 * U)
  assert tuple(layer.bias.shape) == (2, 3 * U) and not layer.bias.detach().any()
  lim = np.sqrt(6.0 / (E + 3 * U))
  k = layer.kernel.detach().numpy()
  assert np.abs(k).max() <= lim and np.abs(k).max() > 0.98 * lim
  assert abs(k.var() - lim * lim / 3.0) < 0.1 * lim * lim / 3.0          # uniform(-lim, lim)
  r = layer.recurrent_kernel.detach().numpy().astype(np.float64)
  for g in range(3):
    blk = r[:, g * U:(g + 1) * U]
    assert np.abs(blk @ blk.T - np.eye(U)).max() < 1e-5 and np.abs(blk.T @ blk - np.eye(U)).max() < 1e-5
  assert np.abs(r[:, :U] - r[:, U:2 * U]).max() > 0.1                    # three draws, not one
  nb = GRU(U, use_bias=False, device="cpu")
  nb.build(E)
  assert nb.bias is None and len(list(nb.parameters())) == 2


def test_weights_round_trip():
  from recommenders_amd.layers import GRU
  d = G.make_inputs(G.Case(2, 2, 5, 7, "none", G.OPTIONS[0], 5))
  layer = GRU(7, device="cpu")
  layer.set_weights([d["kernel"], d["recurrent_kernel"], d["bias"]])
  got = layer.get_weights()
  assert [g.shape for g in got] == [(5, 21), (7, 21), (2, 21)]
  for g, w in zip(got, (d["kernel"], d["recurrent_kernel"], d["bias"])):
    assert g.dtype == np.float32 and np.array_equal(g, w)
  other = GRU(7, device="cpu")                       # not built: takes its input width from the state
  other.load_state_dict(layer.state_dict())
  assert sorted(layer.state_dict()) == ["bias", "kernel", "recurrent_kernel"]
  for g, w in zip(other.get_weights(), got):
    assert np.array_equal(g, w)
  with pytest.raises(ValueError):
    layer.set_weights([d["kernel"], d["recurrent_kernel"]])
  with pytest.raises(ValueError):
    layer.set_weights([d["kernel"][:, :-1], d["recurrent_kernel"], d["bias"]])
  with pytest.raises(ValueError):
    layer.set_weights([d["kernel"], d["recurrent_kernel"].T, d["bias"]])
  nb = GRU(7, use_bias=False, device="cpu")
  nb.set_weights([d["kernel"], d["recurrent_kernel"]])
  assert len(nb.get_weights()) == 2


def test_embedding_compute_mask():
  from recommenders_amd.layers import Embedding
  ids = torch.tensor([[3, 0, 5], [0, 0, 1]])
  on = Embedding(8, 4, mask_zero=True, device="cpu")
  assert on.compute_mask(ids).tolist() == [[True, False, True], [False, False, True]]
  assert on.compute_mask(ids).dtype == torch.bool
  off = Embedding(8, 4, device="cpu")
  assert off.mask_zero is False and off.compute_mask(ids) is None


def test_entry_points_are_declared_bound_and_built():
  from recommenders_amd import _lib
  from recommenders_amd.csrc import build
  with open(os.path.join(ROOT, "include", "tfrs_hip.h")) as f:
    header = f.read()
  for name in ("tfrs_gru_fwd", "tfrs_gru_bwd"):
    assert f"int {name}(" in header
    assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_int
    assert _lib.SIGNATURES[name][1][-1] is _lib.P                    # the stream comes last
  assert len(_lib.SIGNATURES["tfrs_gru_fwd"][1]) == 17 and len(_lib.SIGNATURES["tfrs_gru_bwd"][1]) == 17
  assert "gru.hip" in build.SOURCES
  assert os.path.exists(os.path.join(ROOT, "recommenders_amd", "csrc", "gru.hip"))


@pytest.mark.parametrize("B,U", [(1, 1), (33, 9), (65, 64)])
@pytest.mark.parametrize("mask", G.MASKS)
def test_halving_is_exact_in_float32(B, U, mask):
  """The exactness argument of the GPU halving test, step by step in float32 numpy: with all-zero weights
  a = x 0 + 0 = 0 and q = h 0 + 0 = 0 (sums of zeros), z = r = sigma(0) = 1 / (1 + 1) = 1/2, hh = tanh(0 + 1/2 * 0) = 0,
  and h_t = 1/2 h + 1/2 * 0 is a halving of an integer below 2^11 scaled by at most 2^-T: every intermediate is a
  float32 number, so float32 and float64 agree under == at every step and with `halving_expected`."""
  T, E = 9, 3
  f32 = np.float32
  rng = np.random.default_rng(1)
  x = rng.normal(size=(B, T, E)).astype(f32)
  h0 = G.halving_state(B, U)
  assert h0.max() < 2 ** 11 and h0.min() >= 1 and np.array_equal(h0, np.round(h0))
  assert all(len(set(row)) == len(row) for row in h0)
  m = G.make_mask(mask, B, T, rng)
  live = np.ones((B, T), dtype=bool) if m is None else m
  K, R, b = np.zeros((E, 3 * U), f32), np.zeros((U, 3 * U), f32), np.zeros((2, 3 * U), f32)
  for backwards in (False, True):
    want_seq, want_last = G.halving_expected(h0, m, T, backwards)
    h = h0.copy()
    for t in range(T):
      tt = T - 1 - t if backwards else t
      a = (x[:, tt] @ K + b[0]).astype(f32)
      q = (h @ R + b[1]).astype(f32)
      assert not a.any() and not q.any()
      z = f32(1.0) / (f32(1.0) + np.exp(-(a[:, :U] + q[:, :U]), dtype=f32))
      r = f32(1.0) / (f32(1.0) + np.exp(-(a[:, U:2 * U] + q[:, U:2 * U]), dtype=f32))
      hh = np.tanh(a[:, 2 * U:] + r * q[:, 2 * U:], dtype=f32)
      assert np.all(z == f32(0.5)) and np.all(r == f32(0.5)) and not hh.any()
      hn = (z * h + (f32(1.0) - z) * hh).astype(f32)
      assert hn.dtype == f32 and np.array_equal(hn.astype(np.float64), h.astype(np.float64) / 2.0)
      h = np.where(live[:, tt][:, None], hn, h)
      assert np.array_equal(h, want_seq[:, t])
    assert np.array_equal(h, want_last)
    ref = G.gru(x, K, R, b, m, h0, backwards)
    assert np.array_equal(ref["seq"].value, want_seq.astype(np.float64))
    assert np.array_equal(ref["last"].value, want_last.astype(np.float64))
