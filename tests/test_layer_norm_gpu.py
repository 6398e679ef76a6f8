"""GPU tests of layers.LayerNormalization (csrc/layer_norm.hip) against the plain composition in float64
on the CPU (mean, mean of squared deviations, division by sqrt(var + eps), gamma, beta); a tensor's limit is
max(4 e32, 64 eps) max|ref64|, e32 from the same composition in float32."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# every edge of the dispatch table: D with D % 4 != 0 takes the dword route
DIMS = (1, 3, 4, 32, 33, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096, 4100, 8192)
ROWS_PER_GROUP = {4: 32, 132: 16, 1028: 1, 8192: 1}         # D -> rows of a workgroup; x 1024 + 1: one grid pass and a row
# (center, scale, residual, return_sum), dealt to the cases in turn
VARIANTS = ((True, True, False, False), (True, True, True, True), (False, True, True, False), (True, False, False, False),
            (True, True, True, False), (False, False, True, True))
CASES = [(n, d) for d in DIMS for n in (1, 13)] + [(rows * 1024 + 1, d) for d, rows in ROWS_PER_GROUP.items()]
CASES = [(n, d) + VARIANTS[i % len(VARIANTS)] for i, (n, d) in enumerate(CASES)]


@functools.lru_cache(maxsize=4)
def _inputs(n, d, center=True, scale=True, residual=True, return_sum=True):
  rng = np.random.default_rng(1000 * d + n)
  f = lambda *shape, s=1.0, m=0.0: (rng.normal(size=shape) * s + m).astype(np.float32)
  return {"x": f(n, d, s=2.0, m=0.5), "residual": f(n, d) if residual else None,
          "gamma": f(d, s=0.5, m=1.0) if scale else None, "beta": f(d, s=0.25) if center else None,
          "w": f(n, d), "w2": f(n, d) if return_sum else None}


def _reference(d, eps, dtype):
  """The composition on the CPU in `dtype`: the outputs and every gradient of sum(out w) + sum(sum_out w2), as float64
  arrays."""
  leaf = {k: torch.tensor(d[k], dtype=dtype, requires_grad=True) for k in ("x", "residual", "gamma", "beta")
          if d[k] is not None}
  s = leaf["x"] + leaf["residual"] if "residual" in leaf else leaf["x"]
  dev = s - s.mean(-1, keepdim=True)
  out = dev / torch.sqrt((dev * dev).mean(-1, keepdim=True) + eps) * leaf.get("gamma", 1.0) + leaf.get("beta", 0.0)
  loss = (out * torch.tensor(d["w"], dtype=dtype)).sum()
  got = {"out": out.detach()}
  if d["w2"] is not None:
    loss, got["sum"] = loss + (s * torch.tensor(d["w2"], dtype=dtype)).sum(), s.detach()
  loss.backward()
  got.update({"d" + k: t.grad for k, t in leaf.items()})
  return {k: np.asarray(t.numpy(), dtype=np.float64) for k, t in got.items()}


def _run(d, fused=True):
  """The layer on `d` with the loss of `_reference`; fused=False adds the residual with torch first."""
  from recommenders_amd.layers import LayerNormalization
  layer = LayerNormalization(center=d["beta"] is not None, scale=d["gamma"] is not None)
  layer.set_weights([d[k] for k in ("gamma", "beta") if d[k] is not None])
  t = {k: torch.as_tensor(d[k]).cuda().requires_grad_(k in ("x", "residual")) for k in d if d[k] is not None}
  if fused:
    out = layer(t["x"], residual=t.get("residual"), return_sum="w2" in t)
    got = dict(zip(("out", "sum"), out)) if "w2" in t else {"out": out}
  else:
    got = {"sum": t["x"] + t["residual"]}
    got["out"] = layer(got["sum"])
  loss = (got["out"] * t["w"]).sum() + ((got["sum"] * t["w2"]).sum() if "w2" in t else 0.0)
  loss.backward()
  got.update({"d" + k: t[k].grad for k in ("x", "residual") if k in t})
  got.update({"d" + k: p.grad for k, p in layer.named_parameters()})
  return {k: v.detach() for k, v in got.items()}


def _bits(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_values_and_gradients_against_the_float64_composition(case):
  d = _inputs(*case)
  ref64, ref32 = (_reference(d, 1e-3, dt) for dt in (torch.float64, torch.float32))
  got = _run(d)
  assert set(got) == set(ref64)
  if d["residual"] is not None:          # the fused add against torch's add in front of the layer: bit for bit
    plain = _run(d, fused=False)
    assert all(_bits(got[k], plain[k]) for k in got), [k for k in got if not _bits(got[k], plain[k])]
  for k, want in ref64.items():
    value, top = got[k].cpu().numpy(), np.abs(want).max()
    assert value.shape == want.shape, k
    if top == 0.0:
      assert not value.any(), k
      continue
    limit = max(4.0 * np.abs(ref32[k] - want).max() / top, 64.0 * EPS) * top
    err = np.abs(value - want).max()
    print(f"{k}: observed / limit = {err / limit:.3f}")
    assert err <= limit, (k, err, limit)


@pytest.mark.parametrize("D", [33, 132, 1028, 1030])          # sub-wave and workgroup routes, dword and 16-byte
def test_bitwise_invariants_of_both_entry_points(D):
  from recommenders_amd import _lib
  lib, S, P = _lib.load(), _lib.current_stream(), _lib.ptr
  N, four = 70, 3
  g = torch.Generator(device="cuda").manual_seed(D)
  rand = lambda *shape: torch.randn(shape, generator=g, device="cuda")
  x, r, dy, beta = rand(N, D), rand(N, D), rand(N, D), rand(D)
  x[four], r[four], dy[four] = 1.0, 3.0, 1.0          # x + r is 4.0 throughout: its sums are exact integers

  def guarded(*shape):          # the entry points' outputs get NaN sentinels on either side
    buf = torch.full((int(np.prod(shape)) + 128,), float("nan"), device="cuda")
    return buf[64:-64].view(*shape), buf

  def run(rows):
    n, (x_, r_, dy_) = rows.stop - rows.start, (t[rows].contiguous() for t in (x, r, dy))
    words = lib.tfrs_layer_norm_workspace_bytes(n, D) // 4
    assert words == 2 * D * -(-n // {33: 32, 132: 16}.get(D, 1))          # one slab per workgroup, 256 / G rows each
    outs = [guarded(n, D), guarded(n, D), guarded(n), guarded(n), guarded(n, D), guarded(D), guarded(D)]
    ws = guarded(words)
    (y, s, mean, rstd, dx, dgamma, dbeta) = (o[0] for o in outs)
    _lib.check(lib.tfrs_layer_norm_fwd(P(x_), P(r_), None, P(beta), n, D, 1e-3, P(y), P(s), P(mean), P(rstd), S))
    _lib.check(lib.tfrs_layer_norm_bwd(P(s), P(mean), P(rstd), None, P(dy_), None, n, D, P(dx), P(dgamma), P(dbeta),
                                       P(ws[0]), 4 * words, S))
    for view, buf in outs + [ws]:
      assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
    assert not any(bool(torch.isnan(o[0]).any()) for o in outs)
    return [o[0] for o in outs]

  full = run(slice(0, N))
  assert all(_bits(a, b) for a, b in zip(full, run(slice(0, N))))                    # (c) two runs, dgamma and dbeta too
  for i in (0, four, 37, N - 1):                                                     # (a) a row of the batch, alone
    assert all(_bits(a[i:i + 1], o) for a, o in zip(full[:5], run(slice(i, i + 1)))), i
  y, s, mean, rstd, dx = full[:5]                                                    # (d) the row of fours
  assert _bits(y[four], beta) and not bool(dx[four].any()) and float(mean[four]) == 4.0 and _bits(s, x + r)
  assert float(rstd[four]) == float(1.0 / torch.sqrt(torch.tensor(1e-3, dtype=torch.float32)))


@pytest.mark.parametrize("center,scale", [(True, True), (False, True), (True, False), (False, False)])
def test_surface_weights_config_envelope_and_empty_input(center, scale):
  from recommenders_amd import _lib
  from recommenders_amd.layers import LayerNormalization
  lib, S = _lib.load(), _lib.current_stream()
  for call in (lambda: lib.tfrs_layer_norm_fwd(*[None] * 4, 4, 8193, 1e-3, *[None] * 4, S),       # nothing launched
               lambda: lib.tfrs_layer_norm_bwd(*[None] * 6, 4, 8193, *[None] * 4, 0, S)):
    with pytest.raises(NotImplementedError, match="D = 8193"):
      _lib.check(call())
  with pytest.raises(NotImplementedError, match="8193"):
    LayerNormalization()(torch.zeros((2, 8193), device="cuda"))
  for axis in (0, 1, -2, [1, 2]):
    with pytest.raises(NotImplementedError, match="axis"):
      LayerNormalization(axis=axis)(torch.zeros((2, 3, 4), device="cuda"))
  layer = LayerNormalization(axis=[2], epsilon=1e-5, center=center, scale=scale, name="ln")
  assert layer.get_weights() == [] and layer.state_dict() == {}
  x = torch.randn((2, 3, 6), device="cuda")
  assert tuple(layer(x).shape) == (2, 3, 6) and len(layer.get_weights()) == int(center) + int(scale)
  weights = [np.arange(6, dtype=np.float32) + i for i in range(int(center) + int(scale))]
  layer.set_weights(weights)
  assert all(np.array_equal(a, b) for a, b in zip(layer.get_weights(), weights))
  assert list(layer.state_dict()) == [n for n, on in (("gamma", scale), ("beta", center)) if on]
  clone = LayerNormalization.from_config(layer.get_config())
  clone.load_state_dict(layer.state_dict())                   # rebuilds the lazily built clone
  assert clone.get_config() == layer.get_config() and _bits(clone(x.double()), layer(x))
  empty = torch.zeros((2, 0, 6), device="cuda", requires_grad=True)       # N == 0: no launch, zero parameter gradients
  out = layer(empty, residual=empty)
  out.sum().backward()
  assert tuple(out.shape) == (2, 0, 6) and tuple(empty.grad.shape) == (2, 0, 6)
  assert all(tuple(p.grad.shape) == (6,) and not bool(p.grad.any()) for p in layer.parameters())


@pytest.mark.parametrize("dim", [16])
def test_pre_norm_block_trains_and_the_captured_step_matches_the_eager_one(dim):
  import recommenders_amd as tfrs

  class Block(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.embedding = tfrs.layers.Embedding(50, dim, mask_zero=True)
      self.attention = tfrs.layers.MultiHeadAttention(2, 8)
      self.attention.build(dim, device="cuda")
      self.norm = tfrs.layers.LayerNormalization()
      self.norm.build(dim, device="cuda")
      self.dense = tfrs.layers.blocks.Dense(dim, activation="relu")
      self.dense.build(dim, torch.device("cuda"))
      self.candidates = tfrs.layers.Embedding(40, dim)
      self.task = tfrs.tasks.Retrieval()

    def compute_loss(self, features, training=False):
      ids = features["history"]
      x, m = self.embedding(ids), self.embedding.compute_mask(ids)
      a = self.attention(x, x, query_mask=m, value_mask=m, use_causal_mask=True)
      y, s = self.norm(a, residual=x, return_sum=True)
      out = s + self.dense(y)
      last = m & ~torch.cat([m[:, 1:], torch.zeros_like(m[:, :1])], dim=1)      # a right-padded row's last live step
      return self.task((out * last[:, :, None]).sum(dim=1), self.candidates(features["movie_id"]),
                       compute_metrics=False)

  def tower():
    torch.manual_seed(3)
    m = Block()
    m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.1))
    return m

  rng = np.random.default_rng(11)
  hist = rng.integers(1, 50, size=(64, 9))
  hist[np.arange(9)[None, :] >= rng.integers(1, 10, size=64)[:, None]] = 0      # right-padded with the mask id
  batch = {"history": torch.as_tensor(hist).cuda(), "movie_id": torch.as_tensor(rng.integers(0, 40, size=64)).cuda()}
  eager, graphed = tower(), tower()
  step = graphed.make_graphed_train_step(batch)
  before, losses = [p.detach().clone() for p in eager.parameters()], []
  for _ in range(3):                                  # three eager steps against three replays, bit for bit
    losses.append(float(eager.train_step(batch)["loss"]))
    assert float(step(batch)["loss"]) == losses[-1]
  assert losses[2] < losses[0], losses
  params = list(zip(before, eager.parameters(), graphed.parameters()))
  assert len(params) == 14 and all(_bits(e, g) and not _bits(b, e) for b, e, g in params)
