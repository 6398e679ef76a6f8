"""GPU tests of layers.MultiHeadAttention (csrc/attention.hip) against the plain composition in float64 on
the CPU (projections, masked_fill(-inf), softmax, zero rows where no key is allowed); a tensor's limit is
max(4 e32, 64 eps) max|ref64|, e32 from the same composition in float32."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, EPS = 5, 2.0 ** -24
NAMES = ("query_kernel", "query_bias", "key_kernel", "key_bias", "value_kernel", "value_bias", "output_kernel",
         "output_bias")
# (B, Tq, Tk, key_dim, value_dim, H, mask, causal, inputs, use_bias); inputs: "self" = layer(x, x), "kv" = layer(q, v),
# "cross" = layer(q, v, key=k)
CASES = [
    (1, 1, 1, 1, 1, 1, "none", False, "self", True),
    (5, 10, 10, 32, 32, 1, "right", True, "self", True),
    (5, 31, 31, 9, 32, 3, "right", True, "self", True),
    (5, 32, 33, 32, 9, 1, "left", False, "cross", False),
    (1, 33, 32, 33, 64, 3, "holes", False, "cross", True),
    (5, 64, 65, 64, 33, 1, "full", False, "kv", True),
    (5, 65, 64, 1, 9, 3, "dead_batch_row", False, "cross", False),
    (1, 128, 128, 64, 64, 1, "none", True, "self", True),
    (5, 128, 31, 33, 32, 3, "right", False, "cross", True),
    (5, 1, 128, 32, 33, 1, "holes", False, "kv", False),
    (5, 31, 1, 9, 9, 3, "none", False, "cross", True),
    (1, 64, 64, 32, 32, 3, "full", True, "self", False),
]


def _masks(kind, B, Tq, Tk, rng, self_attention=False):
  """The layer's mask arguments.  right / left: padded keys (and queries, in self-attention), every length >= 1;
  holes: key_mask AND value_mask with holes, as int32; full: a [B, Tq, Tk] mask with one query row of nothing;
  dead_batch_row: right-padded with one batch row of length 0."""
  m = {"attention_mask": None, "query_mask": None, "value_mask": None, "key_mask": None}
  lengths = np.array([1 + (3 * b) % Tk for b in range(B)])[:, None]
  pos = np.arange(Tk)[None, :]
  if kind in ("right", "left", "dead_batch_row"):
    lengths[B // 2] = 0 if kind == "dead_batch_row" else lengths[B // 2]
    m["value_mask"] = pos < lengths if kind != "left" else pos >= Tk - lengths
    m["query_mask"] = m["value_mask"] if self_attention else None
  elif kind == "holes":
    m["key_mask"], m["value_mask"] = ((rng.random((B, Tk)) < 0.8).astype(np.int32) for _ in range(2))
    m["key_mask"][:, 0] = m["value_mask"][:, 0] = 1
  elif kind == "full":
    m["attention_mask"] = rng.random((B, Tq, Tk)) < 0.6
    m["attention_mask"][:, :, 0], m["attention_mask"][0, Tq // 2] = True, False
  return m


@functools.lru_cache(maxsize=None)
def _inputs(B, Tq, Tk, dk, dv, H, mask, inputs="cross", use_bias=True):
  rng = np.random.default_rng(1000 * Tq + 10 * Tk + dk)
  f = lambda *shape, s=1.0: (rng.normal(size=shape) * s).astype(np.float32)
  d = {"query": f(B, Tq, D), "value": None if inputs == "self" else f(B, Tk, D),
       "key": f(B, Tk, D) if inputs == "cross" else None, "w": f(B, Tq, D),
       "query_kernel": f(D, H, dk), "key_kernel": f(D, H, dk, s=dk ** -0.5), "value_kernel": f(D, H, dv),
       "output_kernel": f(H, dv, D, s=(H * dv) ** -0.5)}
  if use_bias:
    d.update(query_bias=f(H, dk, s=0.25), key_bias=f(H, dk, s=0.25), value_bias=f(H, dv, s=0.25),
             output_bias=f(D, s=0.25))
  d.update(_masks(mask, B, Tq, Tk, rng, inputs == "self"))
  return d


def _reference(d, causal, dtype):
  """The composition on the CPU in `dtype`: the output and every gradient of sum(output * w), as float64 arrays."""
  leaf = {n: torch.tensor(d[n], dtype=dtype, requires_grad=True)
          for n in ("query", "value", "key") + NAMES if d.get(n) is not None}
  query = leaf["query"]
  value = leaf.get("value", query)
  key = leaf.get("key", value)
  proj = lambda x, n: torch.einsum("btd,dhe->bhte", x, leaf[n + "_kernel"]) + (
      leaf[n + "_bias"][None, :, None, :] if n + "_bias" in leaf else 0.0)
  q, k, v = proj(query, "query"), proj(key, "key"), proj(value, "value")
  (B, Tq, _), Tk = query.shape, value.shape[1]
  allow = np.ones((B, Tq, Tk), dtype=bool)
  for n, axes in (("attention_mask", np.s_[:, :, :]), ("query_mask", np.s_[:, :, None]),
                  ("value_mask", np.s_[:, None, :]), ("key_mask", np.s_[:, None, :])):
    allow &= True if d[n] is None else (d[n] != 0)[axes]
  allow &= np.tri(Tq, Tk, dtype=bool)[None] if causal else True
  allow = torch.tensor(allow)[:, None]
  live = allow.any(-1, keepdim=True)
  s = (q @ k.transpose(-1, -2) / q.shape[-1] ** 0.5).masked_fill(~allow & live, float("-inf"))
  p = torch.where(live, torch.softmax(s, dim=-1), torch.zeros((), dtype=dtype))
  out = torch.einsum("bhte,hed->btd", p @ v, leaf["output_kernel"]) + leaf.get("output_bias", 0.0)
  (out * torch.tensor(d["w"], dtype=dtype)).sum().backward()
  got = {"out": out.detach(), **{"d" + n: t.grad for n, t in leaf.items()}}
  return {n: np.asarray(t.numpy(), dtype=np.float64) for n, t in got.items()}


def _cuda(a, grad=False):
  return None if a is None else torch.as_tensor(a).cuda().requires_grad_(grad)


def _run(d, causal=False):
  """The layer on `d` with the loss of `_reference`: {name: tensor} of the output and every gradient."""
  from recommenders_amd.layers import MultiHeadAttention
  H, dk = d["query_kernel"].shape[1:]
  layer = MultiHeadAttention(H, dk, value_dim=d["value_kernel"].shape[2], use_bias="query_bias" in d)
  layer.set_weights([d[n] for n in NAMES if n in d])
  x = {n: _cuda(d[n], True) for n in ("query", "value", "key") if d[n] is not None}
  masks = {n: _cuda(d[n]) for n in ("attention_mask", "query_mask", "value_mask", "key_mask")}
  out = layer(x["query"], x.get("value", x["query"]), key=x.get("key"), use_causal_mask=causal, **masks)
  (out * _cuda(d["w"])).sum().backward()
  got = {"out": out, **{"d" + n: t.grad for n, t in x.items()},
         **{"d" + n: p.grad for n, p in layer.named_parameters()}}
  return {n: t.detach() for n, t in got.items()}


def _bits(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v) if isinstance(v, bool) else v) for v in c))
def test_values_and_gradients_against_the_float64_composition(case):
  *shape, causal, inputs, use_bias = case
  d = _inputs(*shape, inputs, use_bias)
  ref64, ref32 = (_reference(d, causal, dt) for dt in (torch.float64, torch.float32))
  got = _run(d, causal)
  assert set(got) == set(ref64)
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


@pytest.mark.parametrize("Tq,Tk,d", [(33, 65, 9), (128, 128, 64), (10, 10, 32)])
def test_bitwise_invariants_of_both_entry_points(Tq, Tk, d):
  from recommenders_amd import _lib
  lib, S, P = _lib.load(), _lib.current_stream(), _lib.ptr
  B, H, dead_q, dead_k = 5, 3, (0, Tq // 2), Tk - 2
  g = torch.Generator(device="cuda").manual_seed(Tq)
  rand = lambda *shape: torch.randn(shape, generator=g, device="cuda")
  q, k, v, dout = rand(B, Tq, H, d), rand(B, Tk, H, d), rand(B, Tk, H, d), rand(B, Tq, H, d)
  km = (torch.rand((B, Tk), generator=g, device="cuda") < 0.8).to(torch.uint8)
  km[:, 0], km[:, dead_k] = 1, 0                    # no query of any row may see key dead_k
  qm = torch.ones((B, Tq), dtype=torch.uint8, device="cuda")
  qm[dead_q] = 0                                    # one query with nothing allowed

  def guarded(*shape):          # the entry points' outputs get NaN sentinels on either side
    buf = torch.full((int(np.prod(shape)) + 128,), float("nan"), device="cuda")
    return buf[64:-64].view(*shape), buf

  def run(rows):
    n, (q_, k_, v_, g_, km_, qm_) = rows.stop - rows.start, (t[rows].contiguous() for t in (q, k, v, dout, km, qm))
    outs = [guarded(n, Tq, H, d), guarded(n, H, Tq), guarded(n, Tq, H, d), guarded(n, Tk, H, d), guarded(n, Tk, H, d)]
    (out, lse, dq, dk, dv) = (o[0] for o in outs)
    _lib.check(lib.tfrs_attention_fwd(P(q_), P(k_), P(v_), None, P(qm_), P(km_), n, Tq, Tk, H, d, d, d ** -0.5, 1,
                                      P(out), P(lse), S))
    _lib.check(lib.tfrs_attention_bwd(P(q_), P(k_), P(v_), None, P(qm_), P(km_), P(out), P(lse), P(g_), n, Tq, Tk, H,
                                      d, d, d ** -0.5, 1, P(dq), P(dk), P(dv), S))
    for view, buf in outs:
      assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all())
      assert not bool(torch.isnan(view).any())
    return [o[0] for o in outs]

  full = run(slice(0, B))
  assert all(_bits(a, b) for a, b in zip(full, run(slice(0, B))))                      # two runs
  for b in (0, 2, 4):                                                                # a row of the batch, alone
    assert all(_bits(a[b:b + 1], o) for a, o in zip(full, run(slice(b, b + 1)))), b
  out, lse, dq, dk, dv = full
  zero = lambda t: bool((t.contiguous().view(torch.int32) == 0).all())
  assert zero(out[dead_q]) and zero(dq[dead_q]) and bool((lse[dead_q[0], :, dead_q[1]] == float("inf")).all())
  assert zero(dk[:, dead_k]) and zero(dv[:, dead_k]) and bool(dq[0, Tq - 1].any()) and bool(dv[:, 0].any())
  assert bool(torch.isfinite(lse).sum() == lse.numel() - H)


def test_shapes_outside_the_envelope_and_unbuilt_options_are_refused():
  from recommenders_amd import _lib
  from recommenders_amd.layers import MultiHeadAttention
  lib, S = _lib.load(), _lib.current_stream()
  for name, (tq, tk, dk, dv) in {"Tq": (129, 8, 8, 8), "Tk": (8, 129, 8, 8), "dk": (8, 8, 65, 8),
                                 "dv": (8, 8, 8, 65)}.items():
    for call in (lambda: lib.tfrs_attention_fwd(*[None] * 6, 4, tq, tk, 2, dk, dv, 1.0, 0, None, None, S),
                 lambda: lib.tfrs_attention_bwd(*[None] * 9, 4, tq, tk, 2, dk, dv, 1.0, 0, None, None, None, S)):
      with pytest.raises(NotImplementedError, match=f"{name} = "):
        _lib.check(call())
  with pytest.raises(NotImplementedError, match="dropout"):
    MultiHeadAttention(2, 8, dropout=0.1)
  x = torch.zeros((2, 3, D), device="cuda")
  with pytest.raises(NotImplementedError, match="return_attention_scores"):
    MultiHeadAttention(2, 8)(x, x, return_attention_scores=True)


@pytest.mark.parametrize("B,Tq", [(0, 9), (4, 0), (0, 0)])
def test_empty_batches_return_the_output_bias_and_zero_gradients(B, Tq):
  from recommenders_amd.layers import MultiHeadAttention
  layer = MultiHeadAttention(2, 8, output_shape=7, bias_initializer="ones")
  layer.build(D, device="cuda")
  query, value = (torch.zeros(s, device="cuda", requires_grad=True) for s in ((B, Tq, D), (B, 9, D)))
  out = layer(query, value)
  assert tuple(out.shape) == (B, Tq, 7) and bool((out == 1.0).all())
  out.sum().backward()
  assert tuple(query.grad.shape) == (B, Tq, D) and tuple(value.grad.shape) == (B, 9, D)
  assert len(list(layer.parameters())) == 8 and all(not bool(p.grad.any()) for p in layer.parameters())


def test_attention_tower_trains_and_the_captured_step_matches_the_eager_one():
  import recommenders_amd as tfrs

  class Sequential(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.embedding = tfrs.layers.Embedding(50, 16, mask_zero=True)
      self.attention = tfrs.layers.MultiHeadAttention(2, 8)
      self.attention.build(16, device="cuda")
      self.candidates = tfrs.layers.Embedding(40, 16)
      self.task = tfrs.tasks.Retrieval()

    def compute_loss(self, features, training=False):
      ids = features["history"]
      x, m = self.embedding(ids), self.embedding.compute_mask(ids)
      y = self.attention(x, x, query_mask=m, value_mask=m, use_causal_mask=True)
      last = m & ~torch.cat([m[:, 1:], torch.zeros_like(m[:, :1])], dim=1)      # a right-padded row's last live step
      return self.task((y * last[:, :, None]).sum(dim=1), self.candidates(features["movie_id"]),
                       compute_metrics=False)

  def tower():
    torch.manual_seed(3)
    m = Sequential()
    m.compile(optimizer=tfrs.optimizers.Adagrad(m.parameters(), learning_rate=0.5))
    return m

  rng = np.random.default_rng(11)
  hist = rng.integers(1, 50, size=(64, 9))
  hist[np.arange(9)[None, :] >= rng.integers(1, 10, size=64)[:, None]] = 0      # right-padded with the mask id
  batch = {"history": _cuda(hist), "movie_id": _cuda(rng.integers(0, 40, size=64))}
  eager, graphed = tower(), tower()
  step = graphed.make_graphed_train_step(batch)
  before, losses = [p.detach().clone() for p in eager.parameters()], []
  for _ in range(3):                                  # three eager steps against three replays, bit for bit
    losses.append(float(eager.train_step(batch)["loss"]))
    assert float(step(batch)["loss"]) == losses[-1]
  assert losses[2] < losses[1] < losses[0], losses
  params = list(zip(before, eager.parameters(), graphed.parameters()))
  assert len(params) == 10 and all(_bits(e, g) and not _bits(b, e) for b, e, g in params)
