"""GPU tests of layers.LSTM (csrc/lstm.hip) against torch.nn.LSTM in float64 on the CPU, run per row over
the row's unmasked steps; a tensor's limit is max(4 e32, 64 eps) max|ref64|, e32 from the same net in float32."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, EPS = 5, 2.0 ** -24
# (B, T, U, mask, return_sequences, return_state, go_backwards, initial_state, use_bias)
CASES = [
    (33, 9, 1, "right", True, True, False, True, True),
    (33, 9, 9, "holes", True, True, True, True, False),
    (33, 2, 32, "none", False, False, False, False, True),
    (33, 9, 33, "left", True, True, False, True, True),
    (33, 9, 64, "row_all_false", True, True, True, True, True),
    (1, 9, 9, "first_false", True, True, False, True, True),
    (32, 1, 9, "none", False, True, True, False, False),
    (65, 9, 9, "left", True, False, False, False, True),
    (1, 2, 64, "none", True, True, False, True, False),
    (32, 9, 64, "holes", False, True, False, True, True),
    (65, 9, 64, "right", True, True, True, True, True),
]


def _mask(kind, B, T, rng):
  if kind == "none":
    return None
  lengths = np.array([(3 * b) % (T + 1) for b in range(B)])[:, None]          # 0, 3, 6, 9, 2, ...: 0 and T included
  pos = np.arange(T)[None, :]
  if kind in ("right", "left"):
    return pos < lengths if kind == "right" else pos >= T - lengths
  m = rng.random((B, T)) < 0.6
  if kind == "holes":
    m[:, [0, -1]], m[:, T // 2] = True, False
  elif kind == "row_all_false":
    m[B // 2] = False
  else:
    m[:, 0] = False
  return m


@functools.lru_cache(maxsize=None)
def _inputs(B, T, U, mask, initial_state=True, use_bias=True):
  rng = np.random.default_rng(1000 * B + 10 * U + T)
  f = lambda *shape, s=1.0: (rng.normal(size=shape) * s).astype(np.float32)
  return {"x": f(B, T, E), "kernel": f(E, 4 * U, s=0.5), "recurrent_kernel": f(U, 4 * U, s=U ** -0.5),
          "bias": f(4 * U, s=0.25) if use_bias else None, "mask": _mask(mask, B, T, rng),
          "h0": f(B, U, s=0.5) if initial_state else None, "c0": f(B, U) if initial_state else None,
          "wseq": f(B, T, U), "wh": f(B, U), "wc": f(B, U)}


def _reference(d, seq, state, backwards, dtype):
  """torch.nn.LSTM on the CPU in `dtype`, row by row over the unmasked steps: values and gradients as float64 arrays."""
  t_ = lambda a, g=False: None if a is None else torch.tensor(a, dtype=dtype, requires_grad=g)
  (B, T, _), U = d["x"].shape, d["recurrent_kernel"].shape[0]
  net = torch.nn.LSTM(E, U, batch_first=True).to(dtype)
  with torch.no_grad():
    net.weight_ih_l0.copy_(t_(d["kernel"].T))
    net.weight_hh_l0.copy_(t_(d["recurrent_kernel"].T))
    net.bias_ih_l0.copy_(t_(d["bias"] if d["bias"] is not None else np.zeros(4 * U)))
    net.bias_hh_l0.zero_()
  x, h0, c0 = t_(d["x"], True), t_(d["h0"], True), t_(d["c0"], True)
  order = list(range(T))[::-1] if backwards else list(range(T))
  seqs, hs, cs = [], [], []
  for b in range(B):
    live = [tt for tt in order if d["mask"] is None or d["mask"][b, tt]]
    h = h0[b] if h0 is not None else torch.zeros(U, dtype=dtype)
    c = c0[b] if c0 is not None else torch.zeros(U, dtype=dtype)
    out = torch.zeros((T, U), dtype=dtype)            # zeros before the first live step
    if live:
      ys, (h, c) = net(x[b, live][None], (h[None, None], c[None, None]))
      h, c = h[0, 0], c[0, 0]
      steps = np.cumsum([tt in live for tt in order]) - 1           # index of the last live step so far
      out = torch.where(torch.tensor(steps >= 0)[:, None], ys[0][np.maximum(steps, 0)], out)
    seqs.append(out), hs.append(h), cs.append(c)
  got = {"seq": torch.stack(seqs), "h": torch.stack(hs), "c": torch.stack(cs)}
  got = {k: v for k, v in got.items() if (k == "seq" and seq) or (k != "seq" and state) or (k == "h" and not seq)}
  loss = sum((v * t_(d["w" + k])).sum() for k, v in got.items())
  if loss.requires_grad:
    loss.backward()
  g = lambda p: np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy()
  got = {k: v.detach().numpy() for k, v in got.items()}
  got.update(dx=g(x), dkernel=g(net.weight_ih_l0).T, drecurrent_kernel=g(net.weight_hh_l0).T)
  got.update({} if d["bias"] is None else {"dbias": g(net.bias_ih_l0)})
  got.update({} if h0 is None else {"dh0": g(h0), "dc0": g(c0)})
  return {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}


def _cuda(a, grad=False):
  return None if a is None else torch.as_tensor(a).cuda().requires_grad_(grad)


def _run(d, seq=True, state=True, backwards=False, grad=True):
  """The layer on `d` with the loss of `_reference`: {name: tensor} of what it returns and every gradient."""
  from recommenders_amd.layers import LSTM
  layer = LSTM(d["recurrent_kernel"].shape[0], return_sequences=seq, return_state=state, go_backwards=backwards,
               use_bias=d["bias"] is not None)
  layer.set_weights([w for w in (d["kernel"], d["recurrent_kernel"], d["bias"]) if w is not None])
  x, h0, c0 = _cuda(d["x"], grad), _cuda(d["h0"], grad), _cuda(d["c0"], grad)
  with torch.set_grad_enabled(grad):
    out = layer(x, mask=_cuda(d["mask"]), initial_state=None if h0 is None else [h0, c0])
  out = out if isinstance(out, tuple) else (out,)
  got = dict(zip(("seq", "h", "c") if seq else ("h", "h", "c"), out))
  if grad:
    sum((v * _cuda(d["w" + k])).sum() for k, v in got.items()).backward()
    got.update(dx=x.grad, dkernel=layer.kernel.grad, drecurrent_kernel=layer.recurrent_kernel.grad)
    got.update({} if layer.bias is None else {"dbias": layer.bias.grad})
    got.update({} if h0 is None else {"dh0": h0.grad, "dc0": c0.grad})
  return {k: v.detach() for k, v in got.items()}


def _bits(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_same = lambda a, b: set(a) == set(b) and all(_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(v) if isinstance(v, bool) else v) for v in c))
def test_values_and_gradients_against_torch_lstm_float64(case):
  B, T, U, mask, seq, state, backwards, initial_state, use_bias = case
  d = _inputs(B, T, U, mask, initial_state, use_bias)
  ref64, ref32 = (_reference(d, seq, state, backwards, dt) for dt in (torch.float64, torch.float32))
  got = _run(d, seq, state, backwards)
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


@pytest.mark.parametrize("U", (9, 64))
def test_bitwise_invariants(U):
  from recommenders_amd import _lib
  from recommenders_amd.layers.feature_interaction.dcn import dense
  B, T, d = 33, 9, _inputs(33, 9, U, "holes")
  a = _run(d)
  assert _same(a, _run(d))                                                  # two runs
  dx, dead = a["dx"].cpu().numpy(), ~d["mask"]
  assert np.all(dx[dead].view(np.uint32) == 0) and np.any(dx[d["mask"]])    # +0 at masked steps
  part = lambda src, rows, t=T: dict(src, **{k: src[k][rows, :t] if k in ("x", "mask") else src[k][rows]
                                             for k in ("x", "mask", "h0", "c0")})
  full = _run(d, grad=False)
  for b in (0, 31, 32):                                                     # a row of the batch against the row alone
    assert _same({k: v[b:b + 1] for k, v in full.items()}, _run(part(d, slice(b, b + 1)), grad=False)), b
  flipped = dict(d, x=d["x"][:, ::-1].copy(), mask=d["mask"][:, ::-1].copy())
  assert _same(_run(d, backwards=True, grad=False), _run(flipped, grad=False))
  r = _inputs(B, T, U, "right")
  last = _run(r, seq=False, grad=False)
  for b in (1, 3, 32):                                                      # lengths 3, 9, 6
    n = int(r["mask"][b].sum())
    one = _run(dict(part(r, slice(b, b + 1), n), mask=None), seq=False, grad=False)
    assert _same({k: v[b:b + 1] for k, v in last.items()}, one), (b, n)
  def guarded(*shape):          # the entry points' outputs get NaN sentinels on either side
    buf = torch.full((int(np.prod(shape)) + 128,), float("nan"), device="cuda")
    return buf[64:-64].view(*shape), buf
  lib, S, P = _lib.load(), _lib.current_stream(), _lib.ptr
  xp = dense(_cuda(d["x"]).reshape(B * T, E), _cuda(d["kernel"]), _cuda(d["bias"]))
  rk, m, h0, c0 = (_cuda(d[k]) for k in ("recurrent_kernel", "mask", "h0", "c0"))
  outs = [guarded(B, T, U), guarded(B, U), guarded(B, U)] + [guarded(B, T, U) for _ in range(6)]
  _lib.check(lib.tfrs_lstm_fwd(P(xp), P(rk), P(m), P(h0), P(c0), B, T, U, 0, *[P(o[0]) for o in outs], S))
  grads = [guarded(B, T, 4 * U), guarded(B, U), guarded(B, U)]
  dseq, dh, dc = (_cuda(d[k]) for k in ("wseq", "wh", "wc"))
  _lib.check(lib.tfrs_lstm_bwd(P(rk), P(m), *[P(o[0]) for o in outs[3:8]], P(dseq), P(dh), P(dc), B, T, U, 0,
                               *[P(g[0]) for g in grads], S))
  for view, buf in outs + grads:
    assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[-64:]).all()) and not bool(torch.isnan(view).any())
  assert _same({k: a[k] for k in ("seq", "h", "c")}, dict(zip(("seq", "h", "c"), (o[0] for o in outs))))
  assert _same({"dh0": a["dh0"], "dc0": a["dc0"]}, {"dh0": grads[1][0], "dc0": grads[2][0]})


def test_tutorial_tower_trains_and_the_captured_step_matches_the_eager_one():
  import recommenders_amd as tfrs

  class Sequential(tfrs.Model):
    def __init__(self):
      super().__init__()
      self.embedding = tfrs.layers.Embedding(50, 16, mask_zero=True)
      self.lstm = tfrs.layers.LSTM(32)
      self.lstm.build(16, "cuda")
      self.candidates = tfrs.layers.Embedding(40, 32)
      self.task = tfrs.tasks.Retrieval()

    def compute_loss(self, features, training=False):
      ids, emb = features["history"], self.embedding
      return self.task(self.lstm(emb(ids), mask=emb.compute_mask(ids)), self.candidates(features["movie_id"]),
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
  assert len(params) == 5 and all(_bits(e, g) and not _bits(b, e) for b, e, g in params)


def test_units_above_the_envelope_are_refused_by_both_entry_points():
  from recommenders_amd import _lib
  lib, S = _lib.load(), _lib.current_stream()
  for call in (lambda: lib.tfrs_lstm_fwd(*[None] * 5, 4, 3, 65, 0, *[None] * 9, S),
               lambda: lib.tfrs_lstm_bwd(*[None] * 10, 4, 3, 65, 0, None, None, None, S)):
    with pytest.raises(NotImplementedError, match="units"):
      _lib.check(call())


@pytest.mark.parametrize("B,T", [(0, 9), (4, 0), (0, 0)])
def test_empty_batches_return_the_initial_state(B, T):
  from recommenders_amd.layers import LSTM
  layer = LSTM(9, return_sequences=True, return_state=True)
  layer.build(E, "cuda")
  x = torch.zeros((B, T, E), device="cuda", requires_grad=True)
  h0, c0 = (torch.full((B, 9), v, device="cuda", requires_grad=True) for v in (0.5, -2.0))
  seq, h, c = layer(x, initial_state=[h0, c0])
  assert tuple(seq.shape) == (B, T, 9) and torch.equal(h, h0) and torch.equal(c, c0)
  (seq.sum() + (2.0 * h).sum() + (3.0 * c).sum()).backward()
  assert tuple(x.grad.shape) == (B, T, E) and all(not bool(p.grad.any()) for p in layer.parameters())
  assert bool((h0.grad == 2.0).all()) and bool((c0.grad == 3.0).all())
