"""Float64 restatement of the GRU layer: forward, masks, go_backwards, initial_state and full BPTT
gradients, written from the formulas with numpy, plus the yardstick and the limits the GPU tests hold the kernels to
and the shapes and mask builders the two test files share.  Test infrastructure only: it shares no code with the
product.

Formulas (Keras' default GRU, reset_after=True, gates z, r, h; K = kernel [E, 3U], R = recurrent_kernel [U, 3U],
b = bias [2, 3U]):
  a   = x_t K + b[0]                       q = h_{t-1} R + b[1]
  z   = sigma(a_z + q_z)                   r = sigma(a_r + q_r)            hh = tanh(a_h + r q_h)
  h_t = z h_{t-1} + (1 - z) hh             mask[b, t] false: h_t = h_{t-1} (the output at t repeats)
  backward, t from last to first, dh carried:
  dh += d out_t;  dhh = dh (1 - z);  dz = dh (h_prev - hh);  dh_prev = dh z
  da_h = dhh (1 - hh^2);  dq_h = da_h r;  dr = da_h q_h;  da_z = dz z (1 - z);  da_r = dr r (1 - r)
  dh_prev += [da_z, da_r, dq_h] R^T;  da = [da_z, da_r, da_h];  dG = [da_z, da_r, dq_h]
  dK = x^T da,  db[0] = sum da,  dx = da K^T,  dR = H_prev^T dG,  db[1] = sum dG  (sums over all rows and steps)

The yardstick of an entry is the sum of the absolute values of the terms that make it up (conftest.float_gate):
  h_t          Y_t = |z| Y_{t-1} + (1 - z) (|hh| + (1 - hh^2) P_h) + |h_{t-1} - hh| z (1 - z) P_z,  Y_0 = |h0|; a masked
               step carries Y.  P_z, P_r = sum |x_k K_k| + |b| + sum |h_k R_k| + |b| are the terms of the pre-activations,
               P_h = sum |x_k K_k| + |b| + r (sum |h_k R_k| + |b|) + |q_h| r (1 - r) P_r; they enter h_t with the gates'
               slopes: hh = tanh(p) can be a small difference of large terms, and then |hh| alone is no yardstick.
               The terms are those of THIS step (|h_{t-1}|, not Y_{t-1}, multiplies |R|): nothing is carried through R
  dh           adding the step's output gradient: Y += |d out_t|;  an unmasked step: Y = |z| Y + sum_j |dG_j| |R_nj|;
               dh0 is the last dh
  dx           sum_j |da_j| |K_ej|   (0 at a masked step: the gradient there is +0 exactly)
  dK, dR       sum over rows and steps of |x| |da|, |h_prev| |dG|;   db: sum |da|, sum |dG|
|z| < 1, so no yard grows with T: a yard is of the size of the entry's own terms.  (A running bound through the
ABSOLUTE step Jacobians with the gates' Lipschitz constants was tried first; it grows like (1 + |R|_1)^T and at
T = 9, U = 64 stood 10^3 .. 10^8 above the float32 error of the same case: it gated nothing.)

The limit.  An entry's float32 error has a part that can be derived and a part that cannot.
  derived     ONE step's local error: a U-term dot product is off by at most U eps sum |terms| in any order, pushed
              through the gates with their Lipschitz constants (sigma 1/4, tanh 1), plus the roundings of the step's sums
              and products.  What earlier steps left in h_{t-1} reaches h_t through the step Jacobian
              d h_t / d h_{t-1}, which is what the float32 recurrence below applies in float32 to its own earlier errors.
  measured    the error of the device's exp / tanh / divide and how the local errors of T steps add up through those
              Jacobians.  The same recurrence runs in float32 with torch on the CPU on the SAME inputs
              (`float32_errors`), its error against the float64 values is taken in this yardstick, per case and per
              gate, and the kernel gets 4 x that (`limits`): the margin every float_gate tier of conftest.py uses,
              because summation order and transcendental implementation differ.
  floor       a case with a handful of entries (B = 1, U = 1) or with nothing but carried values observes a maximum
              over too few roundings to measure anything (the CPU run can be exact there).  The allowance of a gate is
              therefore never below ALLOWANCE_FLOOR = 16 eps of the yard: one step's transcendental charge as
              tests/pairsum_restatement.py counts it (sigma: exp 4, the addition 1, the division 4, the rounded
              argument 1 = 10 eps; tanh the same budget; both gates enter an entry, weighted by |h - hh| <= 2 and
              (1 - z) <= 1, against a yard that is at least the entry) plus 6 roundings of the blend and the sums.
              The limit is thus never below 64 eps = 3.8e-6 of the sum of |terms|: a 1 % error fails it by three
              orders of magnitude (tests/test_gru_host.py proves that for every case and gate).
"""

import functools
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -24
ALLOWANCE_FLOOR = 16.0 * EPS

Entry = namedtuple("Entry", "value yard")


def _sigma(p):
  e = np.exp(-np.abs(p))
  return np.where(p >= 0.0, 1.0, e) / (1.0 + e)


def gru(x, kernel, recurrent_kernel, bias=None, mask=None, initial_state=None, go_backwards=False,
        wseq=None, wlast=None):
  """The layer on float32-valued inputs, in float64.  Returns a dict of Entry: "seq" [B, T, U] in processing order,
  "last" [B, U] and -- when `wseq` [B, T, U] and / or `wlast` [B, U] give the linear loss
  sum(wseq * seq) + sum(wlast * last) -- its gradients "dx", "dh0", "dkernel", "drecurrent", "dbias" ([2, 3U])."""
  f64 = lambda a: np.asarray(a, dtype=np.float64)
  x, K, R = f64(x), f64(kernel), f64(recurrent_kernel)
  B, T, E = x.shape
  U = R.shape[0]
  b0 = f64(bias[0]) if bias is not None else 0.0
  b1 = f64(bias[1]) if bias is not None else 0.0
  live = np.ones((B, T), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
  order = list(range(T - 1, -1, -1)) if go_backwards else list(range(T))
  h = np.zeros((B, U)) if initial_state is None else f64(initial_state)
  yh = np.abs(h)
  steps, seq, yseq = [], [], []
  for tt in order:
    a = x[:, tt, :] @ K + b0
    q = h @ R + b1
    z = _sigma(a[:, :U] + q[:, :U])
    r = _sigma(a[:, U:2 * U] + q[:, U:2 * U])
    qh = q[:, 2 * U:]
    hh = np.tanh(a[:, 2 * U:] + r * qh)
    m = live[:, tt][:, None]
    steps.append((tt, m, z, r, hh, qh, h))
    # sums of |terms| of the three pre-activations (the gates turn them into h_t with slopes z (1 - z), 1 - hh^2)
    ax, ah = np.abs(x[:, tt, :]) @ np.abs(K) + np.abs(b0), np.abs(h) @ np.abs(R) + np.abs(b1)
    pz, pr = ax[:, :U] + ah[:, :U], ax[:, U:2 * U] + ah[:, U:2 * U]
    ph = ax[:, 2 * U:] + r * ah[:, 2 * U:] + np.abs(qh) * r * (1.0 - r) * pr
    local = np.abs(h - hh) * z * (1.0 - z) * pz + (1.0 - z) * (np.abs(hh) + (1.0 - hh * hh) * ph)
    yh = np.where(m, z * yh + local, yh)
    h = np.where(m, z * h + (1.0 - z) * hh, h)
    seq.append(h)
    yseq.append(yh)
  out = {"last": Entry(h, yh)}
  out["seq"] = (Entry(np.stack(seq, axis=1), np.stack(yseq, axis=1)) if T else
                Entry(np.zeros((B, 0, U)), np.zeros((B, 0, U))))
  if wseq is None and wlast is None:
    return out
  # ---- BPTT ----
  dh = np.zeros((B, U)) if wlast is None else f64(wlast)
  ydh = np.abs(dh)
  da, dg, hp_all = np.zeros((B, T, 3 * U)), np.zeros((B, T, 3 * U)), np.zeros((B, T, U))
  for t in range(T - 1, -1, -1):
    tt, m, z, r, hh, qh, hp = steps[t]
    if wseq is not None:
      dh = dh + f64(wseq)[:, t, :]
      ydh = ydh + np.abs(f64(wseq)[:, t, :])
    dhh = dh * (1.0 - z)
    dz = dh * (hp - hh)
    dah = dhh * (1.0 - hh * hh)
    dqh = dah * r
    dr = dah * qh
    daz = dz * z * (1.0 - z)
    dar = dr * r * (1.0 - r)
    dG = np.concatenate([daz, dar, dqh], axis=1)
    da[:, tt] = np.where(m, np.concatenate([daz, dar, dah], axis=1), 0.0)
    dg[:, tt] = np.where(m, dG, 0.0)
    hp_all[:, tt] = hp
    ydh = np.where(m, z * ydh + np.abs(dG) @ np.abs(R.T), ydh)
    dh = np.where(m, dh * z + dG @ R.T, dh)
  out["dh0"] = Entry(dh, ydh)
  da2, dg2, hp2, x2 = da.reshape(B * T, 3 * U), dg.reshape(B * T, 3 * U), hp_all.reshape(B * T, U), x.reshape(B * T, E)
  out["dx"] = Entry((da2 @ K.T).reshape(B, T, E), (np.abs(da2) @ np.abs(K.T)).reshape(B, T, E))
  out["dkernel"] = Entry(x2.T @ da2, np.abs(x2.T) @ np.abs(da2))
  out["drecurrent"] = Entry(hp2.T @ dg2, np.abs(hp2.T) @ np.abs(dg2))
  if bias is not None:
    out["dbias"] = Entry(np.stack([da2.sum(axis=0), dg2.sum(axis=0)]),
                         np.stack([np.abs(da2).sum(axis=0), np.abs(dg2).sum(axis=0)]))
  return out


# ---- shapes, masks and options shared by the test files --------------------------------------------------------------
BATCHES = (1, 31, 32, 33, 65)                 # inside, at and across the 32-row tile; one and several workgroups
UNITS = (1, 8, 9, 32, 33, 64)                 # every padding edge, one wave and two, up to the kernels' 64 units
MASKS = ("none", "all_true", "row_all_false", "right", "left", "holes")

# (return_sequences, return_state, go_backwards, initial_state, use_bias)
OPTIONS = (
    (False, False, False, False, True),
    (True, False, False, True, True),
    (True, True, False, False, False),
    (False, True, True, True, True),
    (True, True, True, True, False),
    (False, False, True, False, False),
)

Case = namedtuple("Case", "B T E U mask opts seed")


def _cases():
  out = []
  i = 0

  def add(B, T, E, U, mask=None):
    nonlocal i
    mk = MASKS[i % len(MASKS)] if mask is None else mask
    if mk != "none":
      T = 9                                   # T = 9 wherever masks are involved
    out.append(Case(B, T, E, U, mk, OPTIONS[i % len(OPTIONS)], 1000 + i))
    i += 1

  for U in UNITS:                             # every U at one B across the tile edge
    add(33, 2, 33, U)
  for U in (9, 33, 64):                       # every B at three U: padded, two waves, full
    for B in BATCHES:
      add(B, 9, 1 if (B + U) % 2 else 33, U)
  add(33, 1, 1, 9, "none")                    # T = 1, E = 1
  add(1, 1, 33, 64, "none")
  add(65, 2, 1, 33, "none")
  for mk in MASKS:                            # every mask kind at the widest kernel too
    add(33, 9, 33, 64, mk)
  return tuple(out)


def make_mask(kind, B, T, rng):
  """[B, T] bool, or None."""
  if kind == "none":
    return None
  m = np.ones((B, T), dtype=bool)
  if kind == "all_true":
    return m
  if kind == "row_all_false":
    m = rng.random((B, T)) < 0.7
    m[0] = False
    m[B // 2] = False
    return m
  if kind in ("right", "left"):
    lengths = np.array([(3 * b) % (T + 1) for b in range(B)])       # 0, 3, 6, 9, 2, ...: includes 0 and T
    if B > 1:
      lengths[-1] = T
    pos = np.arange(T)[None, :]
    return pos < lengths[:, None] if kind == "right" else pos >= (T - lengths)[:, None]
  if kind == "holes":
    m = rng.random((B, T)) < 0.6
    m[:, 0] = True
    m[:, -1] = True
    if T > 2:
      m[:, T // 2] = False
    return m
  raise ValueError(kind)


def make_inputs(case):
  """float32 arrays of one case: x, kernel, recurrent_kernel, bias (or None), mask (or None), h0 (or None),
  wseq (or None), wlast (or None) -- the loss is sum(wseq * seq) + sum(wlast * last) over what the layer returns."""
  rng = np.random.default_rng(case.seed)
  B, T, E, U = case.B, case.T, case.E, case.U
  seq, state, _, with_h0, with_bias = case.opts
  f = lambda a: np.asarray(a, dtype=np.float32)
  lim = np.sqrt(6.0 / (E + 3 * U))
  d = {
      "x": f(rng.normal(size=(B, T, E))),
      "kernel": f(rng.uniform(-lim, lim, size=(E, 3 * U)) * 2.0),
      "recurrent_kernel": f(rng.normal(size=(U, 3 * U)) / np.sqrt(U)),
      "bias": f(rng.normal(size=(2, 3 * U)) * 0.25) if with_bias else None,
      "mask": make_mask(case.mask, B, T, rng),
      "h0": f(rng.normal(size=(B, U)) * 0.5) if with_h0 else None,
      "wseq": f(rng.normal(size=(B, T, U))) if seq else None,
      "wlast": f(rng.normal(size=(B, U))) if (state or not seq) else None,
  }
  return d


def restate(case, d=None):
  d = make_inputs(case) if d is None else d
  return gru(d["x"], d["kernel"], d["recurrent_kernel"], d["bias"], d["mask"], d["h0"], case.opts[2], d["wseq"],
             d["wlast"])


CASES = _cases()
GATES = {"seq": "gru.fwd.seq", "last": "gru.fwd.last", "dx": "gru.bwd.dx", "dh0": "gru.bwd.dh0",
         "dkernel": "gru.bwd.dkernel", "drecurrent": "gru.bwd.drecurrent", "dbias": "gru.bwd.dbias"}
FLOOR = 2.0 ** -126


def ratio(got, entry):
  """max |got - value| / yard, the float_gate statistic."""
  got = np.asarray(got, dtype=np.float64)
  if got.size == 0:
    return 0.0
  return float(np.max(np.abs(got - entry.value) / np.maximum(entry.yard, FLOOR)))


def torch_recurrence(d, go_backwards, dtype):
  """The same recurrence with torch on the CPU in `dtype`, gradients by autograd: dict like gru()'s, plain arrays."""
  import torch
  t_ = lambda a, g=False: None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=g)
  x, K, R = t_(d["x"], True), t_(d["kernel"], True), t_(d["recurrent_kernel"], True)
  bias = t_(d["bias"], True)
  B, T, E = x.shape
  U = R.shape[0]
  h0 = t_(d["h0"], True)
  mask = None if d["mask"] is None else torch.tensor(d["mask"])
  a = x.reshape(B * T, E) @ K
  if bias is not None:
    a = a + bias[0]
  a = a.reshape(B, T, 3 * U)
  h = h0 if h0 is not None else torch.zeros((B, U), dtype=dtype)
  outs = []
  for t in range(T):
    tt = T - 1 - t if go_backwards else t
    q = h @ R
    if bias is not None:
      q = q + bias[1]
    z = torch.sigmoid(a[:, tt, :U] + q[:, :U])
    r = torch.sigmoid(a[:, tt, U:2 * U] + q[:, U:2 * U])
    hh = torch.tanh(a[:, tt, 2 * U:] + r * q[:, 2 * U:])
    hn = z * h + (1.0 - z) * hh
    h = hn if mask is None else torch.where(mask[:, tt][:, None], hn, h)
    outs.append(h)
  seq = torch.stack(outs, dim=1) if T else torch.zeros((B, 0, U), dtype=dtype)
  out = {"seq": seq.detach().numpy(), "last": h.detach().numpy()}
  loss = None
  if d["wseq"] is not None:
    loss = (seq * t_(d["wseq"])).sum()
  if d["wlast"] is not None:
    loss = (h * t_(d["wlast"])).sum() + (0.0 if loss is None else loss)
  if loss is not None and loss.requires_grad:
    loss.backward()
    z_ = lambda p, like: np.zeros_like(like) if p.grad is None else p.grad.numpy()
    out.update(dx=z_(x, d["x"]), dkernel=z_(K, d["kernel"]), drecurrent=z_(R, d["recurrent_kernel"]))
    if h0 is not None:
      out["dh0"] = z_(h0, d["h0"])
    if bias is not None:
      out["dbias"] = z_(bias, d["bias"])
  return out


@functools.lru_cache(maxsize=None)
def float32_errors(case):
  """{key: ratio} of the float32 CPU recurrence against the float64 restatement on the inputs of `case`, in the
  restatement's yardstick."""
  import torch
  d = make_inputs(case)
  ref = restate(case, d)
  got = torch_recurrence(d, case.opts[2], torch.float32)
  return {k: ratio(got[k], ref[k]) for k in got if k in ref}


def limits(case):
  """{gate name: limit} of one case: 4 x max(the float32 CPU ratio of this case and gate, ALLOWANCE_FLOOR)."""
  measured = float32_errors(case)
  return {GATES[k]: 4.0 * max(measured.get(k, 0.0), ALLOWANCE_FLOOR) for k in GATES}


# ---- the halving test ------------------------------------------------------------------------------------------------
def halving_state(B, U):
  """initial_state [B, U] float32 of small distinct integers (1 .. 2^11 at most, B U <= 65 * 64 < 2^13: the values
  are (b U + j) mod 2039 + 1, distinct within every row and between neighbouring rows)."""
  idx = np.arange(B * U, dtype=np.int64).reshape(B, U)
  return (idx % 2039 + 1).astype(np.float32)


def halving_expected(h0, mask, T, go_backwards):
  """([B, T, U] sequence in processing order, [B, U] last) of the layer with all-zero weights: h0 * 2^-(unmasked steps
  so far).  Exact in float32 and float64 alike: a power-of-two scaling of an integer below 2^11 by at most 2^-T."""
  B, U = h0.shape
  live = np.ones((B, T), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
  if go_backwards:
    live = live[:, ::-1]
  counts = np.cumsum(live, axis=1)                                   # unmasked steps up to and including step t
  seq = h0[:, None, :].astype(np.float64) * (2.0 ** -counts)[:, :, None]
  last = seq[:, -1, :] if T else h0.astype(np.float64)
  return seq.astype(np.float32), last.astype(np.float32)
