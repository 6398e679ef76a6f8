"""Host-side tests of the LSTM layer: the constructor's refusals, initialisers and weight plumbing.
No GPU."""

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("kwargs,word", [
    ({"activation": "relu"}, "activation"), ({"recurrent_activation": "hard_sigmoid"}, "recurrent_activation"),
    ({"dropout": 0.1}, "dropout"), ({"recurrent_dropout": 0.1}, "recurrent_dropout"), ({"stateful": True}, "stateful"),
    ({"unroll": True}, "unroll"), ({"time_major": True}, "time_major"), ({"units": 65}, "units")])
def test_what_is_not_built_is_refused_at_construction(kwargs, word):
  from recommenders_amd import layers
  with pytest.raises(NotImplementedError, match=word):
    layers.LSTM(**{"units": 8, **kwargs})


def test_export():
  from recommenders_amd import layers
  from recommenders_amd.layers.recurrent import LSTM
  assert layers.LSTM is LSTM and LSTM(64).get_weights() == []


@pytest.mark.parametrize("unit_forget_bias", (True, False))
def test_initialisers(unit_forget_bias):
  from recommenders_amd.layers import LSTM
  torch.manual_seed(7)
  U, E = 24, 40
  layer = LSTM(U, unit_forget_bias=unit_forget_bias, device="cpu")
  layer.build(E)
  want = np.zeros(4 * U, np.float32)
  want[U:2 * U] = 1.0 if unit_forget_bias else 0.0
  assert np.array_equal(layer.bias.detach().numpy(), want)
  k, lim = layer.kernel.detach().numpy(), np.sqrt(6.0 / (E + 4 * U))
  assert k.shape == (E, 4 * U) and 0.98 * lim < np.abs(k).max() <= lim
  r = layer.recurrent_kernel.detach().numpy().astype(np.float64).reshape(U, 4, U)      # four orthogonal blocks
  assert all(np.abs(r[:, g] @ r[:, g].T - np.eye(U)).max() < 1e-5 for g in range(4))
  assert np.abs(r[:, 2] - r[:, 3]).max() > 0.1                                        # ... four draws, not one


def test_weights_round_trip_and_shape_errors():
  from recommenders_amd.layers import LSTM
  rng = np.random.default_rng(5)
  ws = [rng.normal(size=s).astype(np.float32) for s in ((5, 28), (7, 28), (28,))]
  layer = LSTM(7, device="cpu")
  layer.set_weights(ws)
  other = LSTM(7, device="cpu")                       # not built: takes its input width from the state
  other.load_state_dict(layer.state_dict())
  assert sorted(layer.state_dict()) == ["bias", "kernel", "recurrent_kernel"]
  for got, want in zip(other.get_weights(), ws):
    assert got.dtype == np.float32 and np.array_equal(got, want)
  for bad in (ws[:2], [ws[0][:, :-1], ws[1], ws[2]], [ws[0], ws[1].T, ws[2]], [ws[0], ws[1], ws[2][None]],
              [ws[0][:-1], ws[1], ws[2]]):
    with pytest.raises(ValueError):
      layer.set_weights(bad)
