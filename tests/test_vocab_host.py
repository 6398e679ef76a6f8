"""IntegerLookup / StringLookup without a GPU: constructor and vocabulary errors, the restated table against a
dict on the hand-built cases of the GPU suite, and the argument checks of the C entries."""

import numpy as np
import pytest
import torch

from tests import vocab_restatement as vr


@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


def _layers():
  import recommenders_amd as tfrs
  return tfrs.layers.IntegerLookup, tfrs.layers.StringLookup


def test_layers_are_exported():
  import recommenders_amd as tfrs
  from recommenders_amd.layers import preprocessing
  assert tfrs.layers.IntegerLookup is preprocessing.IntegerLookup
  assert tfrs.layers.StringLookup is preprocessing.StringLookup
  for cls in _layers():
    for name in ("adapt", "set_vocabulary", "get_vocabulary", "vocabulary_size"):
      assert callable(getattr(cls, name))


def test_constructor_errors():
  IntegerLookup, StringLookup = _layers()
  for cls in (IntegerLookup, StringLookup):
    with pytest.raises(NotImplementedError, match="multi_hot"):
      cls(output_mode="multi_hot")
    with pytest.raises(NotImplementedError):
      cls(output_mode="tf_idf")
    with pytest.raises(ValueError, match="num_oov_indices"):
      cls(num_oov_indices=-1)
  with pytest.raises(ValueError, match="differ"):
    IntegerLookup(mask_token=-1)          # equals the default oov_token
  layer = IntegerLookup(mask_value=0)      # the spelling of the reference's dcn tutorial
  assert layer.mask_token == 0 and layer.vocabulary_size() == 2
  assert layer.get_vocabulary() == [0, -1]
  assert StringLookup(num_oov_indices=2).get_vocabulary() == ["[UNK]", "[UNK]"]


@pytest.mark.parametrize("vocabulary", [[4, 9, 4], np.array([1, 2, 3, 1]), torch.tensor([7, 7])])
def test_repeated_tokens_raise(vocabulary):
  IntegerLookup, _ = _layers()
  with pytest.raises(ValueError, match="repeated"):
    IntegerLookup(vocabulary=vocabulary)


def test_repeated_strings_raise():
  _, StringLookup = _layers()
  with pytest.raises(ValueError, match="repeated"):
    StringLookup(vocabulary=["a", "b", b"a"])     # bytes next to str: the same token
  layer = StringLookup()
  with pytest.raises(ValueError, match="repeated"):
    layer.set_vocabulary(np.array(["x", "y", "x"]))


def test_misplaced_special_tokens_raise():
  IntegerLookup, StringLookup = _layers()
  with pytest.raises(ValueError, match="OOV token"):
    IntegerLookup(vocabulary=[5, -1, 6])
  with pytest.raises(ValueError, match="mask token"):
    IntegerLookup(vocabulary=[5, 0, 6], mask_token=0)
  with pytest.raises(ValueError, match="reserved"):                # the mask leads, but the OOV token does not follow it
    IntegerLookup(vocabulary=[0, 5, -1], mask_token=0)
  with pytest.raises(ValueError, match="OOV token"):               # only ONE of the two OOV slots leads
    IntegerLookup(vocabulary=[-1, 5, 6], num_oov_indices=2)
  with pytest.raises(ValueError, match="OOV token"):
    StringLookup(vocabulary=["a", "[UNK]"])
  with pytest.raises(ValueError, match="mask token"):
    StringLookup(vocabulary=["a", ""], mask_token="")
  with pytest.raises(ValueError, match="OOV token"):
    StringLookup(vocabulary=["a", "?"], oov_token="?")


def test_max_tokens_too_small_raises():
  IntegerLookup, StringLookup = _layers()
  with pytest.raises(ValueError, match="max_tokens=3"):
    IntegerLookup(vocabulary=[1, 2, 3], max_tokens=3)               # 3 tokens + 1 OOV slot
  with pytest.raises(ValueError, match="max_tokens=4"):
    IntegerLookup(vocabulary=[1, 2, 3], max_tokens=4, mask_token=0)  # ... + the mask
  with pytest.raises(ValueError, match="max_tokens=2"):
    StringLookup(vocabulary=["a", "b"], max_tokens=2)
  with pytest.raises(ValueError, match="max_tokens=4"):               # leading special tokens are stripped, then counted once
    IntegerLookup(vocabulary=[0, -1, 1, 2, 3], max_tokens=4, mask_token=0)


def test_float_and_bool_input_raise():
  IntegerLookup, StringLookup = _layers()
  layer = IntegerLookup()
  for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool), np.zeros(3, np.float32), [0.5, 1.5]):
    with pytest.raises(ValueError, match="integer"):
      layer(bad)
  with pytest.raises(ValueError, match="integer"):
    IntegerLookup(vocabulary=[1.5, 2.5])
  with pytest.raises(ValueError, match="integer"):
    layer.adapt(torch.zeros(3))
  with pytest.raises(ValueError, match="string"):
    StringLookup()(np.zeros(3))
  with pytest.raises(ValueError, match="string"):
    StringLookup()(torch.zeros(3, dtype=torch.long))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_layers_fail_loudly_without_gpu():
  IntegerLookup, StringLookup = _layers()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    IntegerLookup(vocabulary=[3, 1, 2])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    StringLookup(vocabulary=["a", "b"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    IntegerLookup()(torch.tensor([1, 2]))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    StringLookup()(["a"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    IntegerLookup().adapt(torch.tensor([1, 2, 2]))


# ---- the restated table against a dict --------------------------------------------------------------
def _check_table(tokens, queries, capacity=None):
  table = vr.ProbeTable(tokens, capacity)
  want = {t: i for i, t in enumerate(tokens)}
  assert not table.duplicate
  for q in queries:
    value, steps = table.lookup(q)
    assert value == want.get(q, -1), q
    assert steps <= table.capacity
  return table


def test_restated_table_one_token():
  table = _check_table([42], [42, 41, 43, 0, -1], capacity=2)
  assert table.capacity == vr.capacity_for(1) == 2 and len(table.occupied()) == 1


def test_restated_table_wrapping_chain():
  tokens, absent_home, absent_chain, absent_free = vr.chain_case()
  assert all(vr.home(t, 16) == 13 for t in tokens + absent_home)
  assert [vr.home(q, 16) for q in absent_chain] == [14, 15, 0, 2, 4]
  assert [vr.home(q, 16) for q in absent_free] == [5, 9, 12]
  table = _check_table(tokens, tokens + absent_home + absent_chain + absent_free)
  assert table.capacity == 16 and table.occupied() == [0, 1, 2, 3, 4, 13, 14, 15]
  assert table.lookup(tokens[-1]) == (7, 8)            # the last token sits at the chain's end
  assert table.lookup(absent_home[0]) == (-1, 9)       # walks the whole chain to the first free slot
  assert table.lookup(absent_free[0]) == (-1, 1)


def test_restated_table_extreme_keys():
  keys = [vr.INT64_MIN, vr.INT64_MAX, 0, -1]
  table = _check_table(keys, keys + [1, -2, vr.INT64_MIN + 1, vr.INT64_MAX - 1])
  assert table.empty_value == 0 and len(table.occupied()) == 3      # the empty marker's value never enters the table
  assert _check_table([5, 6], [vr.INT64_MIN, 5]).lookup(vr.INT64_MIN) == (-1, 0)
  assert vr.ProbeTable([3, 4, 3]).duplicate
  assert vr.ProbeTable([vr.INT64_MIN, 1, vr.INT64_MIN]).duplicate


def test_restated_mixer_matches_its_array_form():
  xs = [0, 1, -1, 13, vr.INT64_MIN, vr.INT64_MAX, 0x123456789ABCDEF]
  assert [vr.mix(x) for x in xs] == [int(v) for v in vr.mix_array(np.array(xs, dtype=np.int64))]
  assert vr.mix(0) == 0 and vr.mix(1) == 0xB456BCFC34C2CB2C     # MurmurHash3 fmix64(1)


def test_restated_lookup_rules():
  vocab = [40, -3, 7]
  ids = np.array([[7, 40, 0], [-3, 5, -5]])
  np.testing.assert_array_equal(vr.integer_lookup(ids, vocab), [[3, 1, 0], [2, 0, 0]])
  np.testing.assert_array_equal(vr.integer_lookup(ids, vocab, mask_token=0, num_oov=3), [[6, 4, 0], [5, 3, 2]])
  np.testing.assert_array_equal(vr.integer_lookup(ids, vocab, num_oov=0), [[2, 0, -1], [1, -1, -1]])
  assert vr.vocabulary_size(vocab, 0, 3) == 7
  assert vr.adapt_order([[1, 2, 2], [3, 3, -1, 0], [9]], mask_token=0, oov_token=-1) == [3, 2, 9, 1]
  assert vr.adapt_order([[1, 2, 2], [3, 3, 9]], None, -1, num_oov=1, max_tokens=4) == [3, 2, 9]
  assert vr.adapt_order([["a", b"b", "b"], ["zz", "zz", "c"]], None, "[UNK]", strings=True) == [b"zz", b"b", b"c", b"a"]
  assert vr.inverse([0, 1, 2, 4, 5, -1], vocab, 0, -1) == [0, -1, 40, 7, -1, -1]


# ---- the C entries' argument checks (before any HIP call) --------------------------------------------
def test_c_entries_reject_bad_arguments(lib):
  from recommenders_amd import _lib
  E = _lib.TFRS_EINVAL
  assert lib.tfrs_vocab_build(None, 4, None, 8, None, None) == E
  assert "NULL" in _lib.last_error()
  buf = np.zeros(64, dtype=np.int64)     # host memory: never dereferenced, the checks come first
  p = buf.ctypes.data
  assert lib.tfrs_vocab_build(p, 4, p, 24, p, None) == E
  assert "power of two" in _lib.last_error()
  assert lib.tfrs_vocab_build(p, 5, p, 8, p, None) == E           # 8 < 2 * 5
  assert lib.tfrs_vocab_build(p, 1, p, 1, p, None) == E
  assert lib.tfrs_vocab_build(p, 0, p, 0, p, None) == E
  assert lib.tfrs_vocab_build(p, -1, p, 8, p, None) == E
  look = lambda ids, n, table, cap, n_tokens, out: lib.tfrs_vocab_lookup(
      ids, 1, n, table, cap, n_tokens, 1, 0, 0, -1, 0, 1, 0, None, out, None)
  assert look(None, 4, None, 8, 4, None) == E
  assert look(p, 4, p, 8, 4, None) == E and "NULL" in _lib.last_error()
  assert look(None, 4, p, 8, 4, p) == E
  assert look(p, 4, p, 24, 3, p) == E and "power of two" in _lib.last_error()
  assert look(p, 4, p, 8, 5, p) == E and "power of two" in _lib.last_error()
  assert look(p, 4, p, 0, 0, p) == E
  # a bad index layout: an empty_value that is no vocabulary position
  assert lib.tfrs_vocab_lookup(p, 1, 4, p, 8, 4, 1, 0, 0, 4, 0, 1, 0, None, p, None) == E
  assert lib.tfrs_fingerprint_bytes(None, None, 4, None, None) == E
  assert lib.tfrs_fingerprint_bytes(p, p, -1, p, None) == E
  with pytest.raises(ValueError, match="vocab_build"):
    _lib.check(lib.tfrs_vocab_build(p, 4, p, 24, p, None))
