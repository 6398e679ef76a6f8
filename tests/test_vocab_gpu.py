"""``IntegerLookup`` / ``StringLookup`` on the MI355X (``csrc/vocab.hip``, ``tfrs_fingerprint_bytes``): every
comparison is exact integer equality against the NumPy / dict restatement of tests/vocab_restatement.py --
hand-built tables at the layout's edges, the launch's edges, a build under contention, random vocabularies
over the index layouts, input structures, ``adapt``, ``invert``, strings, persistence, a captured lookup and the
layer in front of an ``Embedding``."""

import numpy as np
import pytest
import torch

from tests import vocab_restatement as vr

pytestmark = pytest.mark.gpu

GRID_PASS = 2048 * 256     # ids one pass of the capped grid covers (kVocabMaxBlocks x 256 lanes)


def _np(t):
  return t.detach().cpu().numpy()


def _b(token):
  return token if isinstance(token, bytes) else token.encode("utf-8", "surrogateescape")


def _layers():
  import recommenders_amd as tfrs
  return tfrs.layers.IntegerLookup, tfrs.layers.StringLookup


def _ilookup(vocabulary, **kw):
  return _layers()[0](vocabulary=vocabulary, **kw)


def _check(layer, ids, vocabulary, mask_token=None, num_oov=1, dtype=torch.int64):
  ids = np.asarray(ids, dtype=np.int64)
  got = layer(torch.as_tensor(ids).to(dtype).cuda())
  assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == ids.shape
  np.testing.assert_array_equal(_np(got), vr.integer_lookup(ids, vocabulary, mask_token, num_oov))
  return got


def _table_slots(layer):
  keys = _np(layer._table)[:, 0]
  return sorted(np.nonzero(keys != vr.EMPTY_KEY)[0].tolist())


def _random_vocabulary(rng, n, forbidden=(-1,)):
  """n distinct int64 ids: a third small, a third around +-2^40, a third over the whole 64-bit range."""
  pools = [rng.integers(-4 * n - 8, 4 * n + 8, size=2 * n), rng.integers(-(1 << 40), 1 << 40, size=2 * n),
           rng.integers(vr.INT64_MIN, vr.INT64_MAX, size=2 * n, endpoint=True)]
  ids = np.unique(np.concatenate(pools))
  ids = ids[~np.isin(ids, np.asarray(forbidden, dtype=np.int64))]
  return rng.permutation(ids)[:n]


def _mixed_queries(rng, vocabulary, n, extra=()):
  """Half known, half (almost surely) unknown, shuffled; ``extra`` ids appended."""
  known = rng.choice(vocabulary, size=n // 2)
  near = rng.choice(vocabulary, size=n // 4).astype(np.int64) + rng.integers(1, 3, size=n // 4)   # next to a token
  far = rng.integers(vr.INT64_MIN, vr.INT64_MAX, size=n - n // 2 - n // 4, endpoint=True)
  return rng.permutation(np.concatenate([known, near, far, np.asarray(extra, dtype=np.int64)]))


# ---- hand-built tables -------------------------------------------------------------------------
def test_one_token_capacity_two():
  layer = _ilookup([42])
  assert tuple(layer._table.shape) == (2, 2) and len(_table_slots(layer)) == 1
  assert layer.vocabulary_size() == 2 and layer.get_vocabulary() == [-1, 42]
  _check(layer, [42, 41, 43, 0, -1, 42], [42])


def test_chain_wraps_past_the_table_end():
  tokens, absent_home, absent_chain, absent_free = vr.chain_case()
  layer = _ilookup(tokens, num_oov_indices=3)
  assert layer._table.shape[0] == 16
  assert _table_slots(layer) == vr.ProbeTable(tokens).occupied() == [0, 1, 2, 3, 4, 13, 14, 15]
  for queries in (tokens, absent_home, absent_chain, absent_free, tokens + absent_home + absent_chain + absent_free):
    _check(layer, queries, tokens, num_oov=3)
  # whatever order the lanes of the build claimed their slots in, a rebuilt table answers the same
  again = _ilookup(tokens[::-1], num_oov_indices=3)
  _check(again, tokens + absent_home, tokens[::-1], num_oov=3)


@pytest.mark.parametrize("num_oov", [0, 1, 3])
def test_extreme_ids_present_and_absent(num_oov):
  extremes = [vr.INT64_MIN, vr.INT64_MAX, 0, -1]
  queries = extremes + [1, -2, vr.INT64_MIN + 1, vr.INT64_MAX - 1] + extremes
  present = _ilookup(extremes, num_oov_indices=num_oov, oov_token=-99)
  assert len(_table_slots(present)) == 3                      # INT64_MIN is answered outside the table
  _check(present, queries, extremes, num_oov=num_oov)
  absent = _ilookup([5, 6, 7], num_oov_indices=num_oov)
  _check(absent, queries, [5, 6, 7], num_oov=num_oov)
  masked = _ilookup([vr.INT64_MAX, 0], mask_token=vr.INT64_MIN, num_oov_indices=num_oov)
  _check(masked, queries, [vr.INT64_MAX, 0], mask_token=vr.INT64_MIN, num_oov=num_oov)


def test_int32_input_with_negative_ids():
  vocab = [-5, 17, -(1 << 31), (1 << 31) - 1, 0, 1 << 40]
  layer = _ilookup(vocab, num_oov_indices=3, oov_token=-99)
  ids = [-5, -6, -1, -2, -3, -4, 17, 0, -(1 << 31), (1 << 31) - 1, -(1 << 31) + 1, 3]
  _check(layer, ids, vocab, num_oov=3, dtype=torch.int32)
  got = layer(np.asarray(ids, dtype=np.int32))                # NumPy integer arrays are accepted too
  np.testing.assert_array_equal(_np(got), vr.integer_lookup(ids, vocab, None, 3))


# ---- launch edges ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_layer():
  rng = np.random.default_rng(11)
  vocab = _random_vocabulary(rng, 1000)
  return rng, vocab, _ilookup(vocab, num_oov_indices=3)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, GRID_PASS + 65])
def test_launch_edges(edge_layer, n):
  rng, vocab, layer = edge_layer
  ids = _mixed_queries(rng, vocab, n) if n >= 4 else vocab[:n]
  assert ids.size == n
  got = layer(torch.as_tensor(ids).cuda())
  assert tuple(got.shape) == (n,) and got.dtype == torch.int64
  if n <= 1024:
    want = vr.integer_lookup(ids, vocab, None, 3)
  else:    # the same rules in array form: a dict walk over half a million ids is slow
    order = np.argsort(vocab)
    pos = np.clip(np.searchsorted(vocab[order], ids), 0, vocab.size - 1)
    hit = vocab[order][pos] == ids
    want = np.where(hit, 3 + order[pos], np.mod(ids, 3))
    np.testing.assert_array_equal(want[:512], vr.integer_lookup(ids[:512], vocab, None, 3))
  np.testing.assert_array_equal(_np(got), want)


# ---- build under contention ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def contended():
  rng = np.random.default_rng(5)
  crowd = np.asarray(vr.keys_homed_at(77, 1 << 18, 256), dtype=np.int64)       # one home slot, 256 lanes racing
  spread = _random_vocabulary(rng, 100_000, forbidden=crowd.tolist() + [-1])
  vocab = rng.permutation(np.concatenate([spread, crowd]))
  return rng, vocab, crowd


def test_build_under_contention(contended):
  rng, vocab, crowd = contended
  dev = torch.as_tensor(vocab).cuda()
  layer = _ilookup(dev)                                   # a device vocabulary: only the build's CAS checks it
  assert layer._table.shape[0] == 1 << 18 and len(_table_slots(layer)) == vocab.size
  got = layer(dev)
  assert torch.equal(got, 1 + torch.arange(vocab.size, device="cuda"))
  other = _ilookup(dev)
  queries = torch.as_tensor(_mixed_queries(rng, vocab, 10_000 - 256, extra=crowd)).cuda()
  a, b = layer(queries), other(queries)
  assert torch.equal(a, b)
  np.testing.assert_array_equal(_np(a), vr.integer_lookup(_np(queries), vocab))


def test_build_reports_a_repeated_key(contended):
  _, vocab, crowd = contended
  for where in (0, vocab.size // 2):
    repeated = np.concatenate([vocab, vocab[where:where + 1]])
    with pytest.raises(ValueError, match="repeated"):
      _ilookup(torch.as_tensor(repeated).cuda())
  with pytest.raises(ValueError, match="repeated"):
    _ilookup(torch.as_tensor([3, vr.INT64_MIN, 4, vr.INT64_MIN]).cuda())     # the value kept outside the table
  with pytest.raises(ValueError, match="repeated"):
    _ilookup(torch.as_tensor([9, 9]).cuda())


# ---- random cases --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_vocabularies():
  rng = np.random.default_rng(2024)
  return {n: _random_vocabulary(rng, n, forbidden=(-1, 0, -7)) for n in (1, 2, 7, 1000, 100_000)}


@pytest.mark.parametrize("mask_token", [None, 0, -7])
@pytest.mark.parametrize("num_oov", [0, 1, 3])
@pytest.mark.parametrize("size", [1, 2, 7, 1000, 100_000])
def test_random_vocabularies(random_vocabularies, size, num_oov, mask_token):
  vocab = random_vocabularies[size]
  rng = np.random.default_rng(size * 31 + num_oov * 7 + (0 if mask_token is None else mask_token + 9))
  layer = _ilookup(torch.as_tensor(vocab) if size > 1000 else vocab.tolist(), num_oov_indices=num_oov,
                   mask_token=mask_token)
  assert layer.vocabulary_size() == vr.vocabulary_size(vocab, mask_token, num_oov)
  ids = _mixed_queries(rng, vocab, 4096, extra=[0, -7, -1, -8, 1, 2, 3, -2, -3])
  got = _check(layer, ids, vocab, mask_token, num_oov)
  if num_oov == 0:
    unknown = int((got == -1).sum())
    assert unknown == int((vr.integer_lookup(ids, vocab, mask_token, 0) == -1).sum()) > 0
    with pytest.raises(ValueError, match=f"^{unknown} of {ids.size} ids"):
      layer(torch.as_tensor(ids).cuda(), validate=True)
    known = torch.as_tensor(vocab[:64]).cuda()
    assert torch.equal(layer(known, validate=True), layer(known))      # nothing unknown: no error


# ---- shapes ------------------------------------------------------------------------------------
def test_input_structures_are_kept():
  from recommenders_amd.layers.tpu_embedding_layer import RaggedIds, SparseIds
  rng = np.random.default_rng(3)
  vocab = _random_vocabulary(rng, 50)
  layer = _ilookup(vocab, mask_token=0)
  ids = _mixed_queries(rng, vocab, 60)
  want = vr.integer_lookup(ids, vocab, 0, 1)
  flat = torch.as_tensor(ids).cuda()
  for shape in ((60,), (12, 5), (3, 4, 5), (60, 1)):
    got = layer(flat.reshape(shape))
    assert tuple(got.shape) == shape
    np.testing.assert_array_equal(_np(got).reshape(-1), want)
  strided = layer(flat.reshape(12, 5).t())                    # a non-contiguous view
  np.testing.assert_array_equal(_np(strided), want.reshape(12, 5).T)
  splits = [0, 3, 3, 10, 60]
  ragged = layer(RaggedIds(flat, splits))
  assert isinstance(ragged, RaggedIds) and ragged.row_splits.tolist() == splits
  np.testing.assert_array_equal(_np(ragged.values), want)
  indices = np.stack([np.arange(60) // 8, np.arange(60) % 8], axis=1)
  sparse = layer(SparseIds(indices, flat, (8, 8)))
  assert isinstance(sparse, SparseIds) and sparse.dense_shape == (8, 8)
  np.testing.assert_array_equal(_np(sparse.indices), indices)
  np.testing.assert_array_equal(_np(sparse.values), want)


# ---- adapt ---------------------------------------------------------------------------------------
def test_adapt_counts_with_ties_over_three_batches():
  IntegerLookup, _ = _layers()
  batches = [[5, 5, 9, 1 << 40, -3, 0], [9, 5, -3, -1, -1, -1, 7], [[1 << 40, 9], [0, 0]]]
  layer = IntegerLookup(mask_token=0)
  layer.adapt([torch.tensor(batches[0]).cuda(), np.asarray(batches[1]), torch.tensor(batches[2])])
  want = vr.adapt_order(batches, mask_token=0, oov_token=-1)
  assert want == [9, 5, 1 << 40, -3, 7]                       # counts 3, 3, 2, 2, 1: ties by token descending
  assert layer.get_vocabulary(include_special_tokens=False) == want
  assert layer.get_vocabulary() == [0, -1] + want and layer.vocabulary_size() == 7
  _check(layer, [9, 5, 7, 0, -1, 8, -3], want, mask_token=0)
  layer.adapt(torch.tensor([4, 4, 6]))                         # a single batch; adapt starts afresh
  assert layer.get_vocabulary() == [0, -1, 4, 6]


def test_adapt_max_tokens_cuts_inside_a_tie():
  IntegerLookup, _ = _layers()
  batches = [[1, 2, 3, 4, 8, 8, 8], [1, 2, 3, 4]]            # 8, then four tokens tied at two
  for max_tokens, num_oov in ((4, 1), (5, 2), (3, 0)):
    layer = IntegerLookup(max_tokens=max_tokens, num_oov_indices=num_oov)
    layer.adapt([np.asarray(b) for b in batches])
    want = vr.adapt_order(batches, None, -1, num_oov=num_oov, max_tokens=max_tokens)
    assert want == [8, 4, 3] and layer.get_vocabulary(include_special_tokens=False) == want
    assert layer.vocabulary_size() == max_tokens
    _check(layer, [8, 4, 3, 2, 1, 0], want, num_oov=num_oov)


# ---- invert --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_token,num_oov", [(None, 1), (0, 2), (None, 0)])
def test_invert_is_the_inverse(mask_token, num_oov):
  rng = np.random.default_rng(8)
  vocab = _random_vocabulary(rng, 300, forbidden=(-1, 0))
  forward = _ilookup(vocab, mask_token=mask_token, num_oov_indices=num_oov)
  backward = _ilookup(vocab, mask_token=mask_token, num_oov_indices=num_oov, invert=True)
  tokens = torch.as_tensor(vocab).cuda().reshape(20, 15)
  back = backward(forward(tokens))
  assert back.dtype == torch.int64 and back.is_cuda and torch.equal(back, tokens)
  size = backward.vocabulary_size()
  indices = list(range(-2, size + 3))
  got = backward(torch.tensor(indices).cuda())
  assert _np(got).tolist() == vr.inverse(indices, vocab.tolist(), mask_token, -1, num_oov)
  base = vr.layout(mask_token, num_oov)[1]
  assert all(t == -1 for t in _np(got)[2 + (mask_token is not None):2 + base].tolist())   # the OOV slots
  assert _np(got)[-3:].tolist() == [-1, -1, -1] and _np(got)[:2].tolist() == [-1, -1]


# ---- strings -------------------------------------------------------------------------------------
TITLES = ["", "1234567", "12345678", "123456789", "0123456789abcdef", "Amélie (2001)", "千と千尋の神隠し",
          b"Toy Story (1995)", b"\xff\x00raw", "Heat (1995)", "a", "b", "Se7en (1995)"]


def test_fingerprint_entry_against_siphash():
  from recommenders_amd import _lib
  from recommenders_amd.layers.hashing import pack_strings
  strings = TITLES + ["x" * n for n in (15, 17, 24, 31, 255, 256, 1000)]
  arr = np.empty(len(strings), dtype=object)
  arr[:] = strings
  blob, offsets = pack_strings(arr, torch.device("cuda"))
  out = torch.empty((len(strings),), dtype=torch.int64, device="cuda")
  _lib.check(_lib.load().tfrs_fingerprint_bytes(_lib.ptr(blob), _lib.ptr(offsets), len(strings), _lib.ptr(out),
                                                _lib.current_stream()))
  assert _np(out).tolist() == [vr.as_signed(vr.fingerprint(s)) for s in strings]
  # the key is the SipHash paper's 00 01 .. 0f: its known answer for the empty message
  assert vr.fingerprint(b"") == 0x726FDB47DD0E0E31


@pytest.mark.parametrize("mask_token,num_oov", [(None, 1), ("", 3), (None, 0)])
def test_string_lookup(mask_token, num_oov):
  _, StringLookup = _layers()
  vocab = [t for t in TITLES if not (mask_token is not None and vr.as_bytes(t) == b"")]
  layer = StringLookup(vocabulary=vocab, mask_token=mask_token, num_oov_indices=num_oov)
  assert layer.vocabulary_size() == vr.vocabulary_size(vocab, mask_token, num_oov)
  unknown = ["", "1234567 ", "12345678" * 2, "Amelie (2001)", b"Toy Story", "千と千尋", "c", "unseen %d" % 3,
             b"\xff\x00raw\x00", "Heat", "A", "B", "[UNK]"]
  queries = [q for pair in zip(vocab, unknown) for q in pair]      # 50 % unknown ("" is known or the mask)
  got = layer(queries)
  assert got.dtype == torch.int64 and got.is_cuda
  np.testing.assert_array_equal(_np(got), vr.string_lookup(queries, vocab, mask_token, num_oov))
  grid = np.array(queries[:24], dtype=object).reshape(4, 6)
  np.testing.assert_array_equal(_np(layer(grid)), vr.string_lookup(grid, vocab, mask_token, num_oov))
  ascii_only = np.array(["a", "b", "zz", "Heat (1995)"])              # a NumPy unicode array
  np.testing.assert_array_equal(_np(layer(ascii_only)), vr.string_lookup(ascii_only, vocab, mask_token, num_oov))
  if num_oov == 0:
    with pytest.raises(ValueError, match="ids are not in the vocabulary"):
      layer(queries, validate=True)


def test_string_adapt_and_invert():
  _, StringLookup = _layers()
  batches = [TITLES, TITLES[3:9] + ["[UNK]", "[UNK]", "[UNK]"], [TITLES[5], TITLES[6], "a", b"a"]]
  layer = StringLookup(max_tokens=9)
  layer.adapt(batches)
  want = vr.adapt_order(batches, None, "[UNK]", max_tokens=9, strings=True)
  assert len(want) == 8 and want[:3] == ["千と千尋の神隠し".encode(), b"a", "Amélie (2001)".encode()]   # all seen 3 times
  assert b"\xff\x00raw" in want                               # not UTF-8: handed back with surrogate escapes
  assert [_b(t) for t in layer.get_vocabulary(include_special_tokens=False)] == want
  queries = TITLES + ["unseen", "[UNK]"]
  np.testing.assert_array_equal(_np(layer(queries)), vr.string_lookup(queries, want, None, 1))
  inverse = StringLookup(vocabulary=want, invert=True)
  names = inverse(layer(queries))
  assert isinstance(names, np.ndarray) and names.shape == (len(queries),)
  for q, name in zip(queries, names.tolist()):
    assert _b(name) == (vr.as_bytes(q) if vr.as_bytes(q) in want else b"[UNK]")
  assert inverse(torch.tensor([[0, 1], [-1, 99]])).tolist() == [["[UNK]", "千と千尋の神隠し"], ["[UNK]", "[UNK]"]]


# ---- persistence -----------------------------------------------------------------------------------
def test_state_dict_round_trip(tmp_path):
  IntegerLookup, StringLookup = _layers()
  rng = np.random.default_rng(21)
  vocab = _random_vocabulary(rng, 500, forbidden=(-1, 0))
  ids = torch.as_tensor(_mixed_queries(rng, vocab, 2000, extra=[0, vr.INT64_MIN])).cuda()
  source = torch.nn.Sequential(IntegerLookup(vocabulary=vocab, mask_token=0, num_oov_indices=2))
  state = source.state_dict()
  assert not any(isinstance(v, torch.Tensor) and v.numel() >= 1024 for v in state.values())   # no table image
  torch.save(state, tmp_path / "lookup.pt")
  target = torch.nn.Sequential(IntegerLookup(vocabulary=[1, 2, 3], mask_token=0, num_oov_indices=2))
  target.load_state_dict(torch.load(tmp_path / "lookup.pt"))
  assert target[0].get_vocabulary() == source[0].get_vocabulary()
  assert torch.equal(target(ids), source(ids))
  strings = StringLookup(vocabulary=TITLES, num_oov_indices=2)
  clone = StringLookup(num_oov_indices=2)
  clone.load_state_dict(strings.state_dict())
  queries = TITLES + ["unseen", "other"]
  assert clone.get_vocabulary() == strings.get_vocabulary()
  assert torch.equal(clone(queries), strings(queries))


# ---- graph capture ---------------------------------------------------------------------------------
def test_lookup_inside_a_captured_graph():
  rng = np.random.default_rng(17)
  vocab = _random_vocabulary(rng, 5000)
  layer = _ilookup(vocab, num_oov_indices=3)
  static_ids = torch.as_tensor(_mixed_queries(rng, vocab, 4096)).cuda()
  side = torch.cuda.Stream()                                   # one stream, no parallel branches
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      layer(static_ids)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = layer(static_ids)
  for _ in range(3):
    ids = _mixed_queries(rng, vocab, 4096)
    static_ids.copy_(torch.as_tensor(ids).cuda(), non_blocking=True)
    graph.replay()
    np.testing.assert_array_equal(_np(out), vr.integer_lookup(ids, vocab, None, 3))


# ---- end to end --------------------------------------------------------------------------------------
def test_lookup_in_front_of_an_embedding():
  import recommenders_amd as tfrs
  rng = np.random.default_rng(29)
  vocab = _random_vocabulary(rng, 40)
  assert np.abs(vocab).max() > 1 << 40                          # sparse 64-bit ids
  model = torch.nn.Sequential(tfrs.layers.IntegerLookup(vocabulary=vocab),
                              tfrs.layers.embedding.Embedding(len(vocab) + 1, 8))
  known = rng.choice(vocab, size=12, replace=False)
  ids = rng.permutation(np.concatenate([known, known[:5], [vocab.max() - 1, 12345678901234]]))
  want = vr.integer_lookup(ids, vocab)
  assert 0 in want                                              # the OOV row
  out = model(torch.as_tensor(ids).cuda())
  assert tuple(out.shape) == (ids.size, 8)
  table = model[1].embeddings
  assert torch.equal(out, table.detach()[torch.as_tensor(want).cuda()])
  out.sum().backward()
  rows = torch.nonzero(table.grad.abs().sum(dim=1)).reshape(-1)
  assert _np(rows).tolist() == sorted(set(want.tolist()))
  counts = np.bincount(want, minlength=len(vocab) + 1).astype(np.float32)
  np.testing.assert_array_equal(_np(table.grad), np.repeat(counts[:, None], 8, axis=1))
