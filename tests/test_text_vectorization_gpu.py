"""``TextVectorization`` on the MI355X (``csrc/text.hip``): every comparison of indices, counts, fingerprints and spans
is exact integer equality against the pure-Python restatement of tests/text_restatement.py -- hand-built strings
over every standardize / split mode, tokens at the SipHash word edges, truncation and padding, the launch's and the
LDS window's edges, random batches, ``adapt``, persistence, a captured call, ``StringLookup`` on ``PackedStrings``
and the tutorial's title tower.  The kernel tests run once per byte route of the kernel (LDS window / direct read),
whichever of the two is the default."""

import numpy as np
import pytest
import torch

from tests import text_restatement as tr
from tests import vocab_restatement as vr
from tests.conftest import float_gate

pytestmark = pytest.mark.gpu

BOTH = "lower_and_strip_punctuation"
WORDS = ["w" + chr(97 + i // 26) + chr(97 + i % 26) + "abcdefgh"[:i % 9] for i in range(300)]     # 300 distinct words


def _np(t):
  return t.detach().cpu().numpy()


def _tv(vocabulary=None, **kw):
  import recommenders_amd as tfrs
  return tfrs.layers.TextVectorization(vocabulary=vocabulary, **kw)


def _packed(strings):
  import recommenders_amd as tfrs
  return tfrs.layers.PackedStrings.from_strings(strings, "cuda")


@pytest.fixture(params=["window", "direct"])
def variant(request):
  from recommenders_amd import _lib
  _lib.set_option("TFRS_TEXT_VARIANT", request.param)
  yield request.param
  _lib.set_option("TFRS_TEXT_VARIANT", None)


def _codes(standardize, split):
  from recommenders_amd.layers import preprocessing
  return preprocessing._STANDARDIZE[standardize], preprocessing._SPLIT[split]


def _counts(packed, standardize, split):
  from recommenders_amd import _lib
  st, sp = _codes(standardize, split)
  counts = torch.empty((packed.n,), dtype=torch.int64, device="cuda")
  _lib.check(_lib.load().tfrs_text_count_tokens(_lib.ptr(packed.bytes), packed.bytes.numel(), _lib.ptr(packed.offsets),
                                                packed.n, st, sp, _lib.ptr(counts), _lib.current_stream()))
  return _np(counts)


def _spans(packed, standardize, split):
  """Per string the list of (fingerprint, start, end) the span entry writes."""
  from recommenders_amd import _lib
  st, sp = _codes(standardize, split)
  counts = _counts(packed, standardize, split)
  splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  total = int(splits[-1])
  out = [torch.full((max(total, 1),), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
  d_splits = torch.as_tensor(splits).cuda()
  _lib.check(_lib.load().tfrs_text_token_spans(
      _lib.ptr(packed.bytes), packed.bytes.numel(), _lib.ptr(packed.offsets), packed.n, st, sp, _lib.ptr(d_splits),
      _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.current_stream()))
  f, s, e = (_np(t)[:total].tolist() for t in out)
  return [list(zip(f[a:b], s[a:b], e[a:b])) for a, b in zip(splits[:-1], splits[1:])]


def _check(strings, vocabulary, standardize=BOTH, split="whitespace", seq_lens=(), packed=None, spans=False):
  """The three output routes, the count pass and (optionally) the span entry against the restatement."""
  packed = _packed(strings) if packed is None else packed
  kw = dict(standardize=standardize, split=split)
  values, splits = tr.vectorize(strings, vocabulary, standardize, split, ragged=True)
  lengths = np.diff(splits)
  dense = _tv(vocabulary, **kw)(packed)
  assert dense.dtype == torch.int64 and dense.is_cuda
  want = tr.vectorize(strings, vocabulary, standardize, split)
  assert tuple(dense.shape) == want.shape == (len(strings), int(lengths.max(initial=0)))
  np.testing.assert_array_equal(_np(dense), want)
  ragged = _tv(vocabulary, ragged=True, **kw)(packed)
  assert ragged.values.dtype == torch.int64 and ragged.values.is_cuda
  np.testing.assert_array_equal(_np(ragged.row_splits), splits)
  np.testing.assert_array_equal(_np(ragged.values), values)
  assert not (values == 0).any()
  # consistency: count pass == ragged row lengths == non-zero entries of a dense row that is long enough
  np.testing.assert_array_equal(_counts(packed, standardize, split), lengths)
  np.testing.assert_array_equal((_np(dense) != 0).sum(axis=1), lengths)
  for seq_len in seq_lens:
    got = _tv(vocabulary, output_sequence_length=seq_len, **kw)(packed)
    assert tuple(got.shape) == (len(strings), seq_len)
    np.testing.assert_array_equal(_np(got), tr.vectorize(strings, vocabulary, standardize, split, seq_len=seq_len))
  if spans:
    assert _spans(packed, standardize, split) == tr.token_spans(strings, standardize, split)
  return dense


def _half_vocabulary(strings, modes=tr.MODES, splits=tr.SPLITS):
  """Every second token the strings give under any mode: half of the lookups hit, half miss."""
  seen = set()
  for st in modes:
    for sp in splits:
      for s in strings:
        seen.update(tr.tokens(s, st, sp))
  seen.discard(b"[UNK]")
  return sorted(seen)[::2]


# ---- hand-built strings ----------------------------------------------------------------------------------
HAND = ["", " ", " \t\n\v\f\r", "!?.,", "...", " - ", "a\tb", "a\nb", "a\vb", "a\fb", "a\rb", "a b", "  lead", "trail  ",
        " both ", "a   b \t\n c", "@AZ[", "`az{", "@AZ[ `az{", b"\x7f", b"\x80", b"\xc3\x89", b"\xff",
        b"\x7f \x80 \xc3\x89 \xff", "É é", b"a\x00b", b"\x00", b"\x00 \x00\x00", "It's a-b a - b",
        "[UNK] Toy Story (1995)", "Toy Story", "TOY-STORY"]


@pytest.mark.parametrize("split", tr.SPLITS)
@pytest.mark.parametrize("standardize", tr.MODES)
def test_hand_built_strings(variant, standardize, split):
  vocab = _half_vocabulary(HAND)
  dense = _check(HAND, vocab, standardize, split, seq_lens=(1, 3), spans=True)
  assert _np(dense)[0].tolist() == [0] * dense.shape[1]              # the empty string: padding only
  if standardize == BOTH and split == "whitespace":
    for row in (1, 2, 3, 4, 5):                                          # only whitespace, only punctuation, " - "
      assert not _np(dense)[row].any()
    np.testing.assert_array_equal(_np(dense)[6:12, :2], np.repeat(_np(dense)[11:12, :2], 6, axis=0))   # six separators


# ---- SipHash word edges ----------------------------------------------------------------------------------
def _edge_token(length, upper=False):
  letters = "".join(chr((65 if upper and k % 2 else 97) + (k * 5 + length) % 26) for k in range(length))
  return ".".join(letters)                                  # a deleted byte between any two kept bytes


def test_siphash_word_edges(variant):
  lengths = (1, 7, 8, 9, 15, 16, 17, 24)
  assert _edge_token(9).count(".") == 8 and len(tr.standardize(_edge_token(9), BOTH)) == 9
  tokens = [_edge_token(n) for n in lengths] + [_edge_token(n, upper=True) for n in lengths]
  strings = tokens + [" ".join(tokens), "\t".join(reversed(tokens)), "a.b.c.d.e.f.g.h.i", "!" + tokens[3] + "?"]
  known = [tr.standardize(_edge_token(n), BOTH) for n in lengths[::2]] + [b"abcdefghi"]
  for standardize in tr.MODES:
    vocab = known if standardize == BOTH else _half_vocabulary(strings, (standardize,), ("whitespace",))
    dense = _check(strings, vocab, standardize, "whitespace", seq_lens=(16,), spans=True)
    if standardize == BOTH:
      assert _np(dense)[:8, 0].tolist() == [2, 1, 3, 1, 4, 1, 5, 1] and _np(dense)[-2, 0] == 6
  _check(strings, known, BOTH, None, spans=True)


# ---- truncation and padding ------------------------------------------------------------------------------
@pytest.mark.parametrize("seq_len", [1, 2, 8])
def test_truncation_and_padding(variant, seq_len):
  vocab = ["story", "toy", "unk", "heat"]
  pool = ["Toy", "story!", "[UNK]", "heat,", "unseen", "(toy)", "x", "Story", "HEAT"]
  rows = [" ".join(pool[(k + j) % len(pool)] for j in range(m)) for k, m in
          enumerate((seq_len - 1, seq_len, seq_len + 1, 0, seq_len + 1, seq_len))]
  got = _tv(vocab, output_sequence_length=seq_len)(rows)
  want = tr.vectorize(rows, vocab, seq_len=seq_len)
  np.testing.assert_array_equal(_np(got), want)
  assert (want[0, seq_len - 1:] == 0).all() and (want[3] == 0).all() and (want[1] != 0).all() and (want[2] != 0).all()
  # "[UNK]" in the data standardises to "unk" and is looked up as that; an unseen token gives 1
  probe = _tv(vocab, output_sequence_length=3)(["[UNK] unseen unk"])
  assert _np(probe).tolist() == [[4, 1, 4]]
  plain = _tv(vocab, output_sequence_length=3, standardize=None)(["[UNK] unseen unk"])
  assert _np(plain).tolist() == [[1, 1, 4]]


def test_input_forms():
  vocab = ["story", "toy"]
  layer = _tv(vocab, output_sequence_length=2)
  want = [[3, 2], [1, 0], [0, 0]]
  strings = ["Toy Story", b"Heat", ""]
  for form in (strings, np.array(strings, dtype=object), np.array(strings, dtype=object).reshape(3, 1),
               [[s] for s in strings], _packed(strings), _packed(strings).to("cpu")):
    assert _np(layer(form)).tolist() == want
  assert _np(layer(np.array(["Toy Story", "Heat", ""]))).tolist() == want           # a NumPy unicode array
  assert tuple(layer([]).shape) == (0, 2) and tuple(_tv(vocab)([]).shape) == (0, 0)
  empty = _tv(vocab, ragged=True)(["", " . "])
  assert empty.values.numel() == 0 and empty.row_splits.tolist() == [0, 0, 0]
  assert tuple(_tv(vocab)(["", " . "]).shape) == (2, 0)
  with pytest.raises(ValueError, match=r"\[n\] or \[n, 1\]"):
    layer([["a", "b"], ["c", "d"]])
  with pytest.raises(ValueError, match="string input"):
    layer(torch.zeros(3, dtype=torch.long).cuda())
  with pytest.raises(ValueError, match="reserved OOV"):
    _tv(["a", "[UNK]"])
  assert _tv(["", "[UNK]", "toy"]).get_vocabulary() == ["", "[UNK]", "toy"]     # leading special tokens are dropped
  assert _np(_tv(["Toy"], output_sequence_length=1)(["Toy"])).tolist() == [[1]]  # the vocabulary is NOT standardised


# ---- launch edges ------------------------------------------------------------------------------------------
def _random_strings(rng, n, known, max_tokens=12):
  seps = [" ", "  ", "\t", "\n", " \r\n", "\v", "\f", " - ", ", ", ". "]
  marks = ["", "", "", "!", "'s", "(", ")", "-x", ":"]
  out = []
  for _ in range(n):
    parts = [seps[rng.integers(len(seps))]] if rng.integers(4) == 0 else []
    for _ in range(int(rng.integers(0, max_tokens + 1))):
      word = known[rng.integers(len(known))] if rng.integers(3) else "q%d" % rng.integers(10 ** 6)
      word = "".join(c.upper() if rng.integers(3) == 0 else c for c in word)
      cut = int(rng.integers(0, len(word) + 1))
      word = word[:cut] + marks[rng.integers(len(marks))] + word[cut:] + marks[rng.integers(len(marks))]
      parts += [word, seps[rng.integers(len(seps))]]
    if parts and rng.integers(2):
      parts.pop()
    out.append("".join(parts))
  return out


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_launch_edges(variant, n):
  rng = np.random.default_rng(n)
  _check(_random_strings(rng, n, WORDS, max_tokens=4), WORDS[::2], seq_lens=(3,))


def test_grid_stride_beyond_the_grid_cap(variant):
  import recommenders_amd as tfrs
  from recommenders_amd.layers import preprocessing
  n = preprocessing.TEXT_MAX_BLOCKS * 256 + 1
  pool = [b"a ", b"b.", b"zz", b"  ", b"A,", b"..", b"Zz", b" c", b"d\t"]
  pick = (np.arange(n) * 7 + np.arange(n) // 256) % len(pool)
  blob = np.frombuffer(b"".join(pool), dtype=np.uint8).reshape(len(pool), 2)[pick].reshape(-1)
  packed = tfrs.layers.PackedStrings(torch.from_numpy(blob.copy()).cuda(), (2 * torch.arange(n + 1)).cuda())
  vocab = ["a", "zz", "d"]
  per_kind = tr.vectorize(pool, vocab, seq_len=1)[:, 0]
  assert per_kind.tolist() == [2, 1, 3, 0, 2, 0, 3, 1, 4]
  got = _tv(vocab, output_sequence_length=1)(packed)
  np.testing.assert_array_equal(_np(got)[:, 0], per_kind[pick])
  np.testing.assert_array_equal(_counts(packed, BOTH, "whitespace"), (per_kind != 0).astype(np.int64)[pick])


# ---- window edges --------------------------------------------------------------------------------------------
def _text_of_length(rng, length):
  """Exactly ``length`` bytes of words, punctuation and separators, ending in a letter."""
  parts, size = [], 0
  while size < length:
    word = WORDS[rng.integers(len(WORDS))] + ["", ",", "!"][rng.integers(3)] + [" ", "  ", "\t"][rng.integers(3)]
    parts.append(word)
    size += len(word)
  return ("".join(parts)[:length - 1] + "x") if length else ""


@pytest.fixture(scope="module")
def window_batches():
  from recommenders_amd.layers import preprocessing
  W = preprocessing.TEXT_WINDOW_BYTES
  rng = np.random.default_rng(77)
  text = lambda length: _text_of_length(rng, length)
  batches = {
      # a string ending exactly at a window's end; the next one starts at the following window's first byte
      "ends_at_window_end": [text(100), text(W - 100), text(50), text(W - 50), "Toy story"],
      # a token straddling two windows with the deleted byte on the boundary: last byte of window 0, first of window 1
      "deleted_byte_last": [text(W - 3), "xy.zw tail"],
      "deleted_byte_first": [text(W - 2), "xy.zw tail"],
      "kept_bytes_across": [text(W - 5), "abcdefghij.klm"],
      # one string of three windows' length holding a single token, then short ones
      "one_token_three_windows": ["head", "a" * (3 * W), "Tail end"],
      # 70 000 bytes with many tokens, between short strings
      "long_string": ["short one", text(70_000), "another, short"],
      "empty_strings": [""] * 256,
      "empty_then_text": [""] * 256 + ["after the empty workgroup", ""],
  }
  vocab = WORDS[::2] + ["xyzw", "tail", "toy", "a" * (3 * W), "abcdefghijklm"]
  want = {k: tr.vectorize(v, vocab, seq_len=6) for k, v in batches.items()}
  return W, batches, vocab, want


@pytest.mark.parametrize("case", ["ends_at_window_end", "deleted_byte_last", "deleted_byte_first", "kept_bytes_across",
                                  "one_token_three_windows", "long_string", "empty_strings", "empty_then_text"])
def test_window_edges(variant, window_batches, case):
  W, batches, vocab, want = window_batches
  strings = batches[case]
  packed = _packed(strings)
  offsets = packed.offsets.tolist()
  if case == "ends_at_window_end":
    assert offsets[2] == W and offsets[4] == 2 * W
  if case == "deleted_byte_last":
    assert strings[1][2] == "." and offsets[1] + 2 == W - 1
  if case == "deleted_byte_first":
    assert offsets[1] + 2 == W
  if case in ("empty_strings",):
    assert packed.bytes.numel() == 0
  got = _tv(vocab, output_sequence_length=6)(packed)
  np.testing.assert_array_equal(_np(got), want[case])
  if case == "one_token_three_windows":
    assert want[case].tolist() == [[1, 0, 0, 0, 0, 0], [2 + len(vocab) - 2, 0, 0, 0, 0, 0], [3 + len(WORDS[::2]), 1, 0, 0, 0, 0]]
  ragged = _tv(vocab, ragged=True)(packed)
  values, splits = tr.vectorize(strings, vocab, ragged=True)
  np.testing.assert_array_equal(_np(ragged.row_splits), splits)
  np.testing.assert_array_equal(_np(ragged.values), values)
  if case in ("deleted_byte_last", "deleted_byte_first", "kept_bytes_across", "one_token_three_windows"):
    assert _spans(packed, BOTH, "whitespace") == tr.token_spans(strings, BOTH, "whitespace")


def test_span_that_starts_off_a_16_byte_boundary(variant):
  import recommenders_amd as tfrs
  rng = np.random.default_rng(5)
  strings = _random_strings(rng, 300, WORDS, max_tokens=5)
  whole = _packed(["xyz"] + strings)
  assert whole.bytes.data_ptr() % 16 == 0 and whole.offsets[1].item() == 3
  shifted = tfrs.layers.PackedStrings(whole.bytes[3:], whole.offsets[1:] - 3)
  assert shifted.bytes.data_ptr() % 16 == 3 and shifted.n == 300
  _check(strings, WORDS[::2], seq_lens=(4,), packed=shifted, spans=True)


# ---- random batches ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_batch():
  rng = np.random.default_rng(2025)
  return _random_strings(rng, 2000, WORDS)


@pytest.mark.parametrize("standardize,split", [(m, "whitespace") for m in tr.MODES] + [(BOTH, None), (None, None)])
def test_random_batches(variant, random_batch, standardize, split):
  vocab = WORDS[::2] if split else _half_vocabulary(random_batch[:200], (standardize,), (None,))
  _check(random_batch, vocab, standardize, split, seq_lens=(8,))


# ---- adapt -------------------------------------------------------------------------------------------------------
def test_adapt_one_batch_with_ties():
  data = ["b a", "B c.", "c a d", "[UNK] unk", " - "]
  layer = _tv()
  layer.adapt(data)
  want = tr.adapt_order([data])
  assert want == [b"unk", b"c", b"b", b"a", b"d"]                    # counts 2 2 2 2 1: ties by token bytes descending
  assert [t.encode() for t in layer.get_vocabulary(include_special_tokens=False)] == want
  assert layer.get_vocabulary()[:2] == ["", "[UNK]"] and layer.vocabulary_size() == 7
  np.testing.assert_array_equal(_np(layer(data)), tr.vectorize(data, want))
  plain = _tv(standardize=None)
  plain.adapt(data)                                                 # "[UNK]" survives and is not counted
  assert [t.encode() for t in plain.get_vocabulary(include_special_tokens=False)] == tr.adapt_order(
      [data], None, "whitespace") == [b"a", b"unk", b"d", b"c.", b"c", b"b", b"B", b"-"]
  layer.adapt(["z z y"])                                            # adapt starts afresh
  assert layer.get_vocabulary() == ["", "[UNK]", "z", "y"]


@pytest.mark.parametrize("max_tokens", [None, 40, 3, 2])
def test_adapt_several_batches(variant, random_batch, max_tokens):
  batches = [random_batch[:700], np.array(random_batch[700:1500], dtype=object), _packed(random_batch[1500:])]
  layer = _tv(max_tokens=max_tokens)
  layer.adapt(batches)
  want = tr.adapt_order([random_batch], max_tokens=max_tokens)
  got = layer.get_vocabulary()
  assert got[:2] == ["", "[UNK]"] and [t.encode() for t in got[2:]] == want
  if max_tokens is not None:
    assert layer.vocabulary_size() == max_tokens
  np.testing.assert_array_equal(_np(layer(random_batch[:300])), tr.vectorize(random_batch[:300], want))


def test_adapt_max_tokens_cuts_inside_a_tie():
  data = [["one two three four", "eight eight eight"], ["one two three four"]]
  layer = _tv(max_tokens=5, split="whitespace")
  layer.adapt(data)
  assert layer.get_vocabulary() == ["", "[UNK]", "eight", "two", "three"]
  assert tr.adapt_order(data, max_tokens=5) == [b"eight", b"two", b"three"]
  whole = _tv(split=None)
  whole.adapt(data)
  assert whole.get_vocabulary(include_special_tokens=False) == ["one two three four", "eight eight eight"]


# ---- persistence ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trip(random_batch):
  source = torch.nn.Sequential(_tv(WORDS[::3], output_sequence_length=6))
  state = source.state_dict()
  assert state and not any(isinstance(v, torch.Tensor) for v in state.values())      # the vocabulary, no table image
  target = torch.nn.Sequential(_tv(["other"], output_sequence_length=6))
  target.load_state_dict(state)
  assert target[0].get_vocabulary() == source[0].get_vocabulary() == ["", "[UNK]"] + WORDS[::3]
  assert torch.equal(target(random_batch[:500]), source(random_batch[:500]))


# ---- graph capture -------------------------------------------------------------------------------------------------
def test_call_inside_a_captured_graph(random_batch):
  import recommenders_amd as tfrs
  vocab = WORDS[::2]
  first = random_batch[:1024]
  rng = np.random.default_rng(9)
  second = [s.swapcase() for s in (first[i] for i in rng.permutation(len(first)))]      # the same byte and string counts
  layer = _tv(vocab, output_sequence_length=8)
  host = _packed(first)
  static = tfrs.layers.PackedStrings(host.bytes.clone(), host.offsets.clone(), validate=False)
  side = torch.cuda.Stream()                                   # one stream, no parallel branches
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      layer(static)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = layer(static)
  graph.replay()
  np.testing.assert_array_equal(_np(out), tr.vectorize(first, vocab, seq_len=8))
  other = _packed(second)
  assert other.bytes.numel() == static.bytes.numel() and other.n == static.n
  static.bytes.copy_(other.bytes, non_blocking=True)
  static.offsets.copy_(other.offsets, non_blocking=True)
  graph.replay()
  want = tr.vectorize(second, vocab, seq_len=8)
  assert (want != tr.vectorize(first, vocab, seq_len=8)).any()
  np.testing.assert_array_equal(_np(out), want)


# ---- StringLookup on PackedStrings ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_token", [None, ""])
def test_string_lookup_on_packed_strings(mask_token):
  import recommenders_amd as tfrs
  titles = ["Toy Story (1995)", "Heat (1995)", "Amélie (2001)", b"\xff\x00raw", "a"]
  layer = tfrs.layers.StringLookup(vocabulary=titles, mask_token=mask_token, num_oov_indices=2)
  queries = titles + ["", "unseen", "toy story (1995)", "a ", "Heat (1995)"]
  want = layer(queries)
  got = layer(_packed(queries))
  assert got.dtype == torch.int64 and tuple(got.shape) == (len(queries),) and torch.equal(got, want)
  np.testing.assert_array_equal(_np(got), vr.string_lookup(queries, titles, mask_token, 2))
  assert torch.equal(layer(_packed(queries).to("cpu")), want)
  assert torch.equal(layer(_packed(["", ""])), layer(["", ""]))           # an empty blob


# ---- the tutorial's tower ------------------------------------------------------------------------------------------
def test_title_tower_mean_of_token_embeddings():
  """TextVectorization(ragged=True) -> embedding_lookup_sparse(combiner="mean") against a float64 mean of the restated
  ids' rows.  Yardstick sum |terms| / count; limit 8 * 2^-23: an f32 sum of at most 8 terms (7 additions, each within
  2^-24 of the partial sum, itself at most the sum of |terms|) and one division (2^-24) stay below 8 * 2^-24 of the
  yardstick, and the bound leaves a factor two -- derived, not measured.  A row without tokens is compared with what
  embedding_lookup_sparse gives for an empty row today."""
  from recommenders_amd.layers import embedding as emb
  rng = np.random.default_rng(31)
  vocab = WORDS[:62]                                             # indices 2 .. 63 of a 64 x 32 table
  table = rng.uniform(-0.05, 0.05, size=(64, 32)).astype(np.float32)
  strings = []
  for r in range(96):
    m = r % 9                                                     # 0 .. 8 tokens
    words = [WORDS[rng.integers(70)] for _ in range(m)]           # some beyond the vocabulary: the [UNK] row
    strings.append(", ".join(w.capitalize() for w in words))
  ids = _tv(vocab, ragged=True)(strings)
  values, splits = tr.vectorize(strings, vocab, ragged=True)
  np.testing.assert_array_equal(_np(ids.values), values)
  assert set(np.diff(splits).tolist()) == set(range(9)) and 1 in values and values.max() <= 63
  table_t = torch.as_tensor(table).cuda()
  got = emb.embedding_lookup_sparse(table_t, ids.values, ids.row_splits.cuda(), combiner="mean")
  assert tuple(got.shape) == (96, 32)
  today = emb.embedding_lookup_sparse(table_t, torch.tensor([5, 6]).cuda(), torch.tensor([0, 0, 2, 2]).cuda(),
                                      combiner="mean")
  empty_row = _np(today)[0].astype(np.float64)
  assert np.array_equal(_np(today)[0], _np(today)[2])
  ref = np.empty((96, 32), dtype=np.float64)
  yard = np.zeros((96, 32), dtype=np.float64)
  for r, (a, b) in enumerate(zip(splits[:-1], splits[1:])):
    if a == b:
      ref[r] = empty_row
    else:
      rows = table[values[a:b]].astype(np.float64)
      ref[r] = rows.mean(axis=0)
      yard[r] = np.abs(rows).sum(axis=0) / (b - a)
  float_gate("text_vectorization.title_tower_mean", _np(got), ref, yard, 8 * 2.0 ** -23)
