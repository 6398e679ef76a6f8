"""``TextVectorization`` and ``PackedStrings`` without a GPU: the restatement against hand-written token lists, the
export and the constructor's errors, ``PackedStrings`` on CPU tensors, the no-GPU behaviour and the argument checks
of the three C entries of ``csrc/text.hip``."""

import os
import re
import string

import numpy as np
import pytest
import torch

from tests import text_restatement as tr
from tests import vocab_restatement as vr

BOTH = "lower_and_strip_punctuation"


@pytest.fixture(scope="module")
def lib():
  import __graft_entry__
  __graft_entry__.build()
  from recommenders_amd import _lib
  return _lib.load()


def _layer():
  import recommenders_amd as tfrs
  return tfrs.layers.TextVectorization


# ---- the restatement against hand-written expectations ---------------------------------------------------
def test_punctuation_and_whitespace_sets():
  from recommenders_amd.layers import preprocessing
  assert tr.PUNCTUATION == string.punctuation.encode() == preprocessing.PUNCTUATION
  assert len(set(tr.PUNCTUATION)) == 32 and all(c < 0x80 for c in tr.PUNCTUATION)
  assert sorted(tr.WHITESPACE) == sorted(preprocessing.WHITESPACE) == [9, 10, 11, 12, 13, 32]
  assert set(preprocessing._STANDARDIZE) == set(tr.MODES) and set(preprocessing._SPLIT) == set(tr.SPLITS)


def test_restated_standardize():
  assert tr.standardize("It's", BOTH) == b"its"
  assert tr.standardize("a-b", BOTH) == b"ab" and tr.standardize("a - b", BOTH) == b"a  b"
  assert tr.standardize("@AZ[`az{", "lower") == b"@az[`az{"
  assert tr.standardize("@AZ[`az{", "strip_punctuation") == b"AZaz"
  assert tr.standardize("@AZ[`az{", BOTH) == b"azaz"
  assert tr.standardize("@AZ[`az{", None) == b"@AZ[`az{"
  assert tr.standardize(b"\x7f\x80\xc3\x89\xff\x00", BOTH) == b"\x7f\x80\xc3\x89\xff\x00"     # É is not lowered
  assert tr.standardize("É".encode(), "lower") == "É".encode()
  assert tr.standardize(string.punctuation, "strip_punctuation") == b""
  every = bytes(range(256))
  kept = tr.standardize(every, BOTH)
  assert len(kept) == 256 - 32 and b"A" not in kept and kept.count(b"a") == 2


def test_restatement_agrees_with_the_layers_host_rule():
  from recommenders_amd.layers import preprocessing
  every = bytes(range(256)) + b"It's a-b [UNK]"
  for mode in tr.MODES:
    assert preprocessing._standardize(every, mode) == tr.standardize(every, mode)


@pytest.mark.parametrize("text,want", [
    ("", []), (" \t\n\v\f\r", []), ("!?.,", []), (" - ", []),
    ("a - b", [b"a", b"b"]), ("a-b", [b"ab"]), ("it's", [b"its"]),
    ("a\tb\nc\vd\fe\rf g", [b"a", b"b", b"c", b"d", b"e", b"f", b"g"]),
    ("  lead", [b"lead"]), ("trail  ", [b"trail"]), ("a   b \t\n c", [b"a", b"b", b"c"]),
    ("@AZ[ `az{", [b"az", b"az"]), (b"\x7f \x80 \xc3\x89 \xff", [b"\x7f", b"\x80", b"\xc3\x89", b"\xff"]),
    (b"a\x00b c", [b"a\x00b", b"c"]), ("[UNK] Toy Story (1995)", [b"unk", b"toy", b"story", b"1995"]),
    ("a.b.c.d.e.f.g.h.i", [b"abcdefghi"]),
])
def test_restated_tokens(text, want):
  assert tr.tokens(text, BOTH, "whitespace") == want
  whole = tr.standardize(text, BOTH)
  assert tr.tokens(text, BOTH, None) == ([whole] if whole else [])
  assert tr.split(tr.standardize(text, BOTH), "whitespace") == want      # standardise then split: the same tokens


def test_restated_modes_and_splits():
  text = "The  Matrix: Re-loaded!"
  assert tr.tokens(text, None, "whitespace") == [b"The", b"Matrix:", b"Re-loaded!"]
  assert tr.tokens(text, "lower", "whitespace") == [b"the", b"matrix:", b"re-loaded!"]
  assert tr.tokens(text, "strip_punctuation", "whitespace") == [b"The", b"Matrix", b"Reloaded"]
  assert tr.tokens(text, BOTH, None) == [b"the  matrix reloaded"]
  assert tr.tokens("   ", None, None) == [b"   "] and tr.tokens("...", BOTH, None) == []
  assert tr.split(b" a  b ", "whitespace") == [b"a", b"b"] and tr.split(b"", None) == []


def test_restated_vectorize_and_spans():
  vocab = ["story", "toy", "the"]
  strings = ["Toy Story", "", "the THE the heat", " - ", "[UNK]"]
  np.testing.assert_array_equal(tr.vectorize(strings, vocab), [[3, 2, 0, 0], [0, 0, 0, 0], [4, 4, 4, 1], [0, 0, 0, 0],
                                                               [1, 0, 0, 0]])
  np.testing.assert_array_equal(tr.vectorize(strings, vocab, seq_len=2), [[3, 2], [0, 0], [4, 4], [0, 0], [1, 0]])
  values, splits = tr.vectorize(strings, vocab, ragged=True)
  assert values.tolist() == [3, 2, 4, 4, 4, 1, 1] and splits.tolist() == [0, 2, 2, 6, 6, 7]
  assert tr.vectorize(strings, vocab, None, "whitespace", seq_len=1).tolist() == [[1], [0], [4], [1], [1]]
  spans = tr.token_spans(["a, b", "", "(c)"], BOTH, "whitespace")
  assert [[(a, b) for _, a, b in row] for row in spans] == [[(0, 2), (3, 4)], [], [(4, 7)]]     # raw runs: "a," and "(c)"
  assert spans[0][0][0] == vr.as_signed(vr.fingerprint(b"a")) and spans[2][0][0] == vr.as_signed(vr.fingerprint(b"c"))
  assert [(a, b) for _, a, b in tr.token_spans([" x y "], BOTH, None)[0]] == [(0, 5)]


def test_restated_adapt_order():
  batches = [["b a", "B c."], ["c a d", "[UNK] unk"]]
  assert tr.adapt_order(batches) == [b"unk", b"c", b"b", b"a", b"d"]          # counts 2 2 2 2 1, ties by bytes descending
  assert tr.adapt_order(batches, max_tokens=5) == [b"unk", b"c", b"b"]
  assert tr.adapt_order(batches, None, "whitespace") == [b"a", b"unk", b"d", b"c.", b"c", b"b", b"B"]   # "[UNK]" is not counted


# ---- export and constructor ------------------------------------------------------------------------------------
def test_layer_is_exported():
  import recommenders_amd as tfrs
  from recommenders_amd.layers import hashing, preprocessing
  assert tfrs.layers.TextVectorization is preprocessing.TextVectorization
  assert tfrs.layers.PackedStrings is hashing.PackedStrings is preprocessing.PackedStrings
  for name in ("adapt", "set_vocabulary", "get_vocabulary", "vocabulary_size", "state_dict", "load_state_dict"):
    assert callable(getattr(tfrs.layers.TextVectorization, name))
  assert callable(preprocessing._standardize)


def test_exported_constants_match_the_header():
  from recommenders_amd.layers import preprocessing
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  header = open(os.path.join(root, "include", "tfrs_hip.h")).read()
  define = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
  assert preprocessing.TEXT_WINDOW_BYTES == define("TFRS_TEXT_WINDOW_BYTES") == 16384
  assert preprocessing.TEXT_MAX_BLOCKS == define("TFRS_TEXT_MAX_BLOCKS")
  assert preprocessing._STANDARDIZE["lower"] == define("TFRS_TEXT_LOWER")
  assert preprocessing._STANDARDIZE["strip_punctuation"] == define("TFRS_TEXT_STRIP_PUNCTUATION")
  assert preprocessing._STANDARDIZE[BOTH] == define("TFRS_TEXT_LOWER") | define("TFRS_TEXT_STRIP_PUNCTUATION")
  assert preprocessing._SPLIT["whitespace"] == define("TFRS_TEXT_SPLIT_WHITESPACE")
  assert preprocessing._SPLIT[None] == define("TFRS_TEXT_SPLIT_NONE")


def test_constructor_errors():
  TextVectorization = _layer()
  for kw in (dict(split="character"), dict(split=str.split), dict(standardize=str.lower), dict(ngrams=2),
             dict(ngrams=(1, 2)), dict(output_mode="multi_hot"), dict(output_mode="count"),
             dict(output_mode="tf_idf")):
    with pytest.raises(NotImplementedError):
      TextVectorization(**kw)
  with pytest.raises(ValueError, match="exclude"):
    TextVectorization(ragged=True, output_sequence_length=4)
  with pytest.raises(ValueError, match="output_sequence_length"):
    TextVectorization(output_sequence_length=0)
  with pytest.raises(ValueError, match="standardize"):
    TextVectorization(standardize="upper")
  with pytest.raises(ValueError, match="split"):
    TextVectorization(split="words")
  for mode in tr.MODES:
    for split in tr.SPLITS:
      layer = TextVectorization(standardize=mode, split=split, max_tokens=10, output_sequence_length=3)
      assert layer.max_tokens == 10 and layer.vocabulary_size() == 2
      assert layer.get_vocabulary() == ["", "[UNK]"] and layer.get_vocabulary(include_special_tokens=False) == []


# ---- PackedStrings -------------------------------------------------------------------------------------------
def test_packed_strings_round_trip_on_cpu():
  from recommenders_amd.layers import PackedStrings
  strings = ["Toy Story (1995)", "", b"\xff\x00raw", "Amélie", "", "x"]
  packed = PackedStrings.from_strings(strings, "cpu")
  assert packed.n == len(packed) == 6 and packed.bytes.dtype == torch.uint8 and packed.offsets.dtype == torch.int64
  assert packed.offsets.tolist() == [0, 16, 16, 21, 28, 28, 29] and packed.bytes.numel() == 29
  assert packed.tolist() == [vr.as_bytes(s) for s in strings]
  again = PackedStrings(packed.bytes, packed.offsets)                     # validates
  assert again.tolist() == packed.tolist() and again.to("cpu") is again
  grid = PackedStrings.from_strings(np.array([["a"], ["bc"]], dtype=object), "cpu")
  assert grid.tolist() == [b"a", b"bc"]
  empty = PackedStrings.from_strings(["", ""], "cpu")
  assert empty.bytes.numel() == 0 and empty.offsets.tolist() == [0, 0, 0]
  assert PackedStrings(empty.bytes, empty.offsets).n == 2
  none = PackedStrings.from_strings([], "cpu")
  assert none.n == 0 and none.tolist() == []


def test_packed_strings_validation_errors():
  from recommenders_amd.layers import PackedStrings
  blob = torch.arange(10, dtype=torch.uint8)
  off = lambda *xs: torch.tensor(xs, dtype=torch.int64)
  with pytest.raises(ValueError, match=r"offsets\[0\]"):
    PackedStrings(blob, off(1, 4, 10))
  with pytest.raises(ValueError, match="decrease"):
    PackedStrings(blob, off(0, 6, 4, 10))
  with pytest.raises(ValueError, match=r"offsets\[-1\]"):
    PackedStrings(blob, off(0, 4, 9))
  with pytest.raises(ValueError, match=r"offsets\[-1\]"):
    PackedStrings(blob, off(0, 4, 11))
  with pytest.raises(ValueError, match="uint8"):
    PackedStrings(blob.to(torch.int32), off(0, 10))
  with pytest.raises(ValueError, match="int64"):
    PackedStrings(blob, off(0, 10).to(torch.int32))
  with pytest.raises(ValueError, match="int64"):
    PackedStrings(blob, torch.zeros((0,), dtype=torch.int64))
  with pytest.raises(ValueError, match="tensors"):
    PackedStrings(b"abc", [0, 3])
  unchecked = PackedStrings(blob, off(0, 6, 4, 10), validate=False)      # the caller's word is taken
  assert unchecked.n == 3


# ---- no GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_layer_fails_loudly_without_gpu():
  import recommenders_amd as tfrs
  TextVectorization = _layer()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    TextVectorization(vocabulary=["toy", "story"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    TextVectorization()(["Toy Story"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    TextVectorization(output_sequence_length=4)(tfrs.layers.PackedStrings.from_strings(["a b"], "cpu"))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    TextVectorization().adapt(["a b", "b c"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    tfrs.layers.PackedStrings.from_strings(["a"])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    tfrs.layers.StringLookup()(tfrs.layers.PackedStrings.from_strings(["a"], "cpu"))


def test_input_errors_come_before_any_launch():
  TextVectorization = _layer()
  layer = TextVectorization(output_sequence_length=4)
  layer._lookup._table = torch.zeros((2, 2), dtype=torch.int64)            # a stand-in: the checks below never reach it
  with pytest.raises(ValueError, match="string input"):
    layer(torch.zeros(3, dtype=torch.long))
  with pytest.raises(ValueError, match="string input"):
    layer(np.zeros(3))
  with pytest.raises(ValueError, match="string input"):
    layer(["a", 3])
  for bad in ([["a", "b"], ["c", "d"]], np.array([[["a"]]], dtype=object), "one string"):
    with pytest.raises(ValueError, match=r"\[n\] or \[n, 1\]"):
      layer(bad)


# ---- the C entries' argument checks (before any HIP call) ---------------------------------------------------------
def test_c_entries_reject_bad_arguments(lib):
  from recommenders_amd import _lib
  E = _lib.TFRS_EINVAL
  buf = np.zeros(64, dtype=np.int64)     # host memory: never dereferenced, the checks come first
  p = buf.ctypes.data + (-buf.ctypes.data) % 16
  count = lambda b, nb, off, n, st, sp, out: lib.tfrs_text_count_tokens(b, nb, off, n, st, sp, out, None)
  assert count(None, 4, None, 4, 3, 1, None) == E and "NULL" in _lib.last_error()
  assert count(None, 4, p, 4, 3, 1, p) == E and "NULL" in _lib.last_error()       # bytes may be NULL only when empty
  assert count(p, 4, None, 4, 3, 1, p) == E and count(p, 4, p, 4, 3, 1, None) == E
  assert count(p, 4, p, -1, 3, 1, p) == E and "bad count" in _lib.last_error()
  assert count(p, -4, p, 4, 3, 1, p) == E and "bad count" in _lib.last_error()
  assert count(p, 4, p, 4, 4, 1, p) == E and "standardize" in _lib.last_error()
  assert count(p, 4, p, 4, -1, 1, p) == E and count(p, 4, p, 4, 3, 2, p) == E
  vec = lambda b, off, n, table, cap, n_tokens, empty, splits, seq_len, out: lib.tfrs_text_vectorize(
      b, 4, off, n, 3, 1, table, cap, n_tokens, empty, splits, seq_len, out, None)
  assert vec(None, None, 4, None, 8, 4, -1, None, 8, None) == E
  assert vec(p, p, 4, None, 8, 4, -1, None, 8, p) == E and "table" in _lib.last_error()
  assert vec(p, p, 4, p + 8, 8, 4, -1, None, 8, p) == E and "16-byte" in _lib.last_error()
  assert vec(p, p, 4, p, 8, 4, -1, None, 8, None) == E and "NULL" in _lib.last_error()
  assert vec(p, None, 4, p, 8, 4, -1, None, 8, p) == E and "NULL" in _lib.last_error()
  assert vec(p, p, 4, p, 24, 3, -1, None, 8, p) == E and "power of two" in _lib.last_error()
  assert vec(p, p, 4, p, 8, 5, -1, None, 8, p) == E and "power of two" in _lib.last_error()
  assert vec(p, p, 4, p, 0, 0, -1, None, 8, p) == E
  assert vec(p, p, 4, p, 8, 4, 4, None, 8, p) == E and "index layout" in _lib.last_error()
  assert vec(p, p, 4, p, 8, 4, -2, None, 8, p) == E
  assert vec(p, p, 4, p, 8, 4, -1, None, 0, p) == E and "seq_len" in _lib.last_error()
  assert vec(p, p, 4, p, 8, 4, -1, None, -3, p) == E and "seq_len" in _lib.last_error()
  assert vec(p, p, -1, p, 8, 4, -1, None, 8, p) == E and "bad count" in _lib.last_error()
  spans = lambda b, off, n, splits, f, s, e: lib.tfrs_text_token_spans(b, 4, off, n, 3, 1, splits, f, s, e, None)
  assert spans(None, None, 4, None, None, None, None) == E and "NULL" in _lib.last_error()
  for hole in range(6):
    args = [p, p, 4, p, p, p, p]
    args[hole if hole < 2 else hole + 1] = None
    assert spans(*args) == E and "NULL" in _lib.last_error()
  assert spans(p, p, -1, p, p, p, p) == E and "bad count" in _lib.last_error()
  with pytest.raises(ValueError, match="text_vectorize"):
    _lib.check(vec(p, p, 4, p, 24, 3, -1, None, 8, p))
