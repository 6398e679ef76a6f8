"""Pure Python / NumPy restatement of ``TextVectorization`` (no test functions; imported by
``test_text_vectorization_host.py`` and ``test_text_vectorization_gpu.py``).

The rules are those of the layer's contract, on bytes, ASCII only: ``lower`` maps ``A-Z`` to
``a-z``; ``strip_punctuation`` deletes the 32 bytes of ``string.punctuation``; bytes ``0x80-0xFF`` pass unchanged.
``split="whitespace"`` cuts at space, ``\\t``, ``\\n``, ``\\v``, ``\\f`` and ``\\r``: tokens are maximal runs of other
bytes, and a run whose bytes were all deleted is no token; ``split=None`` makes the standardised string one token,
none when it is empty.  Index 0 pads, index 1 is the unknown token, the vocabulary follows from 2.  The vocabulary is
a plain ``dict`` from token bytes to index: nothing here hashes.  The fingerprint of a token (for the span entry) is
``vocab_restatement.fingerprint``.
"""

import collections
import string

import numpy as np

from tests import vocab_restatement as vr

PUNCTUATION = string.punctuation.encode("ascii")
WHITESPACE = b" \t\n\x0b\x0c\r"
MODES = (None, "lower", "strip_punctuation", "lower_and_strip_punctuation")
SPLITS = (None, "whitespace")


def as_bytes(x):
  return vr.as_bytes(x)


def standardize(text, mode):
  out = bytearray()
  for c in as_bytes(text):
    if mode in ("strip_punctuation", "lower_and_strip_punctuation") and c in PUNCTUATION:
      continue
    if mode in ("lower", "lower_and_strip_punctuation") and ord("A") <= c <= ord("Z"):
      c += 32
    out.append(c)
  return bytes(out)


def raw_runs(text, mode):
  """The spans [start, end) of the raw pieces a split cuts ``text`` into, before standardisation: the maximal
  runs of bytes that are no whitespace, or the whole string without a split."""
  text = as_bytes(text)
  if mode is None:
    return [(0, len(text))]
  runs, start = [], None
  for p, c in enumerate(text):
    if c in WHITESPACE:
      if start is not None:
        runs.append((start, p))
      start = None
    elif start is None:
      start = p
  if start is not None:
    runs.append((start, len(text)))
  return runs


def split(text, mode):
  """The pieces of ``text`` (already standardised or not) under the split: empty pieces do not exist."""
  text = as_bytes(text)
  return [text[a:b] for a, b in raw_runs(text, mode) if b > a]


def tokens(text, standardize_mode, split_mode):
  """Standardise, split, and drop what standardisation emptied.  Deleting a byte never joins two runs (only
  punctuation is deleted, whitespace stays), so standardising each raw run equals splitting the standardised
  string."""
  text = as_bytes(text)
  pieces = [standardize(text[a:b], standardize_mode) for a, b in raw_runs(text, split_mode)]
  return [p for p in pieces if p]


def token_spans(strings, standardize_mode, split_mode):
  """Per string the list of (fingerprint as signed int64, start, end): the span is the token's RAW run, counted
  from the start of the packed blob (the strings concatenated in order)."""
  rows, base = [], 0
  for s in strings:
    s = as_bytes(s)
    row = []
    for a, b in raw_runs(s, split_mode):
      token = standardize(s[a:b], standardize_mode)
      if token:
        row.append((vr.as_signed(vr.fingerprint(token)), base + a, base + b))
    rows.append(row)
    base += len(s)
  return rows


def index_of(vocabulary):
  """token bytes -> index, for a vocabulary without its two special entries."""
  return {as_bytes(t): 2 + i for i, t in enumerate(vocabulary)}


def vectorize(strings, vocabulary, standardize_mode="lower_and_strip_punctuation", split_mode="whitespace",
              seq_len=None, ragged=False):
  """Dense int64 [n, seq_len] (seq_len None: the longest row), or (values, row_splits) when ``ragged``."""
  index = index_of(vocabulary)
  rows = [[index.get(t, 1) for t in tokens(s, standardize_mode, split_mode)] for s in strings]
  if ragged:
    splits = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=splits[1:])
    return np.array([i for r in rows for i in r], dtype=np.int64), splits
  if seq_len is None:
    seq_len = max([len(r) for r in rows], default=0)
  out = np.zeros((len(rows), seq_len), dtype=np.int64)
  for j, r in enumerate(rows):
    out[j, :min(len(r), seq_len)] = r[:seq_len]
  return out


def adapt_order(batches, standardize_mode="lower_and_strip_punctuation", split_mode="whitespace", max_tokens=None):
  """The vocabulary ``adapt`` builds (without the special entries): count descending, ties by token bytes
  descending, cut to ``max_tokens - 2``; a token spelled like the unknown token is not counted."""
  counts = collections.Counter()
  for batch in batches:
    for s in batch:
      counts.update(tokens(s, standardize_mode, split_mode))
  counts.pop(b"[UNK]", None)
  order = sorted(sorted(counts, reverse=True), key=lambda t: -counts[t])
  return order if max_tokens is None else order[:max(max_tokens - 2, 0)]
