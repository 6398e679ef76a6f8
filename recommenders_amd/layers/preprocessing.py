"""Vocabulary layers: ``IntegerLookup`` and ``StringLookup`` on a device-resident hash table, and
``TextVectorization`` (at the end of this file), which standardises, splits and looks up text in one kernel.

The reference's tutorials put ``tf.keras.layers.StringLookup(vocabulary=..., mask_token=None)`` or
``tf.keras.layers.IntegerLookup(vocabulary=..., mask_value=None)`` in front of every ``Embedding``.  Keras is
not part of the reference tree, so the rules below are the contract of these layers.

Index layout: index 0 is the mask token when ``mask_token`` is not ``None``; the ``num_oov_indices`` OOV slots
come next; the vocabulary follows in order.  An unknown integer ``x`` maps to OOV slot
``floormod(x, num_oov_indices)``, an unknown string to ``fingerprint mod num_oov_indices`` (unsigned).  With
``num_oov_indices=0`` an unknown id maps to ``-1`` and the call stays asynchronous; ``forward(...,
validate=True)`` reads a device counter afterwards and raises ``ValueError`` (Keras always raises; this layer
does not pay a host synchronisation on the hot path).

The table (``csrc/vocab.hip``) is open addressing with linear probing over 16-byte ``{key, value}`` slots,
built on the device with a 64-bit compare-and-swap per token (which also finds repeated keys) and probed by
one lane per id.  A lookup launches one kernel, allocates nothing but its output and never synchronises, so
it can sit inside a captured step.

``StringLookup`` is the same integer table over 64-bit SipHash-2-4 fingerprints of the UTF-8 bytes
(``tfrs_fingerprint_bytes``).  Two vocabulary strings with equal fingerprints raise ``ValueError`` in
``set_vocabulary``; an unknown string whose fingerprint equals a token's is taken for that token (chance
2^-64 per pair).  Keras's own FarmHash is out of scope, as it is for ``Hashing``.

The vocabulary is the persistent state (``state_dict()`` / ``load_state_dict()``); the table is rebuilt on
load, never stored.
"""

import collections
from typing import List, Optional

import numpy as np
import torch

from recommenders_amd import _lib
from recommenders_amd.layers.hashing import PackedStrings, _device, pack_strings
from recommenders_amd.layers.tpu_embedding_layer import RaggedIds, SparseIds

EMPTY_KEY = -(1 << 63)        # TFRS_VOCAB_EMPTY_KEY: marks a free slot, never stored in the table
_DUPLICATE_KEY, _TABLE_FULL = 1, 2


def table_capacity(n: int) -> int:
  """Slots of the table of ``n`` tokens: the power of two >= 2 n (at least 2)."""
  cap = 2
  while cap < 2 * n:
    cap *= 2
  return cap


def _as_bytes(x) -> bytes:
  """UTF-8 bytes of a token; surrogate escapes (``get_vocabulary`` of a token that is not UTF-8) go back to bytes."""
  return bytes(x) if isinstance(x, (bytes, np.bytes_)) else str(x).encode("utf-8", "surrogateescape")


def _string_array(x) -> np.ndarray:
  """Lists become object arrays: NumPy's own conversion would decode ``bytes`` next to ``str`` as ASCII."""
  return x if isinstance(x, np.ndarray) else np.array(x, dtype=object)


def _is_batch(x) -> bool:
  return isinstance(x, (torch.Tensor, np.ndarray, RaggedIds, SparseIds))


def _batches(data):
  """``adapt``'s argument as a sequence of batches: one tensor / array / flat list is one batch."""
  if _is_batch(data) or isinstance(data, (str, bytes)):
    return [data]
  if isinstance(data, (list, tuple)):
    return list(data) if any(_is_batch(x) or isinstance(x, (list, tuple)) for x in data) else [data]
  return data   # any other iterable yields batches


def _values_of(batch):
  return batch.values if isinstance(batch, (RaggedIds, SparseIds)) else batch


class _IndexLookup(torch.nn.Module):
  """What both layers share: the index layout, the table and the lookup launch over int64 keys."""

  _oov_unsigned = 0

  def __init__(self, max_tokens, num_oov_indices, mask_token, oov_token, invert, output_mode, device, mask_value):
    super().__init__()
    if mask_value is not None:
      if mask_token is not None and mask_token != mask_value:
        raise ValueError("`mask_value` is an alias of `mask_token`; pass one of them")
      mask_token = mask_value
    if output_mode != "int":
      raise NotImplementedError(f"output_mode={output_mode!r}: only 'int' is on the hot path")
    if int(num_oov_indices) < 0:
      raise ValueError(f"`num_oov_indices` must be >= 0; got {num_oov_indices}")
    if max_tokens is not None and int(max_tokens) <= 1:
      raise ValueError(f"`max_tokens` must be greater than 1; got {max_tokens}")
    self.max_tokens = None if max_tokens is None else int(max_tokens)
    self.num_oov_indices = int(num_oov_indices)
    self.mask_token = mask_token
    self.oov_token = oov_token
    self.invert = bool(invert)
    self.output_mode = output_mode
    self._device = device
    self._table = None         # [capacity, 2] int64 on the GPU
    self._n_tokens = 0
    self._empty_value = -1     # vocabulary position of the token whose key is EMPTY_KEY, if any
    self._mask_key = 0
    self._unknown = None       # device counter of validate=True
    if mask_token is not None and mask_token == oov_token:
      raise ValueError(f"`mask_token` and `oov_token` must differ; both are {mask_token!r}")

  # ---- index layout ----------------------------------------------------------------------------
  @property
  def _has_mask(self) -> int:
    return 0 if self.mask_token is None else 1

  @property
  def _base(self) -> int:
    return self._has_mask + self.num_oov_indices

  def _special_tokens(self) -> list:
    return [self.mask_token] * self._has_mask + [self.oov_token] * self.num_oov_indices

  def vocabulary_size(self) -> int:
    return self._base + self._n_tokens

  def _check_size(self, n_tokens: int) -> None:
    if self.max_tokens is not None and self._base + n_tokens > self.max_tokens:
      raise ValueError(f"the vocabulary has {self._base + n_tokens} entries with its {self._base} special "
                       f"tokens, more than max_tokens={self.max_tokens}")

  # ---- table -----------------------------------------------------------------------------------
  def _build_table(self, keys: torch.Tensor) -> None:
    """keys[n] int64 on the GPU -> the table; repeated keys raise ValueError."""
    n = keys.numel()
    cap = table_capacity(n)
    table = torch.empty((cap, 2), dtype=torch.int64, device=keys.device)
    flags = torch.empty((1,), dtype=torch.int32, device=keys.device)
    _lib.check(_lib.load().tfrs_vocab_build(_lib.ptr(keys), n, _lib.ptr(table), cap, _lib.ptr(flags),
                                            _lib.current_stream()))
    at_empty = (keys == EMPTY_KEY).nonzero().reshape(-1)
    flag = int(flags.item())
    if flag & _DUPLICATE_KEY or at_empty.numel() > 1:
      raise ValueError(self._duplicate_message())
    if flag & _TABLE_FULL:
      raise RuntimeError("vocabulary table: a token found no free slot")
    self._table, self._n_tokens = table, n
    self._empty_value = int(at_empty[0]) if at_empty.numel() else -1
    self._unknown = torch.zeros((1,), dtype=torch.int64, device=keys.device)

  def _require_table(self) -> torch.Tensor:
    if self._table is None:
      self.set_vocabulary([])
    return self._table

  def _lookup_keys(self, keys: torch.Tensor, validate: bool) -> torch.Tensor:
    table = self._require_table()
    flat = keys.to(table.device).reshape(-1).contiguous()
    out = torch.empty(flat.shape, dtype=torch.int64, device=table.device)
    if validate:
      self._unknown.zero_()
    _lib.check(_lib.load().tfrs_vocab_lookup(
        _lib.ptr(flat), 1 if flat.dtype == torch.int64 else 0, flat.numel(), _lib.ptr(table), table.shape[0],
        self._n_tokens, self._base, self._has_mask, self._mask_key, self._empty_value, self._has_mask,
        self.num_oov_indices, self._oov_unsigned, _lib.ptr(self._unknown if validate else None), _lib.ptr(out),
        _lib.current_stream()))
    if validate and self.num_oov_indices == 0:
      unknown = int(self._unknown.item())
      if unknown:
        raise ValueError(f"{unknown} of {flat.numel()} ids are not in the vocabulary and "
                         "num_oov_indices=0 leaves no index for them")
    return out.reshape(keys.shape)

  def forward(self, inputs, validate: bool = False):
    if isinstance(inputs, RaggedIds):
      return inputs.with_values(self.forward(inputs.values, validate))
    if isinstance(inputs, SparseIds):
      return SparseIds(inputs.indices, self.forward(inputs.values, validate), inputs.dense_shape)
    return self._invert(inputs) if self.invert else self._lookup(inputs, validate)

  # ---- persistence: the vocabulary, not the table ----------------------------------------------
  def get_extra_state(self):
    return {"vocabulary": self._state_tokens()}

  def set_extra_state(self, state):
    self.set_vocabulary(state["vocabulary"])

  def adapt(self, data):
    """Builds the vocabulary from data: a tensor or array, or an iterable of batches.  Tokens are ordered by
    count descending, ties by token descending, and cut to ``max_tokens`` minus the special slots; mask and
    OOV tokens in the data are not counted."""
    tokens = self._count_order(_batches(data))
    if self.max_tokens is not None:
      tokens = tokens[:max(self.max_tokens - self._base, 0)]
    self.set_vocabulary(tokens)


class IntegerLookup(_IndexLookup):
  """``tf.keras.layers.IntegerLookup``: int32 / int64 ids of any shape -> int64 indices on the GPU."""

  def __init__(self, max_tokens: Optional[int] = None, num_oov_indices: int = 1, mask_token: Optional[int] = None,
               oov_token: int = -1, vocabulary=None, invert: bool = False, output_mode: str = "int",
               device: Optional[torch.device] = None, mask_value: Optional[int] = None):
    super().__init__(max_tokens, num_oov_indices, None if mask_token is None else int(mask_token), int(oov_token),
                     invert, output_mode, device, None if mask_value is None else int(mask_value))
    self._tokens = torch.empty((0,), dtype=torch.int64)
    self._inverse = None
    if vocabulary is not None:
      self.set_vocabulary(vocabulary)

  def _duplicate_message(self) -> str:
    return "the vocabulary contains repeated tokens"

  def set_vocabulary(self, vocabulary) -> None:
    """``vocabulary``: a list, array or tensor of integers.  A host vocabulary is checked for repeats on the
    host; a vocabulary that already lives on the GPU is checked by the build's compare-and-swap alone."""
    if isinstance(vocabulary, torch.Tensor):
      vocab = vocabulary.detach()
    else:
      arr = np.asarray(vocabulary if len(vocabulary) else [], dtype=None if len(vocabulary) else np.int64)
      vocab = torch.from_numpy(np.ascontiguousarray(arr))
    if vocab.dtype.is_floating_point or vocab.dtype == torch.bool or vocab.dtype.is_complex:
      raise ValueError(f"IntegerLookup needs an integer vocabulary; got {vocab.dtype}")
    vocab = vocab.reshape(-1).long()
    special = self._special_tokens()
    k = len(special)
    if k and vocab.numel() >= k and vocab[:k].tolist() == special:
      vocab = vocab[k:]
    for name, token in (("mask", self.mask_token), ("OOV", self.oov_token)):
      if token is not None and bool((vocab == token).any()):
        raise ValueError(f"the reserved {name} token {token} is only accepted at its own leading position "
                         "of the vocabulary")
    self._check_size(vocab.numel())
    if not vocab.is_cuda and torch.unique(vocab).numel() != vocab.numel():
      raise ValueError(self._duplicate_message())
    keys = vocab.to(_device(self._device)).contiguous()
    self._mask_key = 0 if self.mask_token is None else self.mask_token
    self._build_table(keys)
    self._tokens = keys
    head = torch.tensor(special, dtype=torch.int64, device=keys.device)
    self._inverse = torch.cat([head, keys])

  def get_vocabulary(self, include_special_tokens: bool = True) -> List[int]:
    return (self._special_tokens() if include_special_tokens else []) + self._tokens.tolist()

  def _state_tokens(self):
    return self._tokens.cpu()

  def _count_order(self, batches) -> torch.Tensor:
    flat = []
    for batch in batches:
      values = _values_of(batch)
      t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
      if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"IntegerLookup needs integer input; got {t.dtype}")
      flat.append(t.reshape(-1).long())
    if not flat:
      return torch.empty((0,), dtype=torch.int64)
    data = torch.cat([t.to(flat[0].device) for t in flat])
    keep = data != self.oov_token
    if self.mask_token is not None:
      keep &= data != self.mask_token
    tokens, counts = torch.unique(data[keep], return_counts=True)   # tokens ascending
    tokens, counts = tokens.flip(0), counts.flip(0)
    return tokens[torch.sort(counts, descending=True, stable=True).indices]

  def _as_ids(self, inputs) -> torch.Tensor:
    if not isinstance(inputs, torch.Tensor):
      arr = np.asarray(inputs)
      if arr.dtype.kind not in ("i", "u"):
        raise ValueError(f"IntegerLookup needs integer input; got dtype {arr.dtype}")
      inputs = torch.as_tensor(arr.astype(np.int64))
    if inputs.dtype not in (torch.int32, torch.int64):
      if inputs.dtype.is_floating_point or inputs.dtype == torch.bool:
        raise ValueError(f"IntegerLookup needs integer input; got {inputs.dtype}")
      inputs = inputs.long()
    return inputs

  def _lookup(self, inputs, validate: bool) -> torch.Tensor:
    return self._lookup_keys(self._as_ids(inputs), validate)

  def _invert(self, inputs) -> torch.Tensor:
    """Indices -> tokens, an int64 tensor on the GPU; OOV slots and out-of-range indices give ``oov_token``."""
    self._require_table()
    idx = self._as_ids(inputs).to(self._inverse.device).long()
    size = self._inverse.numel()
    inside = (idx >= 0) & (idx < size)
    if size == 0:
      return torch.full_like(idx, self.oov_token)
    return torch.where(inside, self._inverse[idx.clamp(0, size - 1)], torch.full_like(idx, self.oov_token))


class StringLookup(_IndexLookup):
  """``tf.keras.layers.StringLookup``: arrays or lists of ``str`` / ``bytes`` -> int64 indices on the GPU.

  A string is known by the 64-bit SipHash-2-4 fingerprint of its UTF-8 bytes: an unknown string whose
  fingerprint equals a token's is taken for that token (chance 2^-64 per pair)."""

  _oov_unsigned = 1

  def __init__(self, max_tokens: Optional[int] = None, num_oov_indices: int = 1, mask_token: Optional[str] = None,
               oov_token: str = "[UNK]", vocabulary=None, invert: bool = False, output_mode: str = "int",
               device: Optional[torch.device] = None, mask_value: Optional[str] = None):
    super().__init__(max_tokens, num_oov_indices, None if mask_token is None else _as_bytes(mask_token),
                     _as_bytes(oov_token), invert, output_mode, device,
                     None if mask_value is None else _as_bytes(mask_value))
    self._tokens: List[bytes] = []
    if vocabulary is not None:
      self.set_vocabulary(vocabulary)

  def _duplicate_message(self) -> str:
    return "the vocabulary contains repeated tokens, or two tokens with the same 64-bit fingerprint"

  def _fingerprints(self, strings, dev: torch.device) -> torch.Tensor:
    arr = np.empty(len(strings), dtype=object)
    arr[:] = [_as_bytes(x) for x in strings]
    d_blob, d_off = pack_strings(arr, dev)
    out = torch.empty((len(strings),), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().tfrs_fingerprint_bytes(_lib.ptr(d_blob), _lib.ptr(d_off), len(strings), _lib.ptr(out),
                                                  _lib.current_stream()))
    return out

  def set_vocabulary(self, vocabulary) -> None:
    """``vocabulary``: a list or array of ``str`` or ``bytes``."""
    arr = _string_array(vocabulary).reshape(-1)
    if any(not isinstance(x, (str, bytes, np.str_, np.bytes_)) for x in arr):
      raise ValueError("StringLookup needs a vocabulary of str or bytes")
    vocab = [_as_bytes(x) for x in arr]
    special = self._special_tokens()
    k = len(special)
    if k and len(vocab) >= k and vocab[:k] == special:
      vocab = vocab[k:]
    for name, token in (("mask", self.mask_token), ("OOV", self.oov_token)):
      if token is not None and token in vocab:
        raise ValueError(f"the reserved {name} token {token!r} is only accepted at its own leading position "
                         "of the vocabulary")
    self._check_size(len(vocab))
    if len(set(vocab)) != len(vocab):
      raise ValueError("the vocabulary contains repeated tokens")
    dev = _device(self._device)
    prints = self._fingerprints(([self.mask_token] if self._has_mask else []) + vocab, dev)
    keys = prints[self._has_mask:]
    if self._has_mask:
      self._mask_key = int(prints[0])
      if bool((keys == self._mask_key).any()):
        raise ValueError("a vocabulary token has the mask token's 64-bit fingerprint")
    self._build_table(keys.contiguous())
    self._tokens = vocab

  def get_vocabulary(self, include_special_tokens: bool = True) -> List[str]:
    tokens = (self._special_tokens() if include_special_tokens else []) + self._tokens
    return [t.decode("utf-8", "surrogateescape") for t in tokens]

  def _state_tokens(self):
    return list(self._tokens)

  def _count_order(self, batches) -> List[bytes]:
    counts = collections.Counter()
    for batch in batches:
      values = _values_of(batch)
      counts.update(_as_bytes(x) for x in _string_array(values).reshape(-1))
    counts.pop(self.oov_token, None)
    if self.mask_token is not None:
      counts.pop(self.mask_token, None)
    by_token = sorted(counts, reverse=True)                       # UTF-8 bytes descending
    return sorted(by_token, key=lambda t: -counts[t])             # stable: count descending

  def _lookup(self, inputs, validate: bool) -> torch.Tensor:
    if isinstance(inputs, PackedStrings):      # each packed string is one token; nothing is packed on the host
      table = self._require_table()
      packed = inputs.to(table.device)
      keys = torch.empty((packed.n,), dtype=torch.int64, device=table.device)
      blob = packed.bytes if packed.bytes.numel() else packed.bytes.new_zeros(1)
      _lib.check(_lib.load().tfrs_fingerprint_bytes(_lib.ptr(blob), _lib.ptr(packed.offsets), packed.n,
                                                    _lib.ptr(keys), _lib.current_stream()))
      return self._lookup_keys(keys, validate)
    if isinstance(inputs, torch.Tensor):
      raise ValueError(f"StringLookup needs string input; got a tensor of {inputs.dtype}")
    arr = _string_array(inputs)
    if arr.dtype.kind not in ("U", "S", "O") or (arr.dtype.kind == "O" and not all(
        isinstance(x, (str, bytes)) for x in arr.reshape(-1))):
      raise ValueError(f"StringLookup needs string input; got dtype {arr.dtype}")
    table = self._require_table()
    return self._lookup_keys(self._fingerprints(arr.reshape(-1), table.device).reshape(arr.shape), validate)

  def _invert(self, inputs) -> np.ndarray:
    """Indices -> tokens, a NumPy array of ``str`` on the host; OOV slots and out-of-range indices give
    ``oov_token``."""
    idx = inputs.detach().cpu().numpy() if isinstance(inputs, torch.Tensor) else np.asarray(inputs)
    if idx.dtype.kind not in ("i", "u"):
      raise ValueError(f"StringLookup(invert=True) needs integer indices; got dtype {idx.dtype}")
    names = np.array(self.get_vocabulary() + [self.oov_token.decode("utf-8", "surrogateescape")], dtype=object)
    oov = len(names) - 1
    idx = idx.astype(np.int64)
    return names[np.where((idx >= 0) & (idx < oov), idx, oov)]


# ---- TextVectorization -------------------------------------------------------------------------------
TEXT_WINDOW_BYTES = 16384     # TFRS_TEXT_WINDOW_BYTES: the LDS window of the kernel's window variant
TEXT_MAX_BLOCKS = 2048        # TFRS_TEXT_MAX_BLOCKS: workgroups of 256 strings per launch, grid-stride beyond
PUNCTUATION = b"!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"     # the 32 bytes `strip_punctuation` deletes
WHITESPACE = b" \t\n\v\f\r"                              # the 6 bytes `split="whitespace"` splits at
_STANDARDIZE = {None: 0, "lower": 1, "strip_punctuation": 2, "lower_and_strip_punctuation": 3}   # TFRS_TEXT_* bits
_SPLIT = {None: 0, "whitespace": 1}
_LOWER = bytes.maketrans(bytes(range(65, 91)), bytes(range(97, 123)))


def _standardize(text: bytes, mode) -> bytes:
  """The kernel's standardisation restated on the host, byte by byte, ASCII only (``adapt`` runs it over one
  span per distinct token)."""
  code = _STANDARDIZE[mode]
  if code & 2:
    text = text.translate(None, PUNCTUATION)
  if code & 1:
    text = text.translate(_LOWER)
  return text


def _text_batches(data):
  if isinstance(data, PackedStrings):
    return [data]
  if isinstance(data, (list, tuple)) and any(isinstance(x, PackedStrings) for x in data):
    return list(data)
  return _batches(data)


class TextVectorization(torch.nn.Module):
  """``tf.keras.layers.TextVectorization``: strings -> int64 token indices on the GPU, standardised, split and
  looked up by ONE kernel (``csrc/text.hip``); the first layer of the title tower
  ``TextVectorization -> Embedding(mask_zero=True) -> GlobalAveragePooling1D`` of the reference's tutorials,
  whose other half is ``embedding.embedding_lookup_sparse(table, values, row_splits, combiner="mean")``.

  Keras is not part of the reference tree: the rules below are this layer's contract.

  Index 0 is the padding token ``""``, index 1 is ``"[UNK]"``, the vocabulary follows from 2; ``max_tokens`` counts
  the two special entries.  Standardisation works on bytes and knows ASCII only: ``lower`` maps ``A-Z`` to
  ``a-z``; ``strip_punctuation`` DELETES the 32 bytes of ``PUNCTUATION`` (``it's`` -> ``its``, ``a-b`` -> ``ab``,
  ``a - b`` -> ``a``, ``b``); bytes ``0x80-0xFF`` pass unchanged (``É`` is not lowered).  ``split="whitespace"``
  cuts at the six bytes of ``WHITESPACE``: tokens are maximal runs of other bytes, and a token whose bytes were all
  deleted does not exist; ``split=None`` makes the whole standardised string one token, and an empty one no token.
  A token is known by the 64-bit SipHash-2-4 fingerprint of its standardised bytes, as in ``StringLookup``, which
  holds the vocabulary, the table and the persistent state of this layer.

  Input: a list or array of ``str`` / ``bytes`` of shape ``[n]`` or ``[n, 1]`` (packed on the host per call, as
  ``StringLookup`` does), or a ``PackedStrings``.  Output, int64 on the GPU:

  * ``output_sequence_length=L``: dense ``[n, L]``, the first ``L`` tokens, padded with 0.  One launch, no host
    synchronisation, nothing allocated but the output: with a device-resident ``PackedStrings`` the call can be
    captured in a graph.
  * ``ragged=True``: a ``RaggedIds`` whose values hold no 0.  One count pass, one host read of the total, one
    launch.
  * neither: dense, padded to the longest row of the batch.  This costs one count pass and one host read of the
    longest row's length before the launch.

  One very long string is walked by one lane of the kernel: correct, and slow for that string alone."""

  def __init__(self, max_tokens: Optional[int] = None, standardize="lower_and_strip_punctuation",
               split="whitespace", ngrams=None, output_mode: str = "int",
               output_sequence_length: Optional[int] = None, vocabulary=None, ragged: bool = False,
               device: Optional[torch.device] = None):
    super().__init__()
    if callable(standardize):
      raise NotImplementedError("a callable `standardize` cannot run inside the kernel; standardise the strings "
                                "first and pass standardize=None")
    if standardize not in _STANDARDIZE:
      raise ValueError(f"`standardize` must be one of {[k for k in _STANDARDIZE]}; got {standardize!r}")
    if callable(split) or split == "character":
      raise NotImplementedError(f"split={split!r}: only 'whitespace' and None are on the hot path")
    if split not in _SPLIT:
      raise ValueError(f"`split` must be 'whitespace' or None; got {split!r}")
    if ngrams is not None:
      raise NotImplementedError("ngrams are not on the hot path")
    if output_mode != "int":
      raise NotImplementedError(f"output_mode={output_mode!r}: only 'int' is on the hot path")
    if ragged and output_sequence_length is not None:
      raise ValueError("`ragged=True` and `output_sequence_length` exclude each other")
    if output_sequence_length is not None and int(output_sequence_length) < 1:
      raise ValueError(f"`output_sequence_length` must be at least 1; got {output_sequence_length}")
    self.standardize, self.split = standardize, split
    self.output_mode = output_mode
    self.output_sequence_length = None if output_sequence_length is None else int(output_sequence_length)
    self.ragged = bool(ragged)
    self._device = device
    self._lookup = StringLookup(max_tokens=max_tokens, num_oov_indices=1, mask_token="", oov_token="[UNK]",
                                device=device)
    if vocabulary is not None:
      self.set_vocabulary(vocabulary)

  @property
  def max_tokens(self) -> Optional[int]:
    return self._lookup.max_tokens

  # ---- vocabulary: all of it is the inner StringLookup's ------------------------------------------------
  def set_vocabulary(self, vocabulary) -> None:
    """``vocabulary``: a list or array of ``str`` / ``bytes``, taken as they are (NOT standardised); a leading
    ``["", "[UNK]"]`` is dropped."""
    self._lookup.set_vocabulary(vocabulary)

  def get_vocabulary(self, include_special_tokens: bool = True) -> List[str]:
    return self._lookup.get_vocabulary(include_special_tokens)

  def vocabulary_size(self) -> int:
    return self._lookup.vocabulary_size()

  # ---- launches -----------------------------------------------------------------------------------------
  def _codes(self):
    return _STANDARDIZE[self.standardize], _SPLIT[self.split]

  def _pack(self, inputs, dev: torch.device) -> PackedStrings:
    if isinstance(inputs, PackedStrings):
      return inputs.to(dev)
    if isinstance(inputs, torch.Tensor):
      raise ValueError(f"TextVectorization needs string input; got a tensor of {inputs.dtype}")
    arr = _string_array(inputs)
    if arr.dtype.kind not in ("U", "S", "O") or (arr.dtype.kind == "O" and not all(
        isinstance(x, (str, bytes)) for x in arr.reshape(-1))):
      raise ValueError(f"TextVectorization needs string input; got dtype {arr.dtype}")
    if not (arr.ndim == 1 or (arr.ndim == 2 and arr.shape[1] == 1)):
      raise ValueError(f"TextVectorization needs input of shape [n] or [n, 1]; got {arr.shape}")
    return PackedStrings.from_strings(arr.reshape(-1), dev)

  def _count(self, packed: PackedStrings):
    """(tokens per string [n], row_splits [n + 1]) on the device."""
    standardize, split = self._codes()
    counts = torch.empty((packed.n,), dtype=torch.int64, device=packed.device)
    _lib.check(_lib.load().tfrs_text_count_tokens(
        _lib.ptr(packed.bytes), packed.bytes.numel(), _lib.ptr(packed.offsets), packed.n, standardize, split,
        _lib.ptr(counts), _lib.current_stream()))
    row_splits = torch.zeros((packed.n + 1,), dtype=torch.int64, device=packed.device)
    torch.cumsum(counts, 0, out=row_splits[1:])
    return counts, row_splits

  def _vectorize(self, packed: PackedStrings, row_splits, seq_len: int, out: torch.Tensor) -> torch.Tensor:
    standardize, split = self._codes()
    table = self._lookup._require_table()
    _lib.check(_lib.load().tfrs_text_vectorize(
        _lib.ptr(packed.bytes), packed.bytes.numel(), _lib.ptr(packed.offsets), packed.n, standardize, split,
        _lib.ptr(table), table.shape[0], self._lookup._n_tokens, self._lookup._empty_value, _lib.ptr(row_splits),
        seq_len, _lib.ptr(out), _lib.current_stream()))
    return out

  def forward(self, inputs):
    dev = self._lookup._require_table().device
    packed = self._pack(inputs, dev)
    n = packed.n
    if self.output_sequence_length is not None:
      out = torch.empty((n, self.output_sequence_length), dtype=torch.int64, device=dev)
      return self._vectorize(packed, None, self.output_sequence_length, out)
    counts, row_splits = self._count(packed)
    if self.ragged:
      values = torch.empty((int(row_splits[-1]),), dtype=torch.int64, device=dev)
      if values.numel():
        self._vectorize(packed, row_splits, 0, values)
      return RaggedIds(values, row_splits)
    longest = int(counts.max()) if n else 0
    out = torch.empty((n, longest), dtype=torch.int64, device=dev)
    return self._vectorize(packed, None, longest, out) if longest else out

  # ---- adapt ----------------------------------------------------------------------------------------------
  def _count_batch(self, packed: PackedStrings, totals: collections.Counter) -> None:
    """Adds the batch's token counts into ``totals``: tokenising, fingerprinting and counting run on the device;
    the host sees one raw span per distinct fingerprint and standardises it with ``_standardize``."""
    standardize, split = self._codes()
    _, row_splits = self._count(packed)
    total = int(row_splits[-1])
    if not total:
      return
    prints, starts, ends = (torch.empty((total,), dtype=torch.int64, device=packed.device) for _ in range(3))
    _lib.check(_lib.load().tfrs_text_token_spans(
        _lib.ptr(packed.bytes), packed.bytes.numel(), _lib.ptr(packed.offsets), packed.n, standardize, split,
        _lib.ptr(row_splits), _lib.ptr(prints), _lib.ptr(starts), _lib.ptr(ends), _lib.current_stream()))
    distinct, inverse, counts = torch.unique(prints, return_inverse=True, return_counts=True)
    first = torch.full((distinct.numel(),), total, dtype=torch.int64, device=packed.device)
    first.scatter_reduce_(0, inverse, torch.arange(total, device=packed.device), reduce="amin")
    lo, hi = starts[first], ends[first]
    lengths = hi - lo
    at = torch.cumsum(lengths, 0) - lengths          # where each span begins in the gathered bytes
    which = torch.repeat_interleave(lo - at, lengths) + torch.arange(int(lengths.sum()), device=packed.device)
    raw = packed.bytes[which].cpu().numpy().tobytes()
    for a, ln, c in zip(at.tolist(), lengths.tolist(), counts.tolist()):
      totals[_standardize(raw[a:a + ln], self.standardize)] += c

  def adapt(self, data) -> None:
    """Builds the vocabulary from data: a list or array of strings, a ``PackedStrings``, or an iterable of such
    batches.  The data is standardised and split as ``forward`` does; tokens are ordered by count descending,
    ties by token bytes descending (``StringLookup.adapt``'s rule), and cut to ``max_tokens - 2``."""
    dev = _device(self._device)
    totals = collections.Counter()
    for batch in _text_batches(data):
      self._count_batch(self._pack(batch, dev), totals)
    totals.pop(self._lookup.oov_token, None)       # "[UNK]" survives standardize=None: it keeps its own index
    by_token = sorted(totals, reverse=True)
    tokens = sorted(by_token, key=lambda t: -totals[t])
    if self.max_tokens is not None:
      tokens = tokens[:max(self.max_tokens - 2, 0)]
    self.set_vocabulary(tokens)
