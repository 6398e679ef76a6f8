"""Layers (mirrors tensorflow_recommenders/layers/__init__.py:18-23)."""

from recommenders_amd.layers import blocks, embedding, sharded_embedding, factorized_top_k, feature_interaction, loss  # noqa: F401
from recommenders_amd.layers import feature_multiplexing, hashing, preprocessing  # noqa: F401
from recommenders_amd.layers.hashing import PackedStrings  # noqa: F401
from recommenders_amd.layers.preprocessing import IntegerLookup, StringLookup, TextVectorization  # noqa: F401
from recommenders_amd.layers import numeric  # noqa: F401
from recommenders_amd.layers.numeric import Discretization, Normalization  # noqa: F401
from recommenders_amd.layers.embedding import Embedding  # noqa: F401
from recommenders_amd.layers.recurrent import GRU  # noqa: F401
