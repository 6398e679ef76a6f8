"""Experimental components (mirrors tensorflow_recommenders/experimental)."""

from recommenders_amd.experimental import layers, models, optimizers  # noqa: F401
