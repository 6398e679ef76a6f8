"""Experimental optimizers (mirrors tensorflow_recommenders/experimental/optimizers)."""

from recommenders_amd.experimental.optimizers.clippy_adagrad import ClippyAdagrad, shrink_by_references  # noqa: F401
from recommenders_amd.experimental.optimizers.composite_optimizer import CompositeOptimizer  # noqa: F401
