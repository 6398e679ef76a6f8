"""Top-K retrieval layers on MI355X.

Host-side mirror of ``tensorflow_recommenders/layers/factorized_top_k.py``
(``TopK`` :140-333, ``Streaming`` :336-512, ``BruteForce`` :515-610, ``ScaNN`` :613-796): same class
names, constructor/call arguments and error behaviour.  The arithmetic
(``tf.matmul`` + ``tf.math.top_k`` + the Streaming reduce) runs in
``libtfrs_hip.so`` -- an f32-MFMA scan with the top-K selection fused behind it.

Deviations forced by the host framework (documented in DESIGN.md):
  * tensors are ``torch.Tensor`` on a CUDA(ROCm) device; NumPy inputs are uploaded;
  * a ``tf.data.Dataset`` of candidates becomes any re-iterable of candidate blocks
    ``[nb, d]`` or ``(identifiers[nb], candidates[nb, d])`` tuples;
  * identifiers of non-numeric dtype (e.g. strings) stay on the host as NumPy arrays:
    the device returns row numbers and the final ``identifiers[idx]`` gather
    (:607, :438) is done host-side; numeric identifiers are gathered on the device;
  * ``ScaNN`` (:613-796; the reference delegates to the external ``scann`` library) is built here: k-means tree,
    4-bit product-quantized residuals scanned on the matrix cores (csrc/scann.hip), optional exact re-ordering;
    its own deviations are listed in its docstring.
"""

from ._base import TopK
from ._common import (BATCH_TOO_SMALL_MESSAGE, MAX_FUSED_DIM, MAX_FUSED_K, NOT_INDEXED_MESSAGE, _as_f32_matrix,
                      compute_scores, top_k_of_block)
from .brute_force import BruteForce
from .scann import ScaNN, scann_probe_plan
from .sharded import ShardedBruteForce, ShardedStreaming
from .streaming import Streaming
