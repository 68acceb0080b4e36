"""``FlatIndex`` -- exact k-nearest-neighbour search over rows kept on the device.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_flat_*, vq_amd/csrc/k_knn.hip):
``D(q, i)`` is ``Distance.compute(q, rows[i])`` bit for bit (f16 rows widened exactly to f32 first), the result per
query is the ``topk`` rows by ``(D, row index)`` ascending with NaN last, and ``rerank`` applies the same order to a
caller's candidate lists; ``range_search`` returns every row with ``D(q, i) <= radius`` instead, in ascending row
index (CSR).  Every argument is checked here before the device is touched; the rows go to the device once,
on the first search (until then the index refers to the caller's array, which must not change in between).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._resident_common import MAX_CANDIDATES, MAX_TOPK, ExactResidentIndex, _check_distance, _count  # noqa: F401
from .distance import Distance
from .errors import DimensionMismatch, InvalidParameter


class FlatIndex(ExactResidentIndex):
    """Exact search over `rows` (n, d) float32 or float16 under `distance` (any metric, cosine included)."""

    def __init__(self, rows, distance: Distance | None = None):
        distance = _check_distance(distance, Distance.euclidean())
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype not in (np.float32, np.float16):
            raise InvalidParameter("rows", f"dtype must be float32 or float16, got {a.dtype}")
        self._set_source(a, "rows", distance)
        self._dtype = a.dtype

    @property
    def dtype(self) -> np.dtype:
        return np.dtype(self._dtype)

    def __repr__(self) -> str:
        return f"FlatIndex(n={self._n}, dim={self._dim}, dtype={np.dtype(self._dtype).name}, distance={self._distance!r})"

    def _make_handle(self) -> "_lib.Flat":
        return _lib.Flat(self._src, self._distance.metric)

    def _add_form(self):
        return "add", self._dtype, ()  # rows in the index's own dtype, stored as they are


def adc_then_rerank(adc_search, n: int, dim: int, queries: np.ndarray, topk: int, rerank, candidates):
    """the standard PQ pipeline: `adc_search(queries, c)` for a short list of c candidates per query (default 4 topk,
    at most 1024 -- ADC's own limit -- and n), then the exact rerank of that list through `rerank`, a FlatIndex or a
    ScalarIndex over the same n rows.  The rerank index's metric is its own (cosine allowed)."""
    c = rerank_candidates(n, dim, topk, rerank, candidates)
    idx, _ = adc_search(queries, c)
    return rerank.rerank(queries, idx, topk)


def rerank_candidates(n: int, dim: int, topk: int, rerank, candidates) -> int:
    """the checks of a short list reranked through `rerank`, a FlatIndex, a ScalarIndex or an AsymmetricBinaryIndex over the
    same n rows of dim: the list's length (default 4 topk, at most 1024 and n)"""
    if not isinstance(rerank, ExactResidentIndex):
        raise InvalidParameter("rerank", f"expected a FlatIndex, a ScalarIndex or an AsymmetricBinaryIndex, got {type(rerank).__name__}")
    if len(rerank) != n:
        raise DimensionMismatch(n, len(rerank))
    if rerank.dim != dim:
        raise DimensionMismatch(dim, rerank.dim)
    c = min(4 * topk, MAX_TOPK, n) if candidates is None else _count(candidates, "candidates")
    if not topk <= c <= min(n, MAX_TOPK):
        raise InvalidParameter("candidates", f"must be between topk and min(n, 1024), got {c}")
    return c
