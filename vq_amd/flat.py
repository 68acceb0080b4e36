"""``FlatIndex`` -- exact k-nearest-neighbour search over rows kept on the device.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_flat_*, vq_amd/csrc/k_knn.hip):
``D(q, i)`` is ``Distance.compute(q, rows[i])`` bit for bit (f16 rows widened exactly to f32 first), the result per
query is the ``topk`` rows by ``(D, row index)`` ascending with NaN last, and ``rerank`` applies the same order to a
caller's candidate lists; ``range_search`` returns every row with ``D(q, i) <= radius`` instead, in ascending row
index (CSR).  Every argument is checked here before the device is touched; the rows go to the device once,
on the first search (until then the index refers to the caller's array, which must not change in between).
"""
from __future__ import annotations

import operator

import numpy as np

from . import _lib
from .distance import Distance
from .errors import DimensionMismatch, EmptyInput, InvalidParameter

MAX_TOPK = 1024
MAX_CANDIDATES = 4096


def _count(v, name: str) -> int:
    try:
        return operator.index(v)
    except TypeError:
        raise InvalidParameter(name, f"must be an integer, got {v!r}") from None


DEFAULT_MAX_RESULTS = 1 << 28  # hits a range search returns at most by default: 2 GB of idx + dist


def _radii(radius, nq: int) -> np.ndarray:
    """the per-query radii float32 (nq,) of a range search from a scalar or nq values; NaN is refused"""
    try:
        r = np.asarray(radius, dtype=np.float32)
    except (TypeError, ValueError):
        raise InvalidParameter("radius", f"must be a number or an array of {nq} numbers, got {radius!r}") from None
    if r.ndim == 0:
        r = np.full(nq, r, np.float32)
    if r.ndim != 1:
        raise InvalidParameter("radius", f"must be a scalar or a 1D array, got {r.ndim} dimensions")
    if r.shape[0] != nq:
        raise DimensionMismatch(nq, r.shape[0])
    if bool(np.isnan(r).any()):
        raise InvalidParameter("radius", f"is NaN for query {int(np.flatnonzero(np.isnan(r))[0])}")
    return np.ascontiguousarray(r)


def _max_results(max_results) -> int:
    m = _count(max_results, "max_results")
    if not 1 <= m < 1 << 64:
        raise InvalidParameter("max_results", f"must be in [1, 2^64), got {m}")
    return m


class FlatIndex:
    """Exact search over `rows` (n, d) float32 or float16 under `distance` (any metric, cosine included)."""

    def __init__(self, rows, distance: Distance | None = None):
        if distance is None:
            distance = Distance.euclidean()
        if not isinstance(distance, Distance):
            raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype not in (np.float32, np.float16):
            raise InvalidParameter("rows", f"dtype must be float32 or float16, got {a.dtype}")
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if a.shape[0] == 0:
            raise EmptyInput()
        if a.shape[1] == 0:
            raise InvalidParameter("rows", "dimension must be at least 1")
        if a.shape[0] >= 1 << 32:
            raise InvalidParameter("rows", f"at most 2^32 - 1 rows, got {a.shape[0]}")
        self._rows = np.ascontiguousarray(a)
        self._n, self._dim = a.shape
        self._dtype = a.dtype
        self._distance = distance
        self._flat = None

    def __len__(self) -> int:
        return self._n

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def dtype(self) -> np.dtype:
        return np.dtype(self._dtype)

    @property
    def distance(self) -> Distance:
        return self._distance

    def __repr__(self) -> str:
        return f"FlatIndex(n={self._n}, dim={self._dim}, dtype={np.dtype(self._dtype).name}, distance={self._distance!r})"

    def _index(self) -> "_lib.Flat":
        if self._flat is None:
            self._flat = _lib.Flat(self._rows, self._distance.metric)
            self._rows = None  # on the device now
        return self._flat

    def _queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError("expected a 2D array (nq, dim)")
        if q.shape[1] != self._dim:
            raise DimensionMismatch(self._dim, q.shape[1])
        return q

    def _topk(self, topk, limit: int, what: str) -> int:
        k = _count(topk, "topk")
        if not 1 <= k <= limit:
            raise InvalidParameter("topk", f"must be between 1 and {what}, got {k}")
        return k

    def search(self, queries, topk: int = 10):
        """(nq, d) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first"""
        q = self._queries(queries)
        k = self._topk(topk, min(self._n, MAX_TOPK), "min(n, 1024)")
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        return self._index().search(q, k)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int) -> None:
        """device pointers: queries [nq][d] f32, results [nq][topk] uint32 / f32 (4-byte aligned); asynchronous on the
        current stream"""
        k = self._topk(topk, min(self._n, MAX_TOPK), "min(n, 1024)")
        n_q = _count(nq, "nq")
        if n_q < 0 or n_q >= 1 << 32:
            raise InvalidParameter("nq", f"must be in [0, 2^32), got {n_q}")
        self._index().search_device(int(dev_queries), n_q, k, int(dev_idx), int(dev_dist))

    def range_search(self, queries, radius, max_results: int = DEFAULT_MAX_RESULTS):
        """every row within `radius` of each query: row i is a hit of query q iff D(q, i) <= radius[q] as a float32
        comparison (NaN distances never hit).  `radius` is a scalar or nq values.  Returns (lims uint64 (nq + 1,),
        idx uint32 (total,), dist float32 (total,)): the hits of query q are idx[lims[q]:lims[q + 1]], in ascending
        row id.  More than `max_results` hits in all: FfiError (ERR_UNSUPPORTED)."""
        q = self._queries(queries)
        r = _radii(radius, q.shape[0])
        m = _max_results(max_results)
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._index().range_search(q, r, m).read()

    def range_search_device(self, dev_queries: int, nq: int, radius, max_results: int = DEFAULT_MAX_RESULTS) -> "_lib.RangeResult":
        """`range_search` with the queries [nq][d] f32 at a device pointer (4-byte aligned) and the result left on the
        device: a RangeResult (.total, .lims, .device_pointers(), .read()).  Returns when the result is complete."""
        n_q = _count(nq, "nq")
        if n_q < 0 or n_q >= 1 << 32:
            raise InvalidParameter("nq", f"must be in [0, 2^32), got {n_q}")
        r = _radii(radius, n_q)
        m = _max_results(max_results)
        return self._index().range_search_device(int(dev_queries), n_q, r, m)

    def rerank(self, queries, candidates, topk: int = 10):
        """per query, the `topk` nearest of its candidate row ids (nq, c), 1 <= c <= 4096, distinct within a query;
        returns (indices uint32 (nq, topk), distances float32 (nq, topk)) in the order of `search`"""
        q = self._queries(queries)
        c = np.asarray(candidates)
        if c.ndim == 1 and q.shape[0] == 1:
            c = c[None, :]
        if c.ndim != 2:
            raise ValueError("expected candidates as a 2D array (nq, c)")
        if c.shape[0] != q.shape[0]:
            raise DimensionMismatch(q.shape[0], c.shape[0])
        if c.dtype.kind not in "iu":
            raise InvalidParameter("candidates", f"row ids must be integers, got {c.dtype}")
        if not 1 <= c.shape[1] <= MAX_CANDIDATES:
            raise InvalidParameter("candidates", f"between 1 and {MAX_CANDIDATES} per query, got {c.shape[1]}")
        k = self._topk(topk, c.shape[1], "the number of candidates")
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        lo, hi = int(c.min()), int(c.max())
        if lo < 0 or hi >= self._n:
            bad = lo if lo < 0 else hi
            raise InvalidParameter("candidates", f"row id {bad} is outside [0, {self._n})")
        s = np.sort(c, axis=1)
        if c.shape[1] > 1 and bool((s[:, 1:] == s[:, :-1]).any()):
            raise InvalidParameter("candidates", "row ids must be distinct within a query")
        return self._index().rerank(q, np.ascontiguousarray(c, dtype=np.uint32), k)


def adc_then_rerank(adc_search, n: int, dim: int, queries: np.ndarray, topk: int, rerank, candidates):
    """the standard PQ pipeline: `adc_search(queries, c)` for a short list of c candidates per query (default 4 topk,
    at most 1024 -- ADC's own limit -- and n), then the exact rerank of that list through `rerank`, a FlatIndex or a
    ScalarIndex over the same n rows.  The rerank index's metric is its own (cosine allowed)."""
    c = rerank_candidates(n, dim, topk, rerank, candidates)
    idx, _ = adc_search(queries, c)
    return rerank.rerank(queries, idx, topk)


def rerank_candidates(n: int, dim: int, topk: int, rerank, candidates) -> int:
    """the checks of a short list reranked through `rerank`, a FlatIndex or a ScalarIndex over the same n rows of dim:
    the list's length (default 4 topk, at most 1024 and n)"""
    from .scalar_index import ScalarIndex

    if not isinstance(rerank, (FlatIndex, ScalarIndex)):
        raise InvalidParameter("rerank", f"expected a FlatIndex or a ScalarIndex, got {type(rerank).__name__}")
    if len(rerank) != n:
        raise DimensionMismatch(n, len(rerank))
    if rerank.dim != dim:
        raise DimensionMismatch(dim, rerank.dim)
    c = min(4 * topk, MAX_TOPK, n) if candidates is None else _count(candidates, "candidates")
    if not topk <= c <= min(n, MAX_TOPK):
        raise InvalidParameter("candidates", f"must be between topk and min(n, 1024), got {c}")
    return c
