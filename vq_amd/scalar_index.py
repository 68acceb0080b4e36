"""``ScalarIndex`` -- exact top-k search and exact rerank over SQ codes kept on the device, one byte per dimension.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_sqindex_*, vq_amd/csrc/k_sqindex.hip):
a ``ScalarQuantizer(min, max, levels)`` fixes ``v(c) = min + float32(c) * step`` for every byte value (codes >= levels
included), and ``D(q, i) = Distance.compute(q, v(codes[i]))`` bit for bit under any of the five metrics.  The queries
are float32 and never quantized.  Every result equals ``FlatIndex(quantizer.dequantize_batch(codes), distance)`` on the
same call -- indices, and distances as uint32 bits -- at a quarter of the device memory: n * d bytes, plus 4 n for the
row norms under cosine.

Every argument is checked here before the device is touched; the index goes to the device on the first search (until
then it refers to the caller's array, which must not change in between).  An index built from float32 rows encodes them
on the device and keeps only the codes.  ``save`` / ``load`` of an index built ``from_codes`` need no device.

File layout (``save`` / ``load``), little-endian, no padding::

    offset  size  field
    0       8     magic  b"VQSQIDX1"
    8       8     n      uint64, rows, 1 <= n < 2^32
    16      4     d      uint32, dimensions, >= 1
    20      4     metric uint32, 0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped
    24      4     min    float32
    28      4     max    float32
    32      4     levels uint32, 2..256
    36      n*d   codes  uint8, row-major
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from .distance import Distance
from .errors import DimensionMismatch, EmptyInput, InvalidData, InvalidParameter
from .flat import DEFAULT_MAX_RESULTS, MAX_CANDIDATES, MAX_TOPK, _count, _max_results, _radii
from .sq import ScalarQuantizer

MAGIC = b"VQSQIDX1"
_HEADER = struct.Struct("<8sQIIffI")  # magic, n, d, metric, min, max, levels
_METRIC_NAMES = {_lib.SQUARED_EUCLIDEAN: "squared_euclidean", _lib.EUCLIDEAN: "euclidean", _lib.MANHATTAN: "manhattan",
                 _lib.COSINE: "cosine", _lib.COSINE_UNCLAMPED: "cosine_unclamped"}


class ScalarIndex:
    """Exact search over `rows` (n, d) float32, stored as the codes of `quantizer`, under `distance` (any metric, cosine
    included; default Euclidean)."""

    def __init__(self, rows, quantizer: ScalarQuantizer, distance: Distance | None = None):
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype != np.float32:
            raise InvalidParameter("rows", f"dtype must be float32, got {a.dtype}")
        self._setup(a, True, quantizer, distance)

    @classmethod
    def from_codes(cls, codes, quantizer: ScalarQuantizer, distance: Distance | None = None) -> "ScalarIndex":
        """u8 SQ codes (n, d), e.g. ``quantizer.quantize_batch(rows)``; every byte value is legal"""
        a = codes if isinstance(codes, np.ndarray) else np.asarray(codes)
        if a.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {a.dtype}")
        self = cls.__new__(cls)
        self._setup(a, False, quantizer, distance)
        return self

    def _setup(self, a: np.ndarray, rows: bool, quantizer, distance) -> None:
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        if distance is None:
            distance = Distance.euclidean()
        if not isinstance(distance, Distance):
            raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
        what = "rows" if rows else "codes"
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if a.shape[0] == 0:
            raise EmptyInput()
        if a.shape[1] == 0:
            raise InvalidParameter(what, "dimension must be at least 1")
        if a.shape[0] >= 1 << 32:
            raise InvalidParameter(what, f"at most 2^32 - 1 rows, got {a.shape[0]}")
        self._src = np.ascontiguousarray(a)
        self._rows = rows
        self._n, self._dim = int(a.shape[0]), int(a.shape[1])
        self._quantizer, self._distance = quantizer, distance
        self._ix = None

    def __len__(self) -> int:
        return self._n

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    @property
    def distance(self) -> Distance:
        return self._distance

    def __repr__(self) -> str:
        return f"ScalarIndex(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, distance={self._distance!r})"

    def _index(self) -> "_lib.SQIndex":
        if self._ix is None:
            q = self._quantizer
            self._ix = _lib.SQIndex(self._src, self._rows, self._n, self._dim, q._min, q._max, q.levels, self._distance.metric)
            self._src = None  # on the device now
        return self._ix

    def _queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError("expected a 2D array (nq, dim)")
        if q.shape[1] != self._dim:
            raise DimensionMismatch(self._dim, q.shape[1])
        if q.shape[0] >= 1 << 32:
            raise InvalidParameter("queries", f"at most 2^32 - 1 queries, got {q.shape[0]}")
        return q

    def _topk(self, topk, limit: int, what: str) -> int:
        k = _count(topk, "topk")
        if not 1 <= k <= limit:
            raise InvalidParameter("topk", f"must be between 1 and {what}, got {k}")
        return k

    def codes(self) -> np.ndarray:
        """the codes, uint8 (n, d): the caller's for an index built from codes and not yet searched, else from the device"""
        if self._ix is None and not self._rows:
            return self._src.copy()
        return self._index().codes()

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
        """every row within `radius` of each query, as ``FlatIndex.range_search`` over the dequantized codes: (lims uint64
        (nq + 1,), idx uint32 (total,), dist float32 (total,)), the hits of a query in ascending row id"""
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

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        codes = self.codes()
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, q._min, q._max, q.levels))
            f.write(np.ascontiguousarray(codes, dtype=np.uint8).tobytes())

    @classmethod
    def load(cls, path) -> "ScalarIndex":
        """read a VQSQIDX1 file; every field is checked here, before anything can reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise InvalidData("truncated scalar index header")
            magic, n, dim, metric, mn, mx, levels = _HEADER.unpack(head)
            if magic != MAGIC:
                raise InvalidData("not a VQSQIDX1 file")
            if metric not in _METRIC_NAMES:
                raise InvalidParameter("distance", f"unknown metric id {metric}")
            if dim < 1:
                raise InvalidParameter("dim", "must be at least 1")
            if not 1 <= n < 1 << 32:
                raise InvalidData(f"row count {n} is outside [1, 2^32)")
            quantizer = ScalarQuantizer(mn, mx, levels)  # the reference's own checks
            raw = f.read(n * dim)
            if len(raw) != n * dim:
                raise InvalidData("truncated codes")
            if f.read(1):
                raise InvalidData("trailing bytes after the codes")
        codes = np.frombuffer(raw, dtype=np.uint8).reshape(n, dim)
        return cls.from_codes(codes, quantizer, Distance(_METRIC_NAMES[metric]))
