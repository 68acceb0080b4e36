"""``IVFFlatIndex`` -- an inverted file over the rows themselves: a query computes the exact distance to the rows of its
nearest coarse centroids' lists only.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_ivfflat_*, vq_amd/csrc/k_ivfflat.hip):
``P(q)`` is ``FlatIndex(coarse, distance).search(q, nprobe)``, ``S(q)`` the rows whose list is in ``P(q)``, ``D(q, i)``
``FlatIndex``'s distance (``Distance.compute`` bit for bit; float16 rows widened exactly), and the result the ``topk`` rows
of ``S(q)`` by ``(D, row id)`` ascending with NaN last -- with ``nprobe == nlist`` exactly ``FlatIndex(rows).search``.
Slots past ``|S(q)|`` hold id ``0xFFFFFFFF`` and distance ``+inf``.  Any of the five metrics.  Constructing, adding rows,
saving and loading need no GPU; the device handle is created by the first probe or search and follows every later add.

File layout (little endian), in the manner of ivf.py's:

    0   8   magic  b"VQIVFFL1"
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped)
    12  4   u32    dim
    16  4   u32    nlist
    20  4   u32    dtype (0 float32, 1 float16)
    24  8   u64    n
    32  ..  f32    coarse centroids [nlist][dim]
    ..  ..  u32    list ids         [n]           (row order)
    ..  ..  f32 or f16  rows        [n][dim]
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from .distance import Distance
from .errors import DimensionMismatch, InvalidParameter
from .ivf import MAX_NLIST, MAX_PROBE, MAX_TOPK, PAD_ID, _count, _nearest_lists  # noqa: F401  (PAD_ID: re-exported)

MAGIC = b"VQIVFFL1"
_HEADER = struct.Struct("<8sIIIIQ")
_METRIC_NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
_DTYPES = [np.dtype(np.float32), np.dtype(np.float16)]


def _row_dtype(dtype) -> np.dtype:
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise InvalidParameter("dtype", f"must be float32 or float16, got {dtype!r}") from None
    if dt not in _DTYPES:
        raise InvalidParameter("dtype", f"must be float32 or float16, got {dt}")
    return dt


class IVFFlatIndex:
    """coarse centroids (nlist, dim) + distance + row dtype, and the rows added to it"""

    def __init__(self, coarse_centroids, distance: Distance | None = None, dtype=np.float32):
        if distance is None:
            distance = Distance.euclidean()
        if not isinstance(distance, Distance):
            raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
        c = np.ascontiguousarray(coarse_centroids, dtype=np.float32)
        if c.ndim != 2:
            raise InvalidParameter("coarse_centroids", "must have shape (nlist, dim)")
        if not 1 <= c.shape[0] <= MAX_NLIST:
            raise InvalidParameter("nlist", f"must be between 1 and {MAX_NLIST}, got {c.shape[0]}")
        if c.shape[1] == 0:
            raise InvalidParameter("coarse_centroids", "dimension must be at least 1")
        self._distance = distance
        self._coarse = c
        self._dtype = _row_dtype(dtype)
        self._lists = np.empty(0, np.uint32)
        self._rows = np.empty((0, c.shape[1]), self._dtype)
        self._ix = None

    # -- shape ------------------------------------------------------------------------------
    @property
    def nlist(self) -> int:
        return self._coarse.shape[0]

    @property
    def dim(self) -> int:
        return self._coarse.shape[1]

    @property
    def dtype(self) -> np.dtype:
        return self._dtype

    @property
    def distance(self) -> Distance:
        return self._distance

    @property
    def coarse_centroids(self) -> np.ndarray:
        return self._coarse

    @property
    def list_ids(self) -> np.ndarray:
        """(n,) uint32: the list of every row, in row order"""
        return self._lists

    @property
    def rows(self) -> np.ndarray:
        """(n, dim): every row as stored, in row order"""
        return self._rows

    def __len__(self) -> int:
        return self._lists.shape[0]

    def __repr__(self) -> str:
        return (f"IVFFlatIndex(n={len(self)}, nlist={self.nlist}, dim={self.dim}, dtype={self._dtype.name}, "
                f"distance={self._distance!r})")

    def list_sizes(self) -> np.ndarray:
        """(nlist,) uint64: rows per list"""
        return np.bincount(self._lists, minlength=self.nlist).astype(np.uint64)

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, max_iters: int = 10, distance: Distance | None = None, seed: int = 42,
              dtype=np.float32) -> "IVFFlatIndex":
        """fit the coarse quantizer on X (k-means of whole rows: a ProductQuantizer with one subspace of nlist centroids,
        as IVFPQIndex.train); the index holds no rows yet (add them with `add`)"""
        from .pq import ProductQuantizer

        distance = distance if distance is not None else Distance.euclidean()
        dt = _row_dtype(dtype)
        coarse = ProductQuantizer(X, 1, nlist, max_iters, distance, seed).codebooks[0]
        return cls(coarse, distance, dt)

    def add(self, X) -> np.ndarray:
        """assign each row of X (n, dim) to its nearest coarse centroid (the reference's nearest-centroid rule, on the
        float32 values of X) and append it, rounded to the index's dtype; returns the new row ids"""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim == 1:
            X = X[None, :]
        if X.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if X.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, X.shape[1])
        if X.shape[0] == 0:
            return np.empty(0, np.uint32)
        return self.add_rows(_nearest_lists(self._coarse, X, self._distance.metric), X)

    def add_rows(self, list_ids, rows) -> np.ndarray:
        """append rows (n, dim), converted to the index's dtype, into the lists list_ids (n,) < nlist; returns the new
        row ids"""
        lid = np.asarray(list_ids)
        r = np.asarray(rows)
        if lid.ndim != 1:
            raise InvalidParameter("list_ids", "must be a 1D array (n,)")
        if r.ndim != 2:
            raise InvalidParameter("rows", f"must have shape (n, {self.dim})")
        if r.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, r.shape[1])
        if r.shape[0] != lid.shape[0]:
            raise DimensionMismatch(lid.shape[0], r.shape[0])
        if r.dtype.kind != "f":
            raise InvalidParameter("rows", f"must be floating point, got {r.dtype}")
        if lid.size and (lid.dtype.kind not in "iu" or int(lid.min()) < 0 or int(lid.max()) >= self.nlist):
            raise InvalidParameter("list_ids", f"must be integers in [0, {self.nlist})")
        n0 = len(self)
        if n0 + lid.shape[0] >= 1 << 32:
            raise InvalidParameter("rows", "an index holds at most 2^32 - 1 rows")
        lid = np.ascontiguousarray(lid, dtype=np.uint32)
        with np.errstate(over="ignore"):
            r = np.ascontiguousarray(r, dtype=self._dtype)
        if self._ix is not None and lid.size:
            self._ix.add(lid, r)
        self._lists = np.concatenate([self._lists, lid])
        self._rows = np.concatenate([self._rows, r])
        return np.arange(n0, n0 + lid.shape[0], dtype=np.uint32)

    def _handle(self) -> "_lib.IVFFlat":
        if self._ix is None:
            ix = _lib.IVFFlat(self._coarse, self._distance.metric, self._dtype)
            if len(self):
                ix.add(self._lists, self._rows)
            self._ix = ix
        return self._ix

    # -- search -----------------------------------------------------------------------------
    def _queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError("expected a 2D array (nq, dim)")
        if q.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, q.shape[1])
        return q

    def _nprobe(self, nprobe) -> int:
        p = _count(nprobe, "nprobe")
        if not 1 <= p <= min(self.nlist, MAX_PROBE):
            raise InvalidParameter("nprobe", f"must be between 1 and min(nlist, 1024), got {p}")
        return p

    def _topk(self, topk) -> int:
        t = _count(topk, "topk")
        if not 1 <= t <= min(len(self), MAX_TOPK):
            raise InvalidParameter("topk", f"must be between 1 and min(n, 1024), got {t}")
        return t

    def probe(self, queries, nprobe: int = 8) -> np.ndarray:
        """(nq, nprobe) uint32: the lists each query scans, nearest first"""
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        if q.shape[0] == 0:
            return np.empty((0, p), np.uint32)
        return self._handle().probe(q, p)

    def search(self, queries, topk: int = 10, nprobe: int = 8):
        """(nq, dim) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first; slots
        past the probed rows hold 0xFFFFFFFF / +inf"""
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        if q.shape[0] == 0:
            return np.empty((0, t), np.uint32), np.empty((0, t), np.float32)
        return self._handle().search(q, p, t)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, nprobe: int = 8) -> None:
        """device pointers: queries [nq][dim] f32, results [nq][topk] uint32 / f32; asynchronous on the current stream"""
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        n_q = _count(nq, "nq")
        if n_q < 0 or n_q >= 1 << 32:
            raise InvalidParameter("nq", f"must be in [0, 2^32), got {n_q}")
        self._handle().search_device(int(dev_queries), n_q, p, t, int(dev_idx), int(dev_dist))

    def close(self) -> None:
        """release the device handle (the next probe or search builds it again)"""
        if self._ix is not None:
            self._ix.close()
            self._ix = None

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._distance.metric, self.dim, self.nlist, _DTYPES.index(self._dtype), len(self)))
            f.write(self._coarse.astype("<f4").tobytes())
            f.write(self._lists.astype("<u4").tobytes())
            f.write(self._rows.astype(self._dtype.newbyteorder("<")).tobytes())

    @classmethod
    def load(cls, path) -> "IVFFlatIndex":
        """read a VQIVFFL1 file; every range is checked here, before anything can reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError("truncated index header")
            magic, metric, dim, nlist, dtype, n = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError("not a VQIVFFL1 file")
            if (metric >= len(_METRIC_NAMES) or dtype >= len(_DTYPES) or not 1 <= nlist <= MAX_NLIST or dim == 0
                    or n >= 1 << 32):
                raise ValueError("corrupt index header")

            def block(count: int, dtype_, what: str) -> np.ndarray:
                dt = np.dtype(dtype_)
                raw = f.read(count * dt.itemsize)
                if len(raw) != count * dt.itemsize:
                    raise ValueError(f"truncated {what}")
                return np.frombuffer(raw, dtype=dt)

            coarse = block(nlist * dim, "<f4", "coarse centroids").reshape(nlist, dim)
            lists = block(n, "<u4", "list ids")
            rows = block(n * dim, _DTYPES[dtype].newbyteorder("<"), "rows").reshape(n, dim)
            if f.read(1):
                raise ValueError("trailing bytes after the rows")
        if n and int(lists.max()) >= nlist:
            raise ValueError(f"corrupt index: a list id is outside [0, {nlist})")
        self = cls(coarse, Distance(_METRIC_NAMES[metric]), _DTYPES[dtype])
        self._lists = lists.astype(np.uint32)
        self._rows = rows.astype(_DTYPES[dtype])
        return self
