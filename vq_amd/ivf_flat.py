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
from ._ivf_common import (MAX_NLIST, PAD_ID, IVFIndexBase, IVFRangeMixin, _Reader, _check_coarse, _check_distance,  # noqa: F401
                          _check_file_lists, _train_coarse)  # (PAD_ID: re-exported)
from ._ivf_filter import IVFFilterMixin
from .distance import Distance
from .errors import DimensionMismatch, InvalidParameter

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


class IVFFlatIndex(IVFFilterMixin, IVFRangeMixin, IVFIndexBase):
    """coarse centroids (nlist, dim) + distance + row dtype, and the rows added to it"""

    def __init__(self, coarse_centroids, distance: Distance | None = None, dtype=np.float32):
        distance = _check_distance(distance)
        self._init_lists(_check_coarse(coarse_centroids), distance)
        self._dtype = _row_dtype(dtype)
        self._rows = np.empty((0, self.dim), self._dtype)

    # -- shape ------------------------------------------------------------------------------
    @property
    def dtype(self) -> np.dtype:
        return self._dtype

    @property
    def rows(self) -> np.ndarray:
        """(n, dim): every row as stored, in row order"""
        return self._rows

    def __repr__(self) -> str:
        return (f"IVFFlatIndex(n={len(self)}, nlist={self.nlist}, dim={self.dim}, dtype={self._dtype.name}, "
                f"distance={self._distance!r})")

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, max_iters: int = 10, distance: Distance | None = None, seed: int = 42,
              dtype=np.float32) -> "IVFFlatIndex":
        """fit the coarse quantizer on X (k-means of whole rows: a ProductQuantizer with one subspace of nlist centroids,
        as IVFPQIndex.train); the index holds no rows yet (add them with `add`, rounded to the index's dtype)"""
        distance = distance if distance is not None else Distance.euclidean()
        dt = _row_dtype(dtype)
        return cls(_train_coarse(X, nlist, max_iters, distance, seed), distance, dt)

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
        self._check_list_ids(lid)
        self._check_room(lid.shape[0], "rows")
        lid = np.ascontiguousarray(lid, dtype=np.uint32)
        with np.errstate(over="ignore"):
            r = np.ascontiguousarray(r, dtype=self._dtype)
        if self._ix is not None and lid.size:
            self._ix.add(lid, r)
        self._rows = np.concatenate([self._rows, r])
        return self._appended(lid)

    def _removed(self, kept: np.ndarray) -> None:
        self._rows = self._rows[kept]

    def _handle(self) -> "_lib.IVFFlat":
        if self._ix is None:
            ix = _lib.IVFFlat(self._coarse, self._distance.metric, self._dtype)
            if len(self):
                ix.add(self._lists, self._rows)
            self._ix = ix
        return self._ix

    # -- search -----------------------------------------------------------------------------
    def search(self, queries, topk: int = 10, nprobe: int = 8, allowed=None):
        """(nq, dim) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first; slots
        past the probed rows hold 0xFFFFFFFF / +inf.  `allowed`: a row mask (IVFFilterMixin) -- the nearest among the
        allowed rows of the probed lists only"""
        return super().search(queries, topk, nprobe, allowed=allowed)

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
            r = _Reader(f)
            coarse = r.block(nlist * dim, "<f4", "coarse centroids").reshape(nlist, dim)
            lists = r.lists(n)
            rows = r.block(n * dim, _DTYPES[dtype].newbyteorder("<"), "rows").reshape(n, dim)
            r.end("rows")
        _check_file_lists(lists, nlist)
        self = cls(coarse, Distance(_METRIC_NAMES[metric]), _DTYPES[dtype])
        self._lists = lists.astype(np.uint32)
        self._rows = rows.astype(_DTYPES[dtype])
        return self
