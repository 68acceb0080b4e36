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
from ._ivf_common import (PAD_ID, IVFFile, IVFIndexBase, IVFRangeMixin, _check_coarse, _check_distance,  # noqa: F401
                          _train_coarse, sizes_ok)  # (PAD_ID: re-exported)
from ._ivf_filter import IVFFilterMixin
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter

MAGIC = b"VQIVFFL1"
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
        coarse = _check_coarse(coarse_centroids)
        self._dtype = _row_dtype(dtype)
        self._init_lists(coarse, distance, np.empty((0, coarse.shape[1]), self._dtype))

    # -- shape ------------------------------------------------------------------------------
    @property
    def dtype(self) -> np.dtype:
        return self._dtype

    @property
    def rows(self) -> np.ndarray:
        """(n, dim): every row as stored, in row order"""
        return self._host

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
        lid, r = self._add_shape(list_ids, rows, "rows", self.dim)
        if r.dtype.kind != "f":
            raise InvalidParameter("rows", f"must be floating point, got {r.dtype}")
        lid = self._add_lists(lid, "rows")
        with np.errstate(over="ignore"):
            r = np.ascontiguousarray(r, dtype=self._dtype)
        return self._append(lid, r)

    def _new_handle(self) -> "_lib.IVFFlat":
        return _lib.IVFFlat(self._coarse, self._distance.metric, self._dtype)

    # -- search -----------------------------------------------------------------------------
    def search(self, queries, topk: int = 10, nprobe: int = 8, allowed=None):
        """(nq, dim) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first; slots
        past the probed rows hold 0xFFFFFFFF / +inf.  `allowed`: a row mask (IVFFilterMixin) -- the nearest among the
        allowed rows of the probed lists only"""
        return super().search(queries, topk, nprobe, allowed=allowed)

    # -- file -------------------------------------------------------------------------------
    _HEADER, _MAGICS = struct.Struct("<8sIIIIQ"), (MAGIC,)

    def _header(self) -> tuple:
        return MAGIC, self._distance.metric, self.dim, self.nlist, _DTYPES.index(self._dtype), len(self)

    @classmethod
    def _file(cls, magic, metric, dim, nlist, dtype, n) -> IVFFile:
        if metric >= len(METRIC_NAMES) or dtype >= len(_DTYPES) or not sizes_ok(dim, nlist, n):
            raise ValueError("corrupt index header")
        return IVFFile(dim, nlist, n, (_DTYPES[dtype].newbyteorder("<"), dim, "rows"),
                       lambda coarse: cls(coarse, Distance(METRIC_NAMES[metric]), _DTYPES[dtype]))
