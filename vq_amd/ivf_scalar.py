"""``IVFScalarIndex`` -- an inverted file over SQ codes: a query computes the exact distance to the dequantized rows of its
nearest coarse centroids' lists only, and a row costs one byte per dimension.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_ivfsq_*, vq_amd/csrc/k_ivfsq.hip): a
``ScalarQuantizer(min, max, levels)`` fixes ``v(c) = min + float32(c) * step`` for every byte value (codes >= levels
included); ``P(q)`` is ``FlatIndex(coarse, distance).search(q, nprobe)``, ``S(q)`` the rows whose list is in ``P(q)``,
``D(q, i) = Distance.compute(q, v(codes[i]))`` bit for bit, and the result the ``topk`` rows of ``S(q)`` by ``(D, row id)``
ascending with NaN last.  So every result equals ``IVFFlatIndex(coarse, distance)`` over
``quantizer.dequantize_batch(codes)`` in the same lists -- indices, and distances as uint32 bits -- and with
``nprobe == nlist`` ``ScalarIndex.from_codes(codes, quantizer, distance).search``.  Slots past ``|S(q)|`` hold id
``0xFFFFFFFF`` and distance ``+inf``.  Any of the five metrics.  Constructing, ``add_codes``, saving and loading need no
GPU; ``add`` and ``add_rows`` encode on the device; the device state is built by the first probe or search and follows
every later add.

File layout (little endian), in the manner of ivf_flat.py's:

    0   8   magic  b"VQIVFSQ1"
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped)
    12  4   u32    dim
    16  4   u32    nlist
    20  4   f32    min
    24  4   f32    max
    28  4   u32    levels (2..256)
    32  8   u64    n
    40  ..  f32    coarse centroids [nlist][dim]
    ..  ..  u32    list ids         [n]           (row order)
    ..  ..  u8     codes            [n][dim]
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._ivf_common import (MAX_NLIST, IVFIndexBase, IVFRangeMixin, _Reader, _check_coarse, _check_distance, _check_file_lists,
                          _train_coarse)
from ._ivf_filter import IVFFilterMixin
from .distance import Distance
from .errors import DimensionMismatch, InvalidParameter
from .sq import ScalarQuantizer

MAGIC = b"VQIVFSQ1"
_HEADER = struct.Struct("<8sIIIffIQ")
_METRIC_NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]


class IVFScalarIndex(IVFFilterMixin, IVFRangeMixin, IVFIndexBase):
    """coarse centroids (nlist, dim) + ScalarQuantizer + distance, and the rows added to it as codes"""

    def __init__(self, coarse_centroids, quantizer: ScalarQuantizer, distance: Distance | None = None):
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        distance = _check_distance(distance)
        self._init_lists(_check_coarse(coarse_centroids), distance)
        self._quantizer = quantizer
        self._host_codes = np.empty((0, self.dim), np.uint8)  # until the handle exists: it then holds the only copy

    # -- shape ------------------------------------------------------------------------------
    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    @property
    def codes(self) -> np.ndarray:
        """(n, dim) uint8: every row's codes, in row order"""
        return self._host_codes if self._ix is None else self._ix.codes()

    def __repr__(self) -> str:
        return (f"IVFScalarIndex(n={len(self)}, nlist={self.nlist}, dim={self.dim}, quantizer={self._quantizer!r}, "
                f"distance={self._distance!r})")

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, quantizer: ScalarQuantizer, max_iters: int = 10, distance: Distance | None = None,
              seed: int = 42) -> "IVFScalarIndex":
        """fit the coarse quantizer on X (k-means of whole rows, as IVFFlatIndex.train); the scalar quantizer is given,
        not trained; the index holds no rows yet (add them with `add`, which encodes them)"""
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        distance = distance if distance is not None else Distance.euclidean()
        return cls(_train_coarse(X, nlist, max_iters, distance, seed), quantizer, distance)

    def _check_add(self, list_ids, a, what: str):
        lid = np.asarray(list_ids)
        a = np.asarray(a)
        if lid.ndim != 1:
            raise InvalidParameter("list_ids", "must be a 1D array (n,)")
        if a.ndim != 2:
            raise InvalidParameter(what, f"must have shape (n, {self.dim})")
        if a.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, a.shape[1])
        if a.shape[0] != lid.shape[0]:
            raise DimensionMismatch(lid.shape[0], a.shape[0])
        self._check_list_ids(lid)
        self._check_room(lid.shape[0], what)
        return np.ascontiguousarray(lid, dtype=np.uint32), a

    def add_rows(self, list_ids, rows) -> np.ndarray:
        """encode rows (n, dim) floating point, as float32, on the device (the codes of quantizer.quantize_batch) and
        append the codes into the lists list_ids (n,) < nlist; returns the new row ids"""
        lid, r = self._check_add(list_ids, rows, "rows")
        if r.dtype.kind != "f":
            raise InvalidParameter("rows", f"must be floating point, got {r.dtype}")
        if lid.size:
            with np.errstate(over="ignore"):
                self._handle().add_rows(lid, np.ascontiguousarray(r, dtype=np.float32))
        return self._appended(lid)

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and codes (n, dim) uint8 (every byte value is legal); returns the
        new row ids"""
        lid, c = self._check_add(list_ids, codes, "codes")
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        c = np.ascontiguousarray(c)
        if self._ix is not None:
            if lid.size:
                self._ix.add_codes(lid, c)
        else:
            self._host_codes = np.concatenate([self._host_codes, c])
        return self._appended(lid)

    def _removed(self, kept: np.ndarray) -> None:
        if self._ix is None:  # (else the handle holds the only copy)
            self._host_codes = self._host_codes[kept]

    def _handle(self) -> "_lib.IVFSQ":
        if self._ix is None:
            q = self._quantizer
            ix = _lib.IVFSQ(self._coarse, q._min, q._max, q.levels, self._distance.metric)
            if len(self):
                ix.add_codes(self._lists, self._host_codes)
            self._ix = ix
            self._host_codes = None
        return self._ix

    def close(self) -> None:
        """release the handle and its device state (the next probe or search builds it again); the codes stay"""
        if self._ix is not None:
            self._host_codes = self._ix.codes()
            super().close()

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._distance.metric, self.dim, self.nlist, q._min, q._max, q.levels, len(self)))
            f.write(self._coarse.astype("<f4").tobytes())
            f.write(self._lists.astype("<u4").tobytes())
            f.write(np.ascontiguousarray(self.codes, dtype=np.uint8).tobytes())

    @classmethod
    def load(cls, path) -> "IVFScalarIndex":
        """read a VQIVFSQ1 file; every range is checked here, before anything can reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError("truncated index header")
            magic, metric, dim, nlist, mn, mx, levels, n = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError("not a VQIVFSQ1 file")
            if metric >= len(_METRIC_NAMES) or not 1 <= nlist <= MAX_NLIST or dim == 0 or n >= 1 << 32:
                raise ValueError("corrupt index header")
            try:
                quantizer = ScalarQuantizer(mn, mx, levels)  # the reference's own checks
            except InvalidParameter as e:
                raise ValueError(f"corrupt index header: {e}") from None
            r = _Reader(f)
            coarse = r.block(nlist * dim, "<f4", "coarse centroids").reshape(nlist, dim)
            lists = r.lists(n)
            codes = r.block(n * dim, np.uint8, "codes").reshape(n, dim)
            r.end("codes")
        _check_file_lists(lists, nlist)
        self = cls(coarse, quantizer, Distance(_METRIC_NAMES[metric]))
        self._lists = lists.astype(np.uint32)
        self._host_codes = codes.copy()
        return self
