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
from ._ivf_common import IVFEncodedBase, IVFFile, IVFRangeMixin, _check_coarse, _check_distance, _train_coarse, sizes_ok
from ._ivf_filter import IVFFilterMixin
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter
from .sq import ScalarQuantizer

MAGIC = b"VQIVFSQ1"


def file_quantizer(metric: int, dim: int, nlist: int, n: int, mn: float, mx: float, levels: int) -> ScalarQuantizer:
    """the checks of the header fields that the files of ``IVFScalarIndex`` and ``IVFScalar4Index`` share; their quantizer"""
    if metric >= len(METRIC_NAMES) or not sizes_ok(dim, nlist, n):
        raise ValueError("corrupt index header")
    try:
        return ScalarQuantizer(mn, mx, levels)  # the reference's own checks
    except InvalidParameter as e:
        raise ValueError(f"corrupt index header: {e}") from None


class IVFScalarIndex(IVFFilterMixin, IVFRangeMixin, IVFEncodedBase):
    """coarse centroids (nlist, dim) + ScalarQuantizer + distance, and the rows added to it as codes"""

    def __init__(self, coarse_centroids, quantizer: ScalarQuantizer, distance: Distance | None = None):
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        distance = _check_distance(distance)
        coarse = _check_coarse(coarse_centroids)
        self._init_lists(coarse, distance, np.empty((0, coarse.shape[1]), np.uint8))
        self._quantizer = quantizer

    # -- shape ------------------------------------------------------------------------------
    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    @property
    def codes(self) -> np.ndarray:
        """(n, dim) uint8: every row's codes, in row order"""
        return self._stored()

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

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and codes (n, dim) uint8 (every byte value is legal); returns the
        new row ids"""
        lid, c = self._add_front(list_ids, codes, "codes", self.dim)
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        return self._append(lid, np.ascontiguousarray(c))

    _UPLOAD, _READ_BACK = "add_codes", "codes"

    def _new_handle(self) -> "_lib.IVFSQ":
        q = self._quantizer
        return _lib.IVFSQ(self._coarse, q._min, q._max, q.levels, self._distance.metric)

    # -- file -------------------------------------------------------------------------------
    _HEADER, _MAGICS = struct.Struct("<8sIIIffIQ"), (MAGIC,)

    def _header(self) -> tuple:
        q = self._quantizer
        return MAGIC, self._distance.metric, self.dim, self.nlist, q._min, q._max, q.levels, len(self)

    @classmethod
    def _file(cls, magic, metric, dim, nlist, mn, mx, levels, n) -> IVFFile:
        quantizer = file_quantizer(metric, dim, nlist, n, mn, mx, levels)
        return IVFFile(dim, nlist, n, (np.uint8, dim, "codes"), lambda coarse: cls(coarse, quantizer, Distance(METRIC_NAMES[metric])))
