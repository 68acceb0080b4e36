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
from ._resident_common import ExactResidentIndex, _check_distance, check_file_rows, read_index_file, write_index_file
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter
from .sq import ScalarQuantizer

MAGIC = b"VQSQIDX1"
_HEADER = struct.Struct("<8sQIIffI")  # magic, n, d, metric, min, max, levels


def file_quantizer(metric: int, dim: int, n: int, mn: float, mx: float, levels: int) -> ScalarQuantizer:
    """the checks of the fields that the files of ``ScalarIndex`` and ``Scalar4Index`` share; their quantizer"""
    if metric >= len(METRIC_NAMES):
        raise InvalidParameter("distance", f"unknown metric id {metric}")
    if dim < 1:
        raise InvalidParameter("dim", "must be at least 1")
    check_file_rows(n)
    return ScalarQuantizer(mn, mx, levels)  # the reference's own checks


class ScalarIndex(ExactResidentIndex):
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
        distance = _check_distance(distance, Distance.euclidean())
        self._set_source(a, "rows" if rows else "codes", distance)
        self._rows = rows
        self._quantizer = quantizer

    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    def __repr__(self) -> str:
        return f"ScalarIndex(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, distance={self._distance!r})"

    def _make_handle(self) -> "_lib.SQIndex":
        q = self._quantizer
        return _lib.SQIndex(self._src, self._rows, self._n, self._dim, q._min, q._max, q.levels, self._distance.metric)

    def _add_form(self):
        return "add_rows", np.float32, ()  # float32 rows, encoded on the device as the constructor encodes them

    def add_codes(self, codes) -> np.ndarray:
        """append u8 SQ codes (b, dim) as they are (``from_codes``'s form); returns their ids uint32 (b,)"""
        a = self._added(codes, np.uint8, "codes")
        return self._append("add_codes", a, a.shape[0])

    def add_codes_device(self, dev_codes: int, n: int) -> np.ndarray:
        """``add_codes`` with the codes [n][dim] at a device pointer; returns their ids"""
        return self._append_device("add_codes_device", dev_codes, n)

    def codes(self) -> np.ndarray:
        """the codes, uint8 (n, d): the caller's for an index built from codes and not yet searched, else from the device"""
        if self._ix is None and not self._rows:
            return self._src.copy()
        return self._index().codes()

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        write_index_file(path, _HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, q._min, q._max, q.levels),
                         self.codes())

    @classmethod
    def load(cls, path) -> "ScalarIndex":
        """read a VQSQIDX1 file; every field is checked here, before anything can reach the device"""
        def fields(n, dim, metric, mn, mx, levels):
            quantizer = file_quantizer(metric, dim, n, mn, mx, levels)
            return n, dim, np.uint8, "codes", lambda codes: cls.from_codes(codes, quantizer, Distance(METRIC_NAMES[metric]))

        return read_index_file(path, _HEADER, MAGIC, "scalar index", fields)
