"""``Scalar4Index`` -- exact search, range search and rerank of float32 queries over SQ codes of at most 16 levels kept on
the device at four bits a dimension: the tier between ``ScalarIndex`` (8 bits) and ``AsymmetricBinaryIndex`` (1 bit).

The reference has no search function; the semantics are include/vqhip.h's (vqhip_sq4index_*,
vq_amd/csrc/k_sq4index.hip): a ``ScalarQuantizer(min, max, levels)`` with ``levels <= 16`` fixes the codes on the way in
(``quantize_batch``'s for float32 rows, bit for bit; u8 codes as they are, each <= 15) and ``v(c) = min + float32(c) *
step`` on the way out for every nibble value 0..15, codes >= levels included.  ``D(q, i) = Distance.compute(q,
v(codes[i]))`` bit for bit under any of the five metrics, cosine included; the queries are float32 and never quantized.
Every result equals ``ScalarIndex.from_codes(codes, quantizer, distance)`` and
``FlatIndex(quantizer.dequantize_batch(codes), distance)`` on the same call -- indices, and distances as uint32 bits --
at half of the former's device memory and an eighth of the latter's: n * ceil(d / 8) * 4 bytes, plus 4 n for the row
norms under cosine.  Layout: ``ScalarQuantizer.pack4_codes``.

It serves as a reranker wherever a ``FlatIndex`` does: ``binary_index.search(Q, 10, rerank=sq4, candidates=100)``.

Every argument is checked here before the device is touched; the index goes to the device on the first search (until
then it refers to the caller's array, which must not change in between).  An index built from float32 rows encodes and
packs them on the device and keeps only the words.  ``save`` / ``load`` of an index built ``from_codes`` or
``from_packed`` need no device.

File layout (``save`` / ``load``), little-endian, no padding::

    offset  size     field
    0       8        magic  b"VQSQ4IX1"
    8       8        n      uint64, rows, 1 <= n < 2^32
    16      4        d      uint32, dimensions, >= 1
    20      4        metric uint32, 0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped
    24      4        min    float32
    28      4        max    float32
    32      4        levels uint32, 2..16
    36      n*W*4    words  uint32, row-major, W = ceil(d / 8), pad nibbles zero
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._resident_common import ExactResidentIndex, PackedSourceMixin, _check_distance, read_index_file, write_index_file
from .distance import METRIC_NAMES, Distance
from .errors import InvalidData, InvalidParameter
from .scalar_index import file_quantizer
from .sq import ScalarQuantizer

MAGIC = b"VQSQ4IX1"
MAX_LEVELS = 16
_HEADER = struct.Struct("<8sQIIffI")  # magic, n, d, metric, min, max, levels


def words_per_row(d: int) -> int:
    return (d + 7) // 8


def _pad_ok(words: np.ndarray, d: int) -> bool:
    """no pad nibble (dimension >= d) of packed rows (n, W) is set"""
    if d % 8 == 0 or words.shape[0] == 0:
        return True
    keep = np.uint32((1 << (4 * (d % 8))) - 1)
    return not bool((words[:, -1] & ~keep).any())


def _codes_ok(codes: np.ndarray, what: str = "codes") -> None:
    if codes.size and int(codes.max()) > 15:
        raise InvalidParameter(what, f"a 4-bit code is at most 15, got {int(codes.max())}")


def _packed_dim(d: int) -> None:
    if d < 1:
        raise InvalidParameter("dim", f"must be at least 1, got {d}")


class Scalar4Index(PackedSourceMixin, ExactResidentIndex):
    """Exact search over `rows` (n, d) float32, stored as the 4-bit codes of `quantizer` (``levels <= 16``), against
    float32 queries under `distance` (any metric, cosine included; default Euclidean)."""

    _F32, _U8, _PACKED, _PAD = _lib.SQ4_F32, _lib.SQ4_U8, _lib.SQ4_PACKED, "nibble"
    _words, _pad_ok = staticmethod(words_per_row), staticmethod(_pad_ok)
    _packed_dim, _codes_ok = staticmethod(_packed_dim), staticmethod(_codes_ok)

    def __init__(self, rows, quantizer: ScalarQuantizer, distance: Distance | None = None):
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype != np.float32:
            raise InvalidParameter("rows", f"dtype must be float32, got {a.dtype}")
        self._setup(a, _lib.SQ4_F32, quantizer, distance)

    @classmethod
    def from_codes(cls, codes, quantizer: ScalarQuantizer, distance: Distance | None = None) -> "Scalar4Index":
        """u8 SQ codes (n, d), e.g. ``quantizer.quantize_batch(rows)``; every value 0..15 is legal"""
        a = codes if isinstance(codes, np.ndarray) else np.asarray(codes)
        if a.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {a.dtype}")
        _codes_ok(a)
        self = cls.__new__(cls)
        self._setup(a, _lib.SQ4_U8, quantizer, distance)
        return self

    @classmethod
    def from_packed(cls, words, dim: int, quantizer: ScalarQuantizer, distance: Distance | None = None) -> "Scalar4Index":
        """uint32 (n, ceil(dim / 8)) packed rows in ``ScalarQuantizer.pack4_codes``' layout, pad nibbles zero"""
        return cls._from_packed(words, dim, quantizer, distance)

    def _setup(self, a: np.ndarray, kind: int, quantizer, distance, dim: int | None = None) -> None:
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        if quantizer.levels > MAX_LEVELS:
            raise InvalidParameter("quantizer", f"levels {quantizer.levels}: a 4-bit index holds at most {MAX_LEVELS}")
        distance = _check_distance(distance, Distance.euclidean())
        self._set_source(a, "words" if kind == _lib.SQ4_PACKED else "codes" if kind == _lib.SQ4_U8 else "rows", distance, dim)
        self._kind = kind
        self._quantizer = quantizer

    def __repr__(self) -> str:
        return f"Scalar4Index(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, distance={self._distance!r})"

    def _make_handle(self) -> "_lib.SQ4Index":
        q = self._quantizer
        return _lib.SQ4Index(self._src, self._kind, self._n, self._dim, q._min, q._max, q.levels, self._distance.metric)

    def add_codes_device(self, dev_codes: int, n: int) -> np.ndarray:
        """``add_codes`` with the codes [n][dim] at a device pointer; a code above 15 is an FfiError
        (ERR_INVALID_INPUT) that leaves the index as it was.  Returns their ids."""
        return self._append_device("add_device", dev_codes, n, _lib.SQ4_U8)

    def packed(self) -> np.ndarray:
        """the packed rows, uint32 (n, ceil(dim / 8)): from the caller's array for an index built ``from_packed`` or
        ``from_codes`` and not yet searched, else from the device"""
        if self._ix is None and self._kind == _lib.SQ4_PACKED:
            return self._src.copy()
        if self._ix is None and self._kind == _lib.SQ4_U8:
            return ScalarQuantizer.pack4_codes(self._src)
        return self._index().packed()

    def codes(self) -> np.ndarray:
        """the codes unpacked, uint8 (n, dim)"""
        if self._ix is None and self._kind == _lib.SQ4_U8:
            return self._src.copy()
        return ScalarQuantizer.unpack4_batch(self.packed(), self._dim)

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        write_index_file(path, _HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, q._min, q._max, q.levels),
                         self.packed())

    @classmethod
    def load(cls, path) -> "Scalar4Index":
        """read a VQSQ4IX1 file; every field is checked here, before anything can reach the device"""
        def fields(n, dim, metric, mn, mx, levels):
            quantizer = file_quantizer(metric, dim, n, mn, mx, levels)
            if levels > MAX_LEVELS:
                raise InvalidParameter("quantizer", f"levels {levels}: a 4-bit index holds at most {MAX_LEVELS}")

            def finish(words):
                if not _pad_ok(words, dim):
                    raise InvalidData(f"a row has a pad nibble (dimension >= {dim}) set")
                return cls.from_packed(words, dim, quantizer, Distance(METRIC_NAMES[metric]))

            return n, words_per_row(dim), "<u4", "packed rows", finish

        return read_index_file(path, _HEADER, MAGIC, "4-bit scalar index", fields)
