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
from ._resident_common import ExactResidentIndex, _check_distance, _count
from .distance import Distance
from .errors import DimensionMismatch, InvalidData, InvalidParameter
from .sq import ScalarQuantizer

MAGIC = b"VQSQ4IX1"
MAX_LEVELS = 16
_HEADER = struct.Struct("<8sQIIffI")  # magic, n, d, metric, min, max, levels
_METRIC_NAMES = {_lib.SQUARED_EUCLIDEAN: "squared_euclidean", _lib.EUCLIDEAN: "euclidean", _lib.MANHATTAN: "manhattan",
                 _lib.COSINE: "cosine", _lib.COSINE_UNCLAMPED: "cosine_unclamped"}


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


class Scalar4Index(ExactResidentIndex):
    """Exact search over `rows` (n, d) float32, stored as the 4-bit codes of `quantizer` (``levels <= 16``), against
    float32 queries under `distance` (any metric, cosine included; default Euclidean)."""

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
        a = words if isinstance(words, np.ndarray) else np.asarray(words)
        if a.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {a.dtype}")
        d = _count(dim, "dim")
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, words)")
        if d < 1:
            raise InvalidParameter("dim", f"must be at least 1, got {d}")
        if a.shape[1] != words_per_row(d):
            raise DimensionMismatch(words_per_row(d), a.shape[1])
        if not _pad_ok(a, d):
            raise InvalidParameter("words", f"a row has a pad nibble (dimension >= {d}) set")
        self = cls.__new__(cls)
        self._setup(a, _lib.SQ4_PACKED, quantizer, distance, dim=d)
        return self

    def _setup(self, a: np.ndarray, kind: int, quantizer, distance, dim: int | None = None) -> None:
        if not isinstance(quantizer, ScalarQuantizer):
            raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
        if quantizer.levels > MAX_LEVELS:
            raise InvalidParameter("quantizer", f"levels {quantizer.levels}: a 4-bit index holds at most {MAX_LEVELS}")
        distance = _check_distance(distance, Distance.euclidean())
        self._set_source(a, "words" if kind == _lib.SQ4_PACKED else "codes" if kind == _lib.SQ4_U8 else "rows", distance, dim)
        self._kind = kind
        self._quantizer = quantizer

    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    def __repr__(self) -> str:
        return f"Scalar4Index(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, distance={self._distance!r})"

    def _make_handle(self) -> "_lib.SQ4Index":
        q = self._quantizer
        return _lib.SQ4Index(self._src, self._kind, self._n, self._dim, q._min, q._max, q.levels, self._distance.metric)

    def _add_form(self):
        return "add", np.float32, (_lib.SQ4_F32,)  # float32 rows, encoded and packed on the device as the constructor's

    def add_codes(self, codes) -> np.ndarray:
        """append u8 SQ codes (b, dim), each <= 15 (``from_codes``'s form); returns their ids uint32 (b,)"""
        a = self._added(codes, np.uint8, "codes")
        _codes_ok(a)
        return self._append("add", a, a.shape[0], _lib.SQ4_U8)

    def add_packed(self, words) -> np.ndarray:
        """append packed rows uint32 (b, ceil(dim / 8)) in the index layout, pad nibbles zero (``from_packed``'s form);
        returns their ids uint32 (b,)"""
        a = self._added(words, np.uint32, "words", words_per_row(self._dim))
        if not _pad_ok(a, self._dim):
            raise InvalidParameter("words", f"a row has a pad nibble (dimension >= {self._dim}) set")
        return self._append("add", a, a.shape[0], _lib.SQ4_PACKED)

    def add_codes_device(self, dev_codes: int, n: int) -> np.ndarray:
        """``add_codes`` with the codes [n][dim] at a device pointer; a code above 15 is an FfiError
        (ERR_INVALID_INPUT) that leaves the index as it was.  Returns their ids."""
        return self._append_device("add_device", dev_codes, n, _lib.SQ4_U8)

    def add_packed_device(self, dev_words: int, n: int) -> np.ndarray:
        """``add_packed`` with the words [n][ceil(dim / 8)] at a device pointer (4-byte aligned); a pad nibble set is an
        FfiError (ERR_INVALID_INPUT) that leaves the index as it was.  Returns their ids."""
        return self._append_device("add_device", dev_words, n, _lib.SQ4_PACKED)

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
        words = self.packed()
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, q._min, q._max, q.levels))
            f.write(np.ascontiguousarray(words, dtype="<u4").tobytes())

    @classmethod
    def load(cls, path) -> "Scalar4Index":
        """read a VQSQ4IX1 file; every field is checked here, before anything can reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise InvalidData("truncated 4-bit scalar index header")
            magic, n, dim, metric, mn, mx, levels = _HEADER.unpack(head)
            if magic != MAGIC:
                raise InvalidData("not a VQSQ4IX1 file")
            if metric not in _METRIC_NAMES:
                raise InvalidParameter("distance", f"unknown metric id {metric}")
            if dim < 1:
                raise InvalidParameter("dim", "must be at least 1")
            if not 1 <= n < 1 << 32:
                raise InvalidData(f"row count {n} is outside [1, 2^32)")
            quantizer = ScalarQuantizer(mn, mx, levels)  # the reference's own checks
            if levels > MAX_LEVELS:
                raise InvalidParameter("quantizer", f"levels {levels}: a 4-bit index holds at most {MAX_LEVELS}")
            w = words_per_row(dim)
            raw = f.read(n * w * 4)
            if len(raw) != n * w * 4:
                raise InvalidData("truncated packed rows")
            if f.read(1):
                raise InvalidData("trailing bytes after the packed rows")
        words = np.frombuffer(raw, dtype="<u4").astype(np.uint32).reshape(n, w)
        if not _pad_ok(words, dim):
            raise InvalidData(f"a row has a pad nibble (dimension >= {dim}) set")
        return cls.from_packed(words, dim, quantizer, Distance(_METRIC_NAMES[metric]))
