"""``AsymmetricBinaryIndex`` -- exact search, range search and rerank of float32 queries over BQ bits packed 32 to a word
on the device: the asymmetric form of the 1-bit tier.

``BinaryIndex`` binarises the query and ranks by the Hamming distance.  This index keeps the same bits and nothing else
(n * ceil(d / 32) * 4 bytes, plus 4 n for the row norms under cosine), leaves the query in float32 and computes its exact
distance to the *dequantized* row.  The reference has no search function; the semantics are include/vqhip.h's
(vqhip_abin_*, vq_amd/csrc/k_abin.hip): a ``BinaryQuantizer(threshold, low, high)`` fixes the bit rule on the way in
(x >= threshold for f32 rows, c >= high for u8 codes, as in ``BinaryIndex``, whose word layout this is) and the decode
rule on the way out, ``v(bit) = float32(high) if bit else float32(low)``, and ``D(q, i) = Distance.compute(q,
v(bits[i]))`` bit for bit under any of the five metrics, cosine included.  Every result equals
``FlatIndex(quantizer.dequantize_batch(bits), distance)`` and ``ScalarIndex.from_codes(bits as 0/1 bytes,
ScalarQuantizer(low, high, 2), distance)`` on the same call -- indices, and distances as uint32 bits.

It is a reranker for Hamming short lists at 1/32 of the float32 rows' memory:
``binary_index.search(Q, 10, rerank=abin, candidates=100)``.

Every argument is checked here before the device is touched; the index goes to the device on the first search (until
then it refers to the caller's array, which must not change in between).  ``save`` / ``load`` of an index built
``from_packed`` need no device.

File layout (``save`` / ``load``), little-endian, no padding::

    offset  size     field
    0       8        magic     b"VQABINX1"
    8       8        n         uint64, rows, 1 <= n < 2^32
    16      4        d         uint32, dimensions, 1..8192
    20      4        metric    uint32, 0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped
    24      4        threshold float32
    28      4        low       uint32, 0..255
    32      4        high      uint32, 0..255
    36      n*W*4    words     uint32, row-major, W = ceil(d / 32), pad bits zero
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._resident_common import ExactResidentIndex, _check_distance, _count
from .binary import MAX_DIM, _pad_ok, pack_bits, words_per_row
from .bq import BinaryQuantizer
from .distance import Distance
from .errors import DimensionMismatch, InvalidData, InvalidParameter

MAGIC = b"VQABINX1"
_HEADER = struct.Struct("<8sQIIfII")  # magic, n, d, metric, threshold, low, high
_METRIC_NAMES = {_lib.SQUARED_EUCLIDEAN: "squared_euclidean", _lib.EUCLIDEAN: "euclidean", _lib.MANHATTAN: "manhattan",
                 _lib.COSINE: "cosine", _lib.COSINE_UNCLAMPED: "cosine_unclamped"}


class AsymmetricBinaryIndex(ExactResidentIndex):
    """Exact search over `rows` (n, d) float32, stored as the bits of `quantizer` (default ``BinaryQuantizer(0.0)``),
    against float32 queries under `distance` (any metric, cosine included; default Euclidean)."""

    def __init__(self, rows, quantizer: BinaryQuantizer | None = None, distance: Distance | None = None):
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype != np.float32:
            raise InvalidParameter("rows", f"dtype must be float32, got {a.dtype}")
        self._setup(a, _lib.BINARY_F32, quantizer, distance)

    @classmethod
    def from_codes(cls, codes, quantizer: BinaryQuantizer | None = None,
                   distance: Distance | None = None) -> "AsymmetricBinaryIndex":
        """u8 BQ codes (n, d), e.g. ``quantizer.quantize_batch(rows)``; bit = code >= high"""
        a = codes if isinstance(codes, np.ndarray) else np.asarray(codes)
        if a.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {a.dtype}")
        self = cls.__new__(cls)
        self._setup(a, _lib.BINARY_U8, quantizer, distance)
        return self

    @classmethod
    def from_packed(cls, words, dim: int, quantizer: BinaryQuantizer | None = None,
                    distance: Distance | None = None) -> "AsymmetricBinaryIndex":
        """uint32 (n, ceil(dim / 32)) packed rows in ``BinaryIndex``'s layout, pad bits zero.  The asymmetric twin of a
        ``BinaryIndex`` b is ``from_packed(b.packed(), b.dim, b.quantizer, distance)``."""
        a = words if isinstance(words, np.ndarray) else np.asarray(words)
        if a.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {a.dtype}")
        d = _count(dim, "dim")
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, words)")
        if not 1 <= d <= MAX_DIM:
            raise InvalidParameter("dim", f"must be between 1 and {MAX_DIM}, got {d}")
        if a.shape[1] != words_per_row(d):
            raise DimensionMismatch(words_per_row(d), a.shape[1])
        if not _pad_ok(a, d):
            raise InvalidParameter("words", f"a row has a pad bit (dimension >= {d}) set")
        self = cls.__new__(cls)
        self._setup(a, _lib.BINARY_PACKED, quantizer, distance, dim=d)
        return self

    def _setup(self, a: np.ndarray, kind: int, quantizer, distance, dim: int | None = None) -> None:
        quantizer = BinaryQuantizer(0.0) if quantizer is None else quantizer
        if not isinstance(quantizer, BinaryQuantizer):
            raise InvalidParameter("quantizer", f"expected a BinaryQuantizer, got {type(quantizer).__name__}")
        distance = _check_distance(distance, Distance.euclidean())
        self._quantizer = quantizer
        self._set_source(a, "words" if kind == _lib.BINARY_PACKED else "codes" if kind == _lib.BINARY_U8 else "rows", distance, dim)
        self._kind = kind

    def _check_dim(self, d: int, what: str) -> None:
        if not 1 <= d <= MAX_DIM:
            raise InvalidParameter("dim", f"must be between 1 and {MAX_DIM}, got {d}")

    @property
    def quantizer(self) -> BinaryQuantizer:
        return self._quantizer

    def __repr__(self) -> str:
        return (f"AsymmetricBinaryIndex(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, "
                f"distance={self._distance!r})")

    def _make_handle(self) -> "_lib.ABin":
        q = self._quantizer
        return _lib.ABin(self._src, self._kind, self._n, self._dim, q.threshold, q.low, q.high, self._distance.metric)

    def _add_form(self):
        return "add", np.float32, (_lib.BINARY_F32,)  # float32 rows, binarised on the device by the quantizer's rule

    def add_codes(self, codes) -> np.ndarray:
        """append u8 BQ codes (b, dim), bit = code >= high (``from_codes``'s form); returns their ids uint32 (b,)"""
        a = self._added(codes, np.uint8, "codes")
        return self._append("add", a, a.shape[0], _lib.BINARY_U8)

    def add_packed(self, words) -> np.ndarray:
        """append packed rows uint32 (b, ceil(dim / 32)) in the index layout, pad bits zero (``from_packed``'s form);
        returns their ids uint32 (b,)"""
        a = self._added(words, np.uint32, "words", words_per_row(self._dim))
        if not _pad_ok(a, self._dim):
            raise InvalidParameter("words", f"a row has a pad bit (dimension >= {self._dim}) set")
        return self._append("add", a, a.shape[0], _lib.BINARY_PACKED)

    def add_packed_device(self, dev_words: int, n: int) -> np.ndarray:
        """``add_packed`` with the words [n][ceil(dim / 32)] at a device pointer (4-byte aligned); a pad bit set is an
        FfiError (ERR_INVALID_INPUT) that leaves the index as it was.  Returns their ids."""
        return self._append_device("add_device", dev_words, n, _lib.BINARY_PACKED)

    def packed(self) -> np.ndarray:
        """the packed rows, uint32 (n, ceil(dim / 32)): the caller's for an index built ``from_packed`` and not yet
        searched, else from the device"""
        if self._ix is None and self._kind == _lib.BINARY_PACKED:
            return self._src.copy()
        return self._index().packed()

    def _host_words(self) -> np.ndarray:
        if self._ix is not None:
            return self._ix.packed()
        if self._kind == _lib.BINARY_PACKED:
            return self._src
        if self._kind == _lib.BINARY_U8:
            return pack_bits(self._src >= np.uint8(self._quantizer.high))
        return pack_bits(self._src >= np.float32(self._quantizer.threshold))

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, np.float32(q.threshold), q.low, q.high))
            f.write(np.ascontiguousarray(self._host_words(), dtype="<u4").tobytes())

    @classmethod
    def load(cls, path) -> "AsymmetricBinaryIndex":
        """read a VQABINX1 file; every field is checked here, before anything can reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise InvalidData("truncated asymmetric binary index header")
            magic, n, dim, metric, thr, low, high = _HEADER.unpack(head)
            if magic != MAGIC:
                raise InvalidData("not a VQABINX1 file")
            if metric not in _METRIC_NAMES:
                raise InvalidParameter("distance", f"unknown metric id {metric}")
            if not 1 <= dim <= MAX_DIM:
                raise InvalidParameter("dim", f"must be between 1 and {MAX_DIM}, got {dim}")
            if not 1 <= n < 1 << 32:
                raise InvalidData(f"row count {n} is outside [1, 2^32)")
            if low > 255 or high > 255:
                raise InvalidParameter("low/high", f"must fit in u8, got {low} / {high}")
            quantizer = BinaryQuantizer(float(thr), low, high)  # the reference's own checks
            w = words_per_row(dim)
            raw = f.read(n * w * 4)
            if len(raw) != n * w * 4:
                raise InvalidData("truncated packed rows")
            if f.read(1):
                raise InvalidData("trailing bytes after the packed rows")
        words = np.frombuffer(raw, dtype="<u4").astype(np.uint32).reshape(n, w)
        if not _pad_ok(words, dim):
            raise InvalidData(f"a row has a pad bit (dimension >= {dim}) set")
        return cls.from_packed(words, dim, quantizer, Distance(_METRIC_NAMES[metric]))
