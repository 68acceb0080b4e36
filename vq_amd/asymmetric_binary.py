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
from ._resident_common import ExactResidentIndex, _check_distance, read_index_file, write_index_file
from .binary import PackedBitsSource, _check_dim
from .bq import BinaryQuantizer
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter

MAGIC = b"VQABINX1"
_HEADER = struct.Struct("<8sQIIfII")  # magic, n, d, metric, threshold, low, high


class AsymmetricBinaryIndex(PackedBitsSource, ExactResidentIndex):
    """Exact search over `rows` (n, d) float32, stored as the bits of `quantizer` (default ``BinaryQuantizer(0.0)``),
    against float32 queries under `distance` (any metric, cosine included; default Euclidean)."""

    def _setup(self, a: np.ndarray, kind: int, quantizer, distance, dim: int | None = None) -> None:
        quantizer = BinaryQuantizer(0.0) if quantizer is None else quantizer
        if not isinstance(quantizer, BinaryQuantizer):
            raise InvalidParameter("quantizer", f"expected a BinaryQuantizer, got {type(quantizer).__name__}")
        distance = _check_distance(distance, Distance.euclidean())
        self._quantizer = quantizer
        self._set_source(a, "words" if kind == _lib.BINARY_PACKED else "codes" if kind == _lib.BINARY_U8 else "rows", distance, dim)
        self._kind = kind

    def _check_dim(self, d: int, what: str) -> None:
        _check_dim(d)

    def __repr__(self) -> str:
        return (f"AsymmetricBinaryIndex(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, "
                f"distance={self._distance!r})")

    def _make_handle(self) -> "_lib.ABin":
        q = self._quantizer
        return _lib.ABin(self._src, self._kind, self._n, self._dim, q.threshold, q.low, q.high, self._distance.metric)

    def packed(self) -> np.ndarray:
        """the packed rows, uint32 (n, ceil(dim / 32)): the caller's for an index built ``from_packed`` and not yet
        searched, else from the device"""
        if self._ix is None and self._kind == _lib.BINARY_PACKED:
            return self._src.copy()
        return self._index().packed()

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        write_index_file(path, _HEADER.pack(MAGIC, self._n, self._dim, self._distance.metric, np.float32(q.threshold), q.low,
                                            q.high), self._host_words())

    @classmethod
    def load(cls, path) -> "AsymmetricBinaryIndex":
        """read a VQABINX1 file; every field is checked here, before anything can reach the device"""
        def fields(n, dim, metric, thr, low, high):
            if metric >= len(METRIC_NAMES):
                raise InvalidParameter("distance", f"unknown metric id {metric}")
            return cls._file_payload(metric, dim, thr, low, high, n)

        return read_index_file(path, _HEADER, MAGIC, "asymmetric binary index", fields)
