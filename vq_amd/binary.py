"""``BinaryIndex`` -- exact Hamming top-k search over BQ codes packed 32 to a word on the device.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_binary_*, vq_amd/csrc/k_binary.hip):
a ``BinaryQuantizer(threshold, low, high)`` fixes the bit rule (x >= threshold for f32 rows and queries, c >= high for
u8 codes), row i / dimension t sits in word ``i * W + t // 32``, bit ``t % 32`` (``W = ceil(d / 32)``, pad bits zero),
and ``D(q, i) = Distance.compute(bq.dequantize(bq.quantize(q)), bq.dequantize(code_i))`` bit for bit for squared
Euclidean, Euclidean and Manhattan -- a function of the Hamming distance alone, read from a table the library builds.
Cosine is refused.  The result per query is the ``topk`` rows by ``(D, row id)`` ascending, ties to the lower row.
``hamming_range_search`` answers the other query, every row within ``radius`` bits, as the CSR triple of
``FlatIndex.range_search``.  ``filtered_search`` and ``filtered_hamming_range_search`` answer both
over the rows a mask allows (``BinaryFilterMixin``).

Every argument is checked here before the device is touched; the index goes to the device on the first search (until
then it refers to the caller's array, which must not change in between).  ``save`` / ``load`` need no device.
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._binary_filter import BinaryFilterMixin
from ._resident_common import (DEFAULT_MAX_RESULTS, PackedSourceMixin, ResidentIndex, _hamming_radii, _max_results, _nq,
                               check_file_rows, read_index_file, write_index_file)
from .bq import BinaryQuantizer
from .distance import METRIC_NAMES, Distance
from .errors import InvalidData, InvalidParameter
from .flat import adc_then_rerank

MAGIC = b"VQBINIX1"
_HEADER = struct.Struct("<8sIIfIIQ")  # magic, metric, dim, threshold, low, high, n
MAX_DIM = 8192
_METRICS = (_lib.SQUARED_EUCLIDEAN, _lib.EUCLIDEAN, _lib.MANHATTAN)


def words_per_row(dim: int) -> int:
    return (int(dim) + 31) // 32


def pack_bits(bits: np.ndarray) -> np.ndarray:
    """bool / 0-1 array (n, d) -> uint32 (n, W), the layout of the index (host numpy)"""
    b = np.asarray(bits).astype(bool)
    n, d = b.shape
    w = words_per_row(d)
    padded = np.zeros((n, 32 * w), bool)
    padded[:, :d] = b
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, w)


def _pad_ok(words: np.ndarray, dim: int) -> bool:
    if dim % 32 == 0 or words.shape[0] == 0:
        return True
    mask = np.uint32((1 << (dim % 32)) - 1)
    return not bool((words[:, -1] & ~mask).any())


def _check_dim(dim: int) -> None:
    if not 1 <= dim <= MAX_DIM:
        raise InvalidParameter("dim", f"must be between 1 and {MAX_DIM}, got {dim}")


def _check_params(dim: int, quantizer, distance) -> None:
    if not isinstance(quantizer, BinaryQuantizer):
        raise InvalidParameter("quantizer", f"expected a BinaryQuantizer, got {type(quantizer).__name__}")
    if not isinstance(distance, Distance):
        raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
    if distance.metric not in _METRICS:
        raise InvalidParameter("distance", f"{distance.name()} is not a function of the Hamming distance alone; "
                                           "use squared_euclidean, euclidean or manhattan")
    _check_dim(dim)


class PackedBitsSource(PackedSourceMixin):
    """the rows of ``BinaryIndex`` and ``AsymmetricBinaryIndex``, one bit a dimension: float32 rows (bit = x >=
    threshold), u8 BQ codes (bit = code >= high) or the packed words, at construction and in every add; the words on the
    host for ``save``; and the fields the two files share.  `quantizer` defaults to ``BinaryQuantizer(0.0)``."""

    _F32, _U8, _PACKED, _PAD = _lib.BINARY_F32, _lib.BINARY_U8, _lib.BINARY_PACKED, "bit"
    _words, _pad_ok, _packed_dim = staticmethod(words_per_row), staticmethod(_pad_ok), staticmethod(_check_dim)

    def __init__(self, rows, quantizer: BinaryQuantizer | None = None, distance: Distance | None = None):
        a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
        if a.dtype != np.float32:
            raise InvalidParameter("rows", f"dtype must be float32, got {a.dtype}")
        self._setup(a, _lib.BINARY_F32, quantizer, distance)

    @classmethod
    def from_codes(cls, codes, quantizer: BinaryQuantizer | None = None, distance: Distance | None = None):
        """u8 BQ codes (n, d), e.g. ``quantizer.quantize_batch(rows)``; bit = code >= high"""
        a = codes if isinstance(codes, np.ndarray) else np.asarray(codes)
        if a.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {a.dtype}")
        self = cls.__new__(cls)
        self._setup(a, _lib.BINARY_U8, quantizer, distance)
        return self

    @classmethod
    def from_packed(cls, words, dim: int, quantizer: BinaryQuantizer | None = None, distance: Distance | None = None):
        """uint32 (n, ceil(dim / 32)) packed rows in the index layout, pad bits zero.  The asymmetric twin of a
        ``BinaryIndex`` b is ``AsymmetricBinaryIndex.from_packed(b.packed(), b.dim, b.quantizer, distance)``."""
        return cls._from_packed(words, dim, quantizer, distance)

    def _host_words(self) -> np.ndarray:
        if self._ix is not None:
            return self._ix.packed()
        if self._kind == _lib.BINARY_PACKED:
            return self._src
        if self._kind == _lib.BINARY_U8:
            return pack_bits(self._src >= np.uint8(self._quantizer.high))
        return pack_bits(self._src >= np.float32(self._quantizer.threshold))

    @classmethod
    def _file_payload(cls, metric: int, dim: int, thr, low: int, high: int, n: int):
        """the checks of a file's fields behind the metric's, and its payload (`read_index_file`)"""
        _check_dim(dim)
        check_file_rows(n)
        if low > 255 or high > 255:
            raise InvalidParameter("low/high", f"must fit in u8, got {low} / {high}")
        quantizer = BinaryQuantizer(float(thr), low, high)  # the reference's own checks

        def finish(words):
            if not _pad_ok(words, dim):
                raise InvalidData(f"a row has a pad bit (dimension >= {dim}) set")
            return cls.from_packed(words, dim, quantizer, Distance(METRIC_NAMES[metric]))

        return n, words_per_row(dim), "<u4", "packed rows", finish


class BinaryIndex(BinaryFilterMixin, PackedBitsSource, ResidentIndex):
    """Exact Hamming top-k over rows binarised by `quantizer` (default ``BinaryQuantizer(0.0)``) under `distance`
    (default Manhattan: with the default quantizer, D is the Hamming count)."""

    def _setup(self, a: np.ndarray, kind: int, quantizer, distance, dim: int | None = None) -> None:
        self._quantizer = BinaryQuantizer(0.0) if quantizer is None else quantizer
        self._set_source(a, "rows", Distance.manhattan() if distance is None else distance, dim)
        self._kind = kind

    def _check_dim(self, d: int, what: str) -> None:
        _check_params(d, self._quantizer, self._distance)

    def __repr__(self) -> str:
        return f"BinaryIndex(n={self._n}, dim={self._dim}, quantizer={self._quantizer!r}, distance={self._distance!r})"

    def _make_handle(self) -> "_lib.Binary":
        q = self._quantizer
        return _lib.Binary(self._src, self._kind, self._n, self._dim, q.threshold, q.low, q.high, self._distance.metric)

    def search(self, queries, topk: int = 10, *, rerank=None, candidates=None):
        """(nq, d) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first.
        rerank: a FlatIndex, a ScalarIndex or an AsymmetricBinaryIndex (the asymmetric twin over the same bits:
        ``AsymmetricBinaryIndex.from_packed(self.packed(), self.dim, self.quantizer, distance)``) over the same rows -- the
        binary search gives `candidates` per query
        (default 4 topk, at most 1024 and n), that index reranks them exactly in its own metric."""
        q = self._queries(queries)
        k = self._topk(topk)
        if rerank is not None:
            return adc_then_rerank(self.search, self._n, self._dim, q, k, rerank, candidates)
        if candidates is not None:
            raise InvalidParameter("candidates", "only with rerank")
        return self._search(q, k)

    def hamming_range_search(self, queries, radius, max_results: int = DEFAULT_MAX_RESULTS):
        """every row within `radius` bits of each query: row i is a hit of query q iff H(q, i) <= radius[q], H being the
        Hamming distance `search` selects on (the query binarised by the quantizer's rule).  `radius` is a non-negative
        integer below 2^32 or nq of them; a radius >= dim returns every row, 0 the exact bit matches.  Returns (lims
        uint64 (nq + 1,), idx uint32 (total,), dist float32 (total,)): the hits of query q are idx[lims[q]:lims[q + 1]],
        in ascending row id, and dist is the distance `search` reports for the row.  More than `max_results` hits in
        all: FfiError (ERR_UNSUPPORTED).  (Named for its unit: a `range_search` takes a radius in the distance.)"""
        q = self._queries(queries)
        r = _hamming_radii(radius, q.shape[0])
        m = _max_results(max_results)
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._index().hamming_range_search(q, r, m).read()

    def hamming_range_search_device(self, dev_queries: int, nq: int, radius,
                                    max_results: int = DEFAULT_MAX_RESULTS) -> "_lib.RangeResult":
        """`hamming_range_search` with the queries [nq][d] f32 at a device pointer (4-byte aligned) and the result left on
        the device: a RangeResult (.total, .lims, .device_pointers(), .read()).  Returns when the result is complete."""
        n_q = _nq(nq)
        r = _hamming_radii(radius, n_q)
        m = _max_results(max_results)
        return self._index().hamming_range_search_device(int(dev_queries), n_q, r, m)

    def packed(self) -> np.ndarray:
        """the packed rows, uint32 (n, ceil(dim / 32)), from the device"""
        return self._index().packed()

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        write_index_file(path, _HEADER.pack(MAGIC, self._distance.metric, self._dim, np.float32(q.threshold), q.low, q.high,
                                            self._n), self._host_words())

    @classmethod
    def load(cls, path) -> "BinaryIndex":
        """read a VQBINIX1 file; every field is checked here, before anything can reach the device"""
        def fields(metric, dim, thr, low, high, n):
            if metric not in _METRICS:
                raise InvalidParameter("distance", f"metric id {metric} is not squared_euclidean, euclidean or manhattan")
            return cls._file_payload(metric, dim, thr, low, high, n)

        return read_index_file(path, _HEADER, MAGIC, "binary index", fields)
