"""``IVFScalar4Index`` -- an inverted file over SQ codes of at most 16 levels at four bits a dimension: ``IVFScalarIndex``
at half the bytes a row, ``Scalar4Index`` over the probed lists only.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_ivfsq4_*, vq_amd/csrc/k_ivfsq4.hip): a
``ScalarQuantizer(min, max, levels)`` with ``levels <= 16`` fixes ``v(c) = min + float32(c) * step`` for every nibble
value 0..15 (codes >= levels included); ``P(q)`` is ``IVFFlatIndex.probe`` exactly, ``S(q)`` the rows whose list is in
``P(q)``, ``D(q, i) = Distance.compute(q, v(codes[i]))`` bit for bit, and the result the ``topk`` rows of ``S(q)`` by
``(D, row id)`` ascending with NaN last.  So every result -- indices, and distances as uint32 bits -- equals
``IVFScalarIndex`` over the same codes in the same lists, ``IVFFlatIndex(coarse, distance)`` over
``quantizer.dequantize_batch(codes)`` in the same lists, and with ``nprobe == nlist``
``Scalar4Index.from_codes(codes, quantizer, distance)`` on the same call.  Slots past ``|S(q)|`` hold id ``0xFFFFFFFF``
and distance ``+inf``.  Any of the five metrics.  Layout of a row: ``ScalarQuantizer.pack4_codes``.  Constructing,
``add_codes``, ``add_packed``, saving and loading need no GPU; ``add`` and ``add_rows`` encode and pack on the device;
the device state is built by the first probe or search and follows every later add.

File layout (little endian), ivf_scalar.py's header under another magic:

    0   8   magic  b"VQIVFS41"
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan, 3 cosine, 4 cosine_unclamped)
    12  4   u32    dim
    16  4   u32    nlist
    20  4   f32    min
    24  4   f32    max
    28  4   u32    levels (2..16)
    32  8   u64    n
    40  ..  f32    coarse centroids [nlist][dim]
    ..  ..  u32    list ids         [n]           (row order)
    ..  ..  u32    words            [n][W]        W = ceil(dim / 8), pad nibbles zero
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
from .scalar4_index import MAX_LEVELS, _codes_ok, _pad_ok, words_per_row
from .sq import ScalarQuantizer

MAGIC = b"VQIVFS41"
_HEADER = struct.Struct("<8sIIIffIQ")
_METRIC_NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]


def _check_quantizer(quantizer) -> None:
    if not isinstance(quantizer, ScalarQuantizer):
        raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
    if quantizer.levels > MAX_LEVELS:
        raise InvalidParameter("quantizer", f"levels {quantizer.levels}: a 4-bit index holds at most {MAX_LEVELS}")


class IVFScalar4Index(IVFFilterMixin, IVFRangeMixin, IVFIndexBase):
    """coarse centroids (nlist, dim) + ScalarQuantizer (levels <= 16) + distance, and the rows added to it as packed
    4-bit codes"""

    def __init__(self, coarse_centroids, quantizer: ScalarQuantizer, distance: Distance | None = None):
        _check_quantizer(quantizer)
        distance = _check_distance(distance)
        self._init_lists(_check_coarse(coarse_centroids), distance)
        self._quantizer = quantizer
        self._host_words = np.empty((0, self.words), np.uint32)  # until the handle exists: it then holds the only copy

    # -- shape ------------------------------------------------------------------------------
    @property
    def quantizer(self) -> ScalarQuantizer:
        return self._quantizer

    @property
    def words(self) -> int:
        """uint32 words of a row: ceil(dim / 8)"""
        return words_per_row(self.dim)

    def packed(self) -> np.ndarray:
        """(n, ceil(dim / 8)) uint32: every row's packed codes, in row order"""
        return self._host_words.copy() if self._ix is None else self._ix.packed()

    def codes(self) -> np.ndarray:
        """(n, dim) uint8: every row's codes unpacked, in row order"""
        if self._ix is not None:
            return self._ix.codes()
        if len(self) == 0:
            return np.empty((0, self.dim), np.uint8)
        return ScalarQuantizer.unpack4_batch(self._host_words, self.dim)

    def __repr__(self) -> str:
        return (f"IVFScalar4Index(n={len(self)}, nlist={self.nlist}, dim={self.dim}, quantizer={self._quantizer!r}, "
                f"distance={self._distance!r})")

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, quantizer: ScalarQuantizer, max_iters: int = 10, distance: Distance | None = None,
              seed: int = 42) -> "IVFScalar4Index":
        """fit the coarse quantizer on X (k-means of whole rows, as IVFFlatIndex.train); the scalar quantizer is given,
        not trained; the index holds no rows yet (add them with `add`, which encodes and packs them)"""
        _check_quantizer(quantizer)
        distance = distance if distance is not None else Distance.euclidean()
        return cls(_train_coarse(X, nlist, max_iters, distance, seed), quantizer, distance)

    def _check_add(self, list_ids, a, what: str, width: int):
        lid = np.asarray(list_ids)
        a = np.asarray(a)
        if lid.ndim != 1:
            raise InvalidParameter("list_ids", "must be a 1D array (n,)")
        if a.ndim != 2:
            raise InvalidParameter(what, f"must have shape (n, {width})")
        if a.shape[1] != width:
            raise DimensionMismatch(width, a.shape[1])
        if a.shape[0] != lid.shape[0]:
            raise DimensionMismatch(lid.shape[0], a.shape[0])
        self._check_list_ids(lid)
        self._check_room(lid.shape[0], what)
        return np.ascontiguousarray(lid, dtype=np.uint32), a

    def add_rows(self, list_ids, rows) -> np.ndarray:
        """encode rows (n, dim) floating point, as float32, on the device (the codes of quantizer.quantize_batch), pack
        them there and append the words into the lists list_ids (n,) < nlist; returns the new row ids"""
        lid, r = self._check_add(list_ids, rows, "rows", self.dim)
        if r.dtype.kind != "f":
            raise InvalidParameter("rows", f"must be floating point, got {r.dtype}")
        if lid.size:
            with np.errstate(over="ignore"):
                self._handle().add_rows(lid, np.ascontiguousarray(r, dtype=np.float32))
        return self._appended(lid)

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and codes (n, dim) uint8, each <= 15 (codes >= levels are legal);
        returns the new row ids.  A refused add leaves the index as it was."""
        lid, c = self._check_add(list_ids, codes, "codes", self.dim)
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        _codes_ok(c)
        c = np.ascontiguousarray(c)
        if self._ix is not None:
            if lid.size:
                self._ix.add_codes(lid, c)
        else:
            self._host_words = np.concatenate([self._host_words, ScalarQuantizer.pack4_codes(c)])
        return self._appended(lid)

    def add_packed(self, list_ids, words) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and packed words (n, ceil(dim / 8)) uint32 in
        ``ScalarQuantizer.pack4_codes``' layout, pad nibbles zero; returns the new row ids"""
        lid, w = self._check_add(list_ids, words, "words", self.words)
        if w.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {w.dtype}")
        if not _pad_ok(w, self.dim):
            raise InvalidParameter("words", f"a row has a pad nibble (dimension >= {self.dim}) set")
        w = np.ascontiguousarray(w)
        if self._ix is not None:
            if lid.size:
                self._ix.add_packed(lid, w)
        else:
            self._host_words = np.concatenate([self._host_words, w])
        return self._appended(lid)

    def _removed(self, kept: np.ndarray) -> None:
        if self._ix is None:  # (else the handle holds the only copy)
            self._host_words = self._host_words[kept]

    def _handle(self) -> "_lib.IVFSQ4":
        if self._ix is None:
            q = self._quantizer
            ix = _lib.IVFSQ4(self._coarse, q._min, q._max, q.levels, self._distance.metric)
            if len(self):
                ix.add_packed(self._lists, self._host_words)
            self._ix = ix
            self._host_words = None
        return self._ix

    def close(self) -> None:
        """release the handle and its device state (the next probe or search builds it again); the words stay"""
        if self._ix is not None:
            self._host_words = self._ix.packed()
            super().close()

    # -- file -------------------------------------------------------------------------------
    def save(self, path) -> None:
        q = self._quantizer
        with open(path, "wb") as f:
            f.write(_HEADER.pack(MAGIC, self._distance.metric, self.dim, self.nlist, q._min, q._max, q.levels, len(self)))
            f.write(self._coarse.astype("<f4").tobytes())
            f.write(self._lists.astype("<u4").tobytes())
            f.write(np.ascontiguousarray(self.packed(), dtype="<u4").tobytes())

    @classmethod
    def load(cls, path) -> "IVFScalar4Index":
        """read a VQIVFS41 file; every field, the pad nibbles and the list ids are checked here, before anything can
        reach the device"""
        with open(path, "rb") as f:
            head = f.read(_HEADER.size)
            if len(head) != _HEADER.size:
                raise ValueError("truncated index header")
            magic, metric, dim, nlist, mn, mx, levels, n = _HEADER.unpack(head)
            if magic != MAGIC:
                raise ValueError("not a VQIVFS41 file")
            if metric >= len(_METRIC_NAMES) or not 1 <= nlist <= MAX_NLIST or dim == 0 or n >= 1 << 32:
                raise ValueError("corrupt index header")
            try:
                quantizer = ScalarQuantizer(mn, mx, levels)  # the reference's own checks
            except InvalidParameter as e:
                raise ValueError(f"corrupt index header: {e}") from None
            if levels > MAX_LEVELS:
                raise ValueError(f"corrupt index header: levels {levels}: a 4-bit index holds at most {MAX_LEVELS}")
            w = words_per_row(dim)
            r = _Reader(f)
            coarse = r.block(nlist * dim, "<f4", "coarse centroids").reshape(nlist, dim)
            lists = r.lists(n)
            words = r.block(n * w, "<u4", "words").reshape(n, w)
            r.end("words")
        _check_file_lists(lists, nlist)
        words = words.astype(np.uint32)
        if not _pad_ok(words, dim):
            raise ValueError(f"corrupt index: a row has a pad nibble (dimension >= {dim}) set")
        self = cls(coarse, quantizer, Distance(_METRIC_NAMES[metric]))
        self._lists = lists.astype(np.uint32)
        self._host_words = words
        return self
