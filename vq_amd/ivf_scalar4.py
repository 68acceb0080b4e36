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
from ._ivf_common import IVFEncodedBase, IVFFile, IVFRangeMixin, _check_coarse, _check_distance, _train_coarse
from ._ivf_filter import IVFFilterMixin
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter
from .ivf_scalar import file_quantizer
from .scalar4_index import MAX_LEVELS, _codes_ok, _pad_ok, words_per_row
from .sq import ScalarQuantizer

MAGIC = b"VQIVFS41"


def _check_quantizer(quantizer) -> None:
    if not isinstance(quantizer, ScalarQuantizer):
        raise InvalidParameter("quantizer", f"expected a ScalarQuantizer, got {type(quantizer).__name__}")
    if quantizer.levels > MAX_LEVELS:
        raise InvalidParameter("quantizer", f"levels {quantizer.levels}: a 4-bit index holds at most {MAX_LEVELS}")


class IVFScalar4Index(IVFFilterMixin, IVFRangeMixin, IVFEncodedBase):
    """coarse centroids (nlist, dim) + ScalarQuantizer (levels <= 16) + distance, and the rows added to it as packed
    4-bit codes"""

    def __init__(self, coarse_centroids, quantizer: ScalarQuantizer, distance: Distance | None = None):
        _check_quantizer(quantizer)
        distance = _check_distance(distance)
        coarse = _check_coarse(coarse_centroids)
        self._init_lists(coarse, distance, np.empty((0, words_per_row(coarse.shape[1])), np.uint32))
        self._quantizer = quantizer

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
        return self._host.copy() if self._host is not None else self._ix.packed()

    def codes(self) -> np.ndarray:
        """(n, dim) uint8: every row's codes unpacked, in row order"""
        if self._ix is not None:
            return self._ix.codes()
        if len(self) == 0:
            return np.empty((0, self.dim), np.uint8)
        return ScalarQuantizer.unpack4_batch(self._host, self.dim)

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

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and codes (n, dim) uint8, each <= 15 (codes >= levels are legal);
        returns the new row ids.  A refused add leaves the index as it was."""
        lid, c = self._add_front(list_ids, codes, "codes", self.dim)
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        _codes_ok(c)
        return self._append(lid, np.ascontiguousarray(c), "add_codes", ScalarQuantizer.pack4_codes)

    def add_packed(self, list_ids, words) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and packed words (n, ceil(dim / 8)) uint32 in
        ``ScalarQuantizer.pack4_codes``' layout, pad nibbles zero; returns the new row ids"""
        lid, w = self._add_front(list_ids, words, "words", self.words)
        if w.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {w.dtype}")
        if not _pad_ok(w, self.dim):
            raise InvalidParameter("words", f"a row has a pad nibble (dimension >= {self.dim}) set")
        return self._append(lid, np.ascontiguousarray(w))

    _UPLOAD, _READ_BACK = "add_packed", "packed"

    def _new_handle(self) -> "_lib.IVFSQ4":
        q = self._quantizer
        return _lib.IVFSQ4(self._coarse, q._min, q._max, q.levels, self._distance.metric)

    # -- file -------------------------------------------------------------------------------
    _HEADER, _MAGICS = struct.Struct("<8sIIIffIQ"), (MAGIC,)

    def _header(self) -> tuple:
        q = self._quantizer
        return MAGIC, self._distance.metric, self.dim, self.nlist, q._min, q._max, q.levels, len(self)

    @classmethod
    def _file(cls, magic, metric, dim, nlist, mn, mx, levels, n) -> IVFFile:
        quantizer = file_quantizer(metric, dim, nlist, n, mn, mx, levels)
        if levels > MAX_LEVELS:
            raise ValueError(f"corrupt index header: levels {levels}: a 4-bit index holds at most {MAX_LEVELS}")

        def check(words):
            if not _pad_ok(words, dim):
                raise ValueError(f"corrupt index: a row has a pad nibble (dimension >= {dim}) set")

        return IVFFile(dim, nlist, n, ("<u4", words_per_row(dim), "words"),
                       lambda coarse: cls(coarse, quantizer, Distance(METRIC_NAMES[metric])), check=check)
