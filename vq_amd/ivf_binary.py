"""``IVFBinaryIndex`` -- an inverted file over packed BQ bits: a query computes the Hamming distance to the rows of its
nearest coarse centroids' lists only, and a row costs one bit per dimension.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_ivfbin_*, vq_amd/csrc/k_ivfbin.hip): a
``BinaryQuantizer(threshold, low, high)`` fixes the bit rules of ``BinaryIndex`` (x >= threshold for f32 rows and
queries, c >= high for u8 codes; row i / dimension t in word ``i * W + t // 32``, bit ``t % 32``, pad bits zero).
``distance`` is the metric of the reported distance (squared Euclidean, Euclidean or Manhattan -- the default, as
``BinaryIndex``; cosine is refused as there); ``coarse_distance`` the metric lists are probed under and rows are
assigned under in ``add`` (any of the five, default Euclidean).  ``P(q)`` is ``FlatIndex(coarse,
coarse_distance).search(q, nprobe)`` for the float32 query -- it is never binarised for probing --, ``S(q)`` the rows
whose list is in ``P(q)``, ``H(q, i) = popcount(bits(q) xor words[i])``, ``D(q, i)`` ``BinaryIndex``'s reported distance
for ``H`` and the result the ``topk`` rows of ``S(q)`` by ``(D, row id)`` ascending, which is ``(H, row id)``.  With
``nprobe == nlist`` the result equals ``BinaryIndex.from_packed(words, dim, quantizer, distance).search`` -- indices,
and distances as uint32 bits.  Slots past ``|S(q)|`` hold id ``0xFFFFFFFF`` and distance ``+inf``.
``hamming_range_search`` returns every row of ``S(q)`` with ``H(q, i) <= radius`` instead, in ascending row id; with
``nprobe == nlist`` it equals ``BinaryIndex.hamming_range_search``.  ``filtered_search`` and
``filtered_hamming_range_search`` answer both over the allowed rows of the probed lists (``IVFBinaryFilterMixin``;
DESIGN.md section 24).  Constructing,
``add_packed``, ``add_codes``, saving and loading need no GPU; ``add`` and ``add_rows`` pack on the device; the device
state is built by the first probe or search and follows every later add.

File layout (little endian), in the manner of ivf_scalar.py's:

    0   8   magic  b"VQIVFBN1"
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan)
    12  4   u32    coarse metric (0 .. 4: the three, cosine, cosine_unclamped)
    16  4   u32    dim (1..8192)
    20  4   u32    nlist
    24  4   f32    threshold
    28  4   u32    low  (0..255)
    32  4   u32    high (0..255)
    36  8   u64    n
    44  ..  f32    coarse centroids [nlist][dim]
    ..  ..  u32    list ids         [n]           (row order)
    ..  ..  u32    words            [n][ceil(dim / 32)]
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._binary_filter import IVFBinaryFilterMixin
from ._ivf_common import MAX_NLIST, IVFEncodedBase, IVFFile, _check_coarse, _check_distance, _train_coarse
from ._resident_common import DEFAULT_MAX_RESULTS, _hamming_radii, _max_results, _nq
from .binary import MAX_DIM, _check_params, _pad_ok, pack_bits, words_per_row
from .bq import BinaryQuantizer
from .distance import METRIC_NAMES, Distance
from .errors import InvalidParameter

MAGIC = b"VQIVFBN1"


class IVFBinaryIndex(IVFBinaryFilterMixin, IVFEncodedBase):
    """coarse centroids (nlist, dim) + BinaryQuantizer (default ``BinaryQuantizer(0.0)``) + distance (default Manhattan)
    + coarse_distance (default Euclidean), and the rows added to it as packed words"""

    def __init__(self, coarse_centroids, quantizer: BinaryQuantizer | None = None, distance: Distance | None = None,
                 coarse_distance: Distance | None = None):
        if quantizer is None:
            quantizer = BinaryQuantizer(0.0)
        if distance is None:
            distance = Distance.manhattan()
        coarse_distance = _check_distance(coarse_distance)
        coarse = _check_coarse(coarse_centroids)
        _check_params(coarse.shape[1], quantizer, distance)
        self._init_lists(coarse, distance, np.empty((0, words_per_row(coarse.shape[1])), np.uint32))
        self._coarse_distance = coarse_distance
        self._quantizer = quantizer

    # -- shape ------------------------------------------------------------------------------
    @property
    def quantizer(self) -> BinaryQuantizer:
        return self._quantizer

    @property
    def coarse_distance(self) -> Distance:
        """the metric lists are probed under, and rows assigned under in `add`"""
        return self._coarse_distance

    def packed(self) -> np.ndarray:
        """(n, ceil(dim / 32)) uint32: every row's words, in row order"""
        return self._stored()

    def __repr__(self) -> str:
        return (f"IVFBinaryIndex(n={len(self)}, nlist={self.nlist}, dim={self.dim}, quantizer={self._quantizer!r}, "
                f"distance={self._distance!r}, coarse_distance={self._coarse_distance!r})")

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, quantizer: BinaryQuantizer | None = None, max_iters: int = 10, distance: Distance | None = None,
              coarse_distance: Distance | None = None, seed: int = 42) -> "IVFBinaryIndex":
        """fit the coarse quantizer on X (k-means of whole rows under coarse_distance, as IVFFlatIndex.train); the binary
        quantizer is given, not trained; the index holds no rows yet (add them with `add`, which packs them)"""
        coarse_distance = _check_distance(coarse_distance)
        if quantizer is not None and not isinstance(quantizer, BinaryQuantizer):
            raise InvalidParameter("quantizer", f"expected a BinaryQuantizer, got {type(quantizer).__name__}")
        return cls(_train_coarse(X, nlist, max_iters, coarse_distance, seed), quantizer, distance, coarse_distance)

    def _assign_metric(self) -> int:
        return self._coarse_distance.metric

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and BQ codes (n, dim) uint8 (bit = code >= high); returns the new
        row ids"""
        lid, c = self._add_front(list_ids, codes, "codes", self.dim)
        if c.dtype != np.uint8:
            raise InvalidParameter("codes", f"dtype must be uint8, got {c.dtype}")
        return self._append(lid, np.ascontiguousarray(c), "add_codes", lambda c: pack_bits(c >= np.uint8(self._quantizer.high)))

    def add_packed(self, list_ids, words) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and packed words (n, ceil(dim / 32)) uint32 in the index layout, pad
        bits zero; returns the new row ids"""
        lid, w = self._add_front(list_ids, words, "words", words_per_row(self.dim))
        if w.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {w.dtype}")
        if not _pad_ok(w, self.dim):
            raise InvalidParameter("words", f"a row has a pad bit (dimension >= {self.dim}) set")
        return self._append(lid, np.ascontiguousarray(w))

    _UPLOAD, _READ_BACK = "add_packed", "packed"

    def _new_handle(self) -> "_lib.IVFBin":
        q = self._quantizer
        return _lib.IVFBin(self._coarse, q.threshold, q.low, q.high, self._distance.metric, self._coarse_distance.metric)

    # -- range search ----------------------------------------------------------------------
    def hamming_range_search(self, queries, radius, nprobe: int = 8, max_results: int = DEFAULT_MAX_RESULTS):
        """every row of the nprobe nearest lists within `radius` bits of each query: row i is a hit of query q iff its
        list is probed and H(q, i) <= radius[q] (`BinaryIndex.hamming_range_search`'s rule and radii).  Returns (lims
        uint64 (nq + 1,), idx uint32 (total,), dist float32 (total,)): the hits of query q are idx[lims[q]:lims[q + 1]],
        in ascending row id, dist the distance `search` reports.  With nprobe == nlist the result equals
        ``BinaryIndex.from_packed(words, ...).hamming_range_search``.  More than `max_results` hits in all: FfiError
        (ERR_UNSUPPORTED)."""
        q = self._queries(queries)
        r = _hamming_radii(radius, q.shape[0])
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._handle().hamming_range_search(q, p, r, m).read()

    def hamming_range_search_device(self, dev_queries: int, nq: int, radius, nprobe: int = 8,
                                    max_results: int = DEFAULT_MAX_RESULTS) -> "_lib.RangeResult":
        """`hamming_range_search` with the queries [nq][dim] f32 at a device pointer (4-byte aligned) and the result left
        on the device: a RangeResult (.total, .lims, .device_pointers(), .read()).  Returns when the result is complete."""
        n_q = _nq(nq)
        r = _hamming_radii(radius, n_q)
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        return self._handle().hamming_range_search_device(int(dev_queries), n_q, p, r, m)

    # -- file -------------------------------------------------------------------------------
    _HEADER, _MAGICS = struct.Struct("<8sIIIIfIIQ"), (MAGIC,)

    def _header(self) -> tuple:
        q = self._quantizer
        return (MAGIC, self._distance.metric, self._coarse_distance.metric, self.dim, self.nlist, np.float32(q.threshold), q.low,
                q.high, len(self))

    @classmethod
    def _file(cls, magic, metric, cmetric, dim, nlist, thr, low, high, n) -> IVFFile:
        if (metric > _lib.MANHATTAN or cmetric >= len(METRIC_NAMES) or not 1 <= nlist <= MAX_NLIST or not 1 <= dim <= MAX_DIM
                or n >= 1 << 32 or low > 255 or high > 255):
            raise ValueError("corrupt index header")
        try:
            quantizer = BinaryQuantizer(float(thr), low, high)  # the reference's own checks
        except (InvalidParameter, ValueError, OverflowError) as e:
            raise ValueError(f"corrupt index header: {e}") from None

        def check(words):
            if not _pad_ok(words, dim):
                raise ValueError(f"corrupt index: a row has a pad bit (dimension >= {dim}) set")

        return IVFFile(dim, nlist, n, ("<u4", words_per_row(dim), "words"),
                       lambda coarse: cls(coarse, quantizer, Distance(METRIC_NAMES[metric]), Distance(METRIC_NAMES[cmetric])),
                       check=check)
