"""``IVFPQIndex`` -- an inverted-file index over PQ codes: a query scans only the lists of its nearest coarse centroids.

The reference has no search function; the semantics are include/vqhip.h's (vqhip_ivfpq_*, vq_amd/csrc/k_ivf.hip):
``P(q)`` is ``FlatIndex(coarse, distance).search(q, nprobe)``, ``S(q)`` the rows whose list is in ``P(q)``, and the result
the ``topk`` rows of ``S(q)`` by ``(ADC distance, row id)`` ascending -- with ``nprobe == nlist`` exactly
``PQIndex(codebooks, codes).search``.  Slots past ``|S(q)|`` hold id ``0xFFFFFFFF`` and distance ``+inf``.  By default
non-residual: the codes encode the rows themselves.  ``residual=True`` (IVFADC): a row ``x`` in list ``l`` is stored as the
codes of ``x - C[l]``, and its distance to ``q`` is the ADC distance of those codes to ``r = q - C[l]`` (f32, one rounding
per element); probing, order, ties, NaN and padding are as above.  Constructing, adding codes, saving and loading need
no GPU; the device handle is created by the first probe or search and follows every later add.

File layout (little endian), in the manner of store.py's:

    0   8   magic  b"VQIVFPQ1" (non-residual) or b"VQIVFRP1" (residual)
    8   4   u32    metric (0 squared_euclidean, 1 euclidean, 2 manhattan)
    12  4   u32    dim
    16  4   u32    nlist
    20  4   u32    m
    24  4   u32    k
    28  4   u32    reserved (0)
    32  8   u64    n
    40  ..  f32    coarse centroids [nlist][dim]
    ..  ..  f32    codebooks        [m][k][dim/m]
    ..  ..  u32    list ids         [n]           (row order)
    ..  ..  u8     codes            [n][m]        (k <= 256; u16 little endian above: the library's code width)
"""
from __future__ import annotations

import struct

import numpy as np

from . import _lib
from ._ivf_common import (MAX_NLIST, MAX_PROBE, MAX_TOPK, PAD_ID, IVFFile, IVFIndexBase,  # noqa: F401  (re-exported)
                          _check_distance, _check_nlist, _coarse_array, _nearest_lists, _train_coarse, sizes_ok)
from ._resident_common import _allowed, _nq
from .distance import METRIC_NAMES, Distance
from .errors import DimensionMismatch, InvalidParameter

MAGIC = b"VQIVFPQ1"
MAGIC_RESIDUAL = b"VQIVFRP1"
MAX_TABLE = 38400  # m * k: one query's ADC table in the LDS (include/vqhip.h)


def _code_dtype(k: int):
    return np.dtype(np.uint8) if k <= 256 else np.dtype("<u2")


def _check_shape(coarse, codebooks, distance):
    """(coarse f32 (nlist, dim), codebooks f32 (m, k, sub_dim)) after the index's checks"""
    _check_distance(distance)
    if distance.metric not in (_lib.SQUARED_EUCLIDEAN, _lib.EUCLIDEAN, _lib.MANHATTAN):
        raise InvalidParameter("distance", "cosine distance is not a sum over subspaces: no ADC form")
    c = _coarse_array(coarse)
    cb = np.ascontiguousarray(codebooks, dtype=np.float32)
    if cb.ndim != 3:
        raise InvalidParameter("codebooks", "must have shape (m, k, sub_dim)")
    nlist, dim = c.shape
    m, k, sd = cb.shape
    _check_nlist(nlist)
    if m == 0 or k == 0 or sd == 0:
        raise InvalidParameter("codebooks", "m, k and sub_dim must be positive")
    if k > 65536:
        raise InvalidParameter("k", "codes are at most two bytes: k <= 65536")
    if m * k > MAX_TABLE:
        raise InvalidParameter("codebooks", f"m * k = {m * k} exceeds the ADC table limit {MAX_TABLE}")
    if dim != m * sd:
        raise DimensionMismatch(m * sd, dim)
    return c, cb


class IVFPQIndex(IVFIndexBase):
    """coarse centroids (nlist, dim) + PQ codebooks (m, k, dim / m) + distance, and the rows added to it"""

    def __init__(self, coarse_centroids, codebooks, distance: Distance | None = None, *, residual: bool = False):
        if not isinstance(residual, (bool, np.bool_)):
            raise InvalidParameter("residual", f"must be a bool, got {type(residual).__name__}")
        distance = distance if distance is not None else Distance.euclidean()
        coarse, self._codebooks = _check_shape(coarse_centroids, codebooks, distance)
        m, k = self._codebooks.shape[:2]
        self._init_lists(coarse, distance, np.empty((0, m), _code_dtype(k)))
        self._residual = bool(residual)

    # -- shape ------------------------------------------------------------------------------
    @property
    def m(self) -> int:
        return self._codebooks.shape[0]

    @property
    def k(self) -> int:
        return self._codebooks.shape[1]

    @property
    def residual(self) -> bool:
        """True: the codes of a row in list l quantise x - C[l]"""
        return self._residual

    @property
    def codebooks(self) -> np.ndarray:
        return self._codebooks

    @property
    def codes(self) -> np.ndarray:
        """(n, m): every row's codes, in row order"""
        return self._host

    def __repr__(self) -> str:
        return (f"IVFPQIndex(n={len(self)}, nlist={self.nlist}, dim={self.dim}, m={self.m}, k={self.k}, "
                f"distance={self._distance!r}" + (", residual=True)" if self._residual else ")"))

    # -- build ------------------------------------------------------------------------------
    @classmethod
    def train(cls, X, nlist: int, m: int, k: int, max_iters: int = 10, distance: Distance | None = None,
              seed: int = 42, residual: bool = False) -> "IVFPQIndex":
        """fit the coarse quantizer (k-means of whole rows: a ProductQuantizer with one subspace of nlist centroids) and
        the PQ codebooks on X -- with residual=True on the residuals X - C[list] of X's rows in their nearest lists; the
        index holds no rows yet (add them with `add`)"""
        from .pq import ProductQuantizer

        if not isinstance(residual, (bool, np.bool_)):
            raise InvalidParameter("residual", f"must be a bool, got {type(residual).__name__}")
        distance = distance if distance is not None else Distance.euclidean()
        coarse = _train_coarse(X, nlist, max_iters, distance, seed)
        if residual:
            X = np.ascontiguousarray(X, dtype=np.float32)
            X = X - coarse[_nearest_lists(coarse, X, distance.metric)]
        cb = ProductQuantizer(X, m, k, max_iters, distance, seed).codebooks
        return cls(coarse, cb, distance, residual=bool(residual))

    def add(self, X) -> np.ndarray:
        """assign each row of X (n, dim) to its nearest coarse centroid (the reference's nearest-centroid rule: a PQ encode
        with one subspace of nlist centroids), encode it with the codebooks, append; returns the new row ids"""
        X = self._add_rows_2d(X)
        if X.shape[0] == 0:
            return np.empty(0, np.uint32)
        lists = _nearest_lists(self._coarse, X, self._distance.metric)
        if self._residual:
            X = X - self._coarse[lists]  # (f32, one rounding per element)
        pq = _lib.PQEncoder(self._codebooks, self._distance.metric)
        try:
            codes, _ = pq.encode(X, want_f16=False)
        finally:
            pq.close()
        return self.add_codes(lists, codes)

    def add_codes(self, list_ids, codes) -> np.ndarray:
        """append rows given as list ids (n,) < nlist and codes (n, m) < k; returns the new row ids"""
        lid, c = self._add_shape(list_ids, codes, "codes", self.m, shape_only=True)
        self._check_list_ids(lid)  # (the halves of _add_lists: the codes' own check stands between them)
        if c.size and (c.dtype.kind not in "iu" or int(c.min()) < 0 or int(c.max()) >= self.k):
            raise InvalidParameter("codes", f"must be integers in [0, {self.k})")
        self._check_room(lid.shape[0], "codes")
        return self._append(np.ascontiguousarray(lid, dtype=np.uint32), np.ascontiguousarray(c, dtype=_code_dtype(self.k)))

    def _new_handle(self) -> "_lib.IVFPQ":
        return _lib.IVFPQ(self._coarse, self._codebooks, self._distance.metric, _lib.IVF_RESIDUAL if self._residual else 0)

    # -- filtered search ----------------------------------------------------------------------
    def masked_search(self, queries, allowed, topk: int = 10, nprobe: int = 8, *, rerank=None, candidates: int | None = None):
        """`search` among the allowed rows only.  allowed: one row mask for the call, a bool array (n,) (True: the row may
        be returned) or its uint32 words (`pack_row_mask`), n being ``len(index)`` at the time of the call.  Probing takes
        no mask: a query scans its nprobe nearest lists whatever they hold, and a query with fewer than `topk` allowed rows
        in them has the slots behind them padded with 0xFFFFFFFF / +inf (`topk` itself stays within 1 .. min(n, 1024)).
        With `rerank`, the mask filters the first stage: the reranker sees allowed rows only."""
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        w = _allowed(allowed, len(self))
        if rerank is not None:
            return self._search_rerank(q, t, p, rerank, candidates, allowed=w)
        if q.shape[0] == 0:
            return np.empty((0, t), np.uint32), np.empty((0, t), np.float32)
        return self._handle().search_masked(q, p, t, w)

    def masked_search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, dev_allowed: int,
                             nprobe: int = 8) -> None:
        """`search_device` among the allowed rows only; `dev_allowed`: the row mask's ceil(n / 32) uint32 words at a device
        pointer (4-byte aligned)"""
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        n_q = _nq(nq)
        if dev_allowed is None:
            raise InvalidParameter("dev_allowed", "must be a device pointer, got None")
        self._handle().search_masked_device(int(dev_queries), n_q, p, t, int(dev_allowed), int(dev_idx), int(dev_dist))

    # -- file -------------------------------------------------------------------------------
    _HEADER, _MAGICS = struct.Struct("<8sIIIIIIQ"), (MAGIC, MAGIC_RESIDUAL)

    def _header(self) -> tuple:
        magic = MAGIC_RESIDUAL if self._residual else MAGIC
        return magic, self._distance.metric, self.dim, self.nlist, self.m, self.k, 0, len(self)

    def _file_extra(self) -> tuple:
        return (self._codebooks,)

    @classmethod
    def _file(cls, magic, metric, dim, nlist, m, k, reserved, n) -> IVFFile:
        if (metric > _lib.MANHATTAN or reserved != 0 or not sizes_ok(dim, nlist, n) or m == 0 or k == 0 or k > 65536
                or m * k > MAX_TABLE or dim % m != 0):
            raise ValueError("corrupt index header")

        def check(codes):
            if n and int(codes.max()) >= k:
                raise ValueError(f"corrupt index: a code is outside [0, {k})")

        return IVFFile(dim, nlist, n, (_code_dtype(k), m, "codes"),
                       lambda coarse, cb: cls(coarse, cb, Distance(METRIC_NAMES[metric]), residual=magic == MAGIC_RESIDUAL),
                       extra=(((m, k, dim // m), "codebooks"),), check=check)
