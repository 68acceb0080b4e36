"""What ``IVFPQIndex``, ``IVFFlatIndex``, ``IVFScalarIndex``, ``IVFScalar4Index`` and ``IVFBinaryIndex`` share: the coarse
centroids and list ids, the front of every add, the payload (codes, rows or words) on the host and in the handle, the
checks of queries, ``nprobe`` and ``topk``, probe / search / rerank over the device handle, and the one writer and
reader of the index files.  A subclass keeps the checks of its own stored form, how its handle is made, and the fields
of its file.  ``IVFEncodedBase`` is the base of the three indexes that encode float rows on the device and hand their
payload to the handle.  ``IVFRangeMixin`` adds the range search of the indexes whose distances are exact (not
``IVFPQIndex``)."""
from __future__ import annotations

import math
from typing import Callable, NamedTuple

import numpy as np

from . import _lib
from ._resident_common import DEFAULT_MAX_RESULTS, _count, _max_results, _nq, _radii, pack_row_mask
from .distance import Distance
from .errors import DimensionMismatch, InvalidParameter

MAX_NLIST = 65536
MAX_PROBE = 1024
MAX_TOPK = 1024
PAD_ID = 0xFFFFFFFF


def _nearest_lists(coarse, X, metric: int) -> np.ndarray:
    """(n,) uint32: each row's nearest coarse centroid (the reference's nearest-centroid rule: a PQ encode with one
    subspace of nlist centroids)"""
    enc = _lib.PQEncoder(coarse[None, :, :], metric)
    try:
        lists, _ = enc.encode(X, want_f16=False)
    finally:
        enc.close()
    return np.asarray(lists).reshape(-1).astype(np.uint32)


def _check_distance(distance) -> Distance:
    if distance is None:
        distance = Distance.euclidean()
    if not isinstance(distance, Distance):
        raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
    return distance


def _coarse_array(coarse_centroids) -> np.ndarray:
    c = np.ascontiguousarray(coarse_centroids, dtype=np.float32)
    if c.ndim != 2:
        raise InvalidParameter("coarse_centroids", "must have shape (nlist, dim)")
    return c


def _check_nlist(nlist: int) -> None:
    if not 1 <= nlist <= MAX_NLIST:
        raise InvalidParameter("nlist", f"must be between 1 and {MAX_NLIST}, got {nlist}")


def _check_coarse(coarse_centroids) -> np.ndarray:
    """coarse f32 (nlist, dim) after the checks of an index whose dimension is the centroids' own"""
    c = _coarse_array(coarse_centroids)
    _check_nlist(c.shape[0])
    if c.shape[1] == 0:
        raise InvalidParameter("coarse_centroids", "dimension must be at least 1")
    return c


def _train_coarse(X, nlist: int, max_iters: int, distance: Distance, seed: int) -> np.ndarray:
    """the coarse quantizer: k-means of whole rows (a ProductQuantizer with one subspace of nlist centroids)"""
    from .pq import ProductQuantizer

    return ProductQuantizer(X, 1, nlist, max_iters, distance, seed).codebooks[0]


class IVFFile(NamedTuple):
    """what a subclass reads from a file's header (``_file``): the sizes, the payload block, and how to make the index"""
    dim: int
    nlist: int
    n: int
    payload: tuple  # (dtype in the file, items a row, the block's name)
    make: Callable  # (coarse, *extra blocks) -> the index, empty
    extra: tuple = ()  # blocks between the coarse centroids and the list ids: (shape, name), f32
    check: Callable | None = None  # the payload's own check: raises ValueError


def sizes_ok(dim: int, nlist: int, n: int) -> bool:
    """the header fields that every inverted file has"""
    return 1 <= nlist <= MAX_NLIST and dim >= 1 and n < 1 << 32


def _block(f, shape: tuple, dtype, what: str) -> np.ndarray:
    """a block of an index file in the machine's byte order, checked for truncation"""
    dt = np.dtype(dtype)
    count = math.prod(shape)
    raw = f.read(count * dt.itemsize)
    if len(raw) != count * dt.itemsize:
        raise ValueError(f"truncated {what}")
    return np.frombuffer(raw, dtype=dt).astype(dt.newbyteorder("=")).reshape(shape)


def rerank_hits(q: np.ndarray, hits: np.ndarray, topk: int, rerank):
    """the exact rerank of a first stage that may be short: hits (nq, c) row ids with PAD_ID behind every real one (a
    query whose probed lists, or whose allowed rows, are fewer than c).  A full query is reranked as it is; a short one
    over its real hits, and keeps the padding behind them."""
    nq, c = hits.shape
    idx = np.full((nq, topk), PAD_ID, np.uint32)
    dist = np.full((nq, topk), np.inf, np.float32)
    real = (hits != PAD_ID).sum(axis=1)  # (padding follows every real hit)
    full = real == c
    if full.any():
        idx[full], dist[full] = rerank.rerank(q[full], hits[full], topk)
    for j in np.flatnonzero((real > 0) & ~full):  # a query with fewer hits keeps its padding
        r = int(real[j])
        t = min(topk, r)
        idx[j, :t], dist[j, :t] = (a[0] for a in rerank.rerank(q[j:j + 1], hits[j:j + 1, :r], t))
    return idx, dist


def filtered_adc_then_rerank(adc_search, n: int, dim: int, q: np.ndarray, topk: int, rerank, candidates):
    """`flat.adc_then_rerank` behind a filtered first stage: `adc_search(q, c)` returns allowed rows only, PAD_ID behind them
    where a query has fewer than c, so the exact rerank goes through `rerank_hits`"""
    from .flat import rerank_candidates

    c = rerank_candidates(n, dim, topk, rerank, candidates)
    hits, _ = adc_search(q, c)
    return rerank_hits(q, hits, topk, rerank)


class IVFIndexBase:
    """coarse centroids (nlist, dim) + distance + the list id of every added row; `_ix` is the device handle or None.
    `_host` is the payload on the host, one stored row per added row -- or None once the handle holds the only copy.
    A subclass states ``_new_handle()``, `_UPLOAD` (the handle's add entry that takes the stored form), `_READ_BACK` (the
    handle's accessor of the stored form: the payload is then handed over to the handle, and read back by ``close``;
    None: the host twin stays), and for its file `_HEADER`, `_MAGICS`, ``_header()``, ``_file()``."""

    _UPLOAD = "add"
    _READ_BACK = None

    def _init_lists(self, coarse: np.ndarray, distance: Distance, payload: np.ndarray) -> None:
        """payload: the empty (0, items a row) array of the stored form"""
        self._distance = distance
        self._coarse = coarse
        self._lists = np.empty(0, np.uint32)
        self._host = payload
        self._ix = None

    # -- shape ------------------------------------------------------------------------------
    @property
    def nlist(self) -> int:
        return self._coarse.shape[0]

    @property
    def dim(self) -> int:
        return self._coarse.shape[1]

    @property
    def distance(self) -> Distance:
        return self._distance

    @property
    def coarse_centroids(self) -> np.ndarray:
        return self._coarse

    @property
    def list_ids(self) -> np.ndarray:
        """(n,) uint32: the list of every row, in row order"""
        return self._lists

    def __len__(self) -> int:
        return self._lists.shape[0]

    def list_sizes(self) -> np.ndarray:
        """(nlist,) uint64: rows per list"""
        return np.bincount(self._lists, minlength=self.nlist).astype(np.uint64)

    # -- build ------------------------------------------------------------------------------
    def _add_rows_2d(self, X) -> np.ndarray:
        """the rows given to `add` as float32 (n, dim)"""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim == 1:
            X = X[None, :]
        if X.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if X.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, X.shape[1])
        return X

    def add(self, X) -> np.ndarray:
        """assign each row of X (n, dim) to its nearest coarse centroid (the reference's nearest-centroid rule, on the
        float32 values of X) and append it with `add_rows`; returns the new row ids"""
        X = self._add_rows_2d(X)
        if X.shape[0] == 0:
            return np.empty(0, np.uint32)
        return self.add_rows(_nearest_lists(self._coarse, X, self._assign_metric()), X)

    def _assign_metric(self) -> int:
        """the metric that assigns rows to lists in `add`: the one the index probes under"""
        return self._distance.metric

    def _check_list_ids(self, lid: np.ndarray) -> None:
        if lid.size and (lid.dtype.kind not in "iu" or int(lid.min()) < 0 or int(lid.max()) >= self.nlist):
            raise InvalidParameter("list_ids", f"must be integers in [0, {self.nlist})")

    def _check_room(self, n_new: int, what: str) -> None:
        if len(self) + n_new >= 1 << 32:
            raise InvalidParameter(what, "an index holds at most 2^32 - 1 rows")

    def _add_shape(self, list_ids, a, what: str, width: int, shape_only: bool = False):
        """the first half of an add's front: list ids (n,) against the array `a` (n, width), named `what` in the errors.
        shape_only: a wrong width is reported as a wrong shape (IVFPQIndex).  Returns both as arrays."""
        lid = np.asarray(list_ids)
        a = np.asarray(a)
        if lid.ndim != 1:
            raise InvalidParameter("list_ids", "must be a 1D array (n,)")
        if a.ndim != 2 or (shape_only and a.shape[1] != width):
            raise InvalidParameter(what, f"must have shape (n, {width})")
        if a.shape[1] != width:
            raise DimensionMismatch(width, a.shape[1])
        if a.shape[0] != lid.shape[0]:
            raise DimensionMismatch(lid.shape[0], a.shape[0])
        return lid, a

    def _add_lists(self, lid: np.ndarray, what: str) -> np.ndarray:
        """the second half: list ids in range and room for them; the list ids as uint32"""
        self._check_list_ids(lid)
        self._check_room(lid.shape[0], what)
        return np.ascontiguousarray(lid, dtype=np.uint32)

    def _add_front(self, list_ids, a, what: str, width: int):
        """both halves, for a class whose checks of `a` itself come behind them"""
        lid, a = self._add_shape(list_ids, a, what, width)
        return self._add_lists(lid, what), a

    def _append(self, lid: np.ndarray, given: np.ndarray, entry: str | None = None, stored=None) -> np.ndarray:
        """append checked rows to whichever side holds the payload: `given` goes to the handle, if there is one, through
        its add `entry` (default: the upload's); to the host array, if it holds the rows, as ``stored(given)`` (default:
        as given).  Returns the new row ids."""
        if self._ix is not None and lid.size:
            getattr(self._ix, entry or self._UPLOAD)(lid, given)  # the handle first: the one step that can fail
        if self._host is not None:
            self._host = np.concatenate([self._host, given if stored is None else stored(given)])
        return self._appended(lid)

    def _appended(self, lid: np.ndarray) -> np.ndarray:
        n0 = len(self)
        self._lists = np.concatenate([self._lists, lid])
        return np.arange(n0, n0 + lid.shape[0], dtype=np.uint32)

    def _stored(self) -> np.ndarray:
        """(n, items a row): the payload, from the host or from the handle that holds it"""
        return self._host if self._host is not None else getattr(self._ix, self._READ_BACK)()

    def _new_handle(self):
        """the _lib handle over the coarse centroids, empty (a subclass's)"""
        raise NotImplementedError

    def _handle(self):
        """the handle, made and given the rows on first use"""
        if self._ix is None:
            ix = self._new_handle()
            if len(self):
                getattr(ix, self._UPLOAD)(self._lists, self._host)
            self._ix = ix
            if self._READ_BACK is not None:
                self._host = None  # the handle holds the only copy
        return self._ix

    def remove_rows(self, mask_or_ids) -> np.ndarray:
        """remove the rows of a bool mask (n,) -- True: remove -- or of an integer array of row ids in [0, n), in any
        order, repeats welcome.  The remaining rows keep their order, their lists and move up: returns `kept` uint32, the
        old ids of the remaining rows in their new order (``kept[new id] = old id``), as ``ResidentIndex.remove_rows``
        does -- so a reranker over the same rows follows with the same argument.  Removing every row is allowed: the
        index is then as empty as a trained one, and adds work.  Every check runs before anything changes.  A device
        state that is current stays current (the next search pays no upload); without one no device is touched."""
        n = len(self)
        a = np.asarray(mask_or_ids)
        if a.size == 0 and a.ndim == 1 and a.dtype != np.bool_:
            a = a.astype(np.int64)  # (an empty list of ids)
        if n == 0:  # an empty index accepts only an empty removal
            if a.ndim != 1:
                raise InvalidParameter("mask_or_ids", f"must be a 1D array, got {a.ndim} dimensions")
            if a.dtype != np.bool_ and a.dtype.kind not in "iu":
                raise InvalidParameter("mask_or_ids", f"must be a bool array or an integer array of row ids, got {a.dtype}")
            if a.size:
                if a.dtype == np.bool_:
                    raise DimensionMismatch(0, a.shape[0])
                raise InvalidParameter("mask_or_ids", "the index holds no row")
            return np.empty(0, np.uint32)
        words = pack_row_mask(a, n)
        gone = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
        kept = np.flatnonzero(~gone).astype(np.uint32)
        if kept.shape[0] == n:
            return kept
        if self._ix is not None:
            self._ix.remove(words)  # the handle first: the one step that can fail
        self._lists = self._lists[kept]
        if self._host is not None:  # (else the handle holds the only copy)
            self._host = self._host[kept]
        return kept

    # -- search -----------------------------------------------------------------------------
    def _queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError("expected a 2D array (nq, dim)")
        if q.shape[1] != self.dim:
            raise DimensionMismatch(self.dim, q.shape[1])
        return q

    def _nprobe(self, nprobe) -> int:
        p = _count(nprobe, "nprobe")
        if not 1 <= p <= min(self.nlist, MAX_PROBE):
            raise InvalidParameter("nprobe", f"must be between 1 and min(nlist, 1024), got {p}")
        return p

    def _topk(self, topk) -> int:
        t = _count(topk, "topk")
        if not 1 <= t <= min(len(self), MAX_TOPK):
            raise InvalidParameter("topk", f"must be between 1 and min(n, 1024), got {t}")
        return t

    def probe(self, queries, nprobe: int = 8) -> np.ndarray:
        """(nq, nprobe) uint32: the lists each query scans, nearest first"""
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        if q.shape[0] == 0:
            return np.empty((0, p), np.uint32)
        return self._handle().probe(q, p)

    def search(self, queries, topk: int = 10, nprobe: int = 8, *, rerank=None, candidates: int | None = None):
        """(nq, dim) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first; slots
        past the probed rows hold 0xFFFFFFFF / +inf.  rerank: a FlatIndex or a ScalarIndex over the same rows -- the search
        then returns `candidates` hits per query (default 4 topk, at most 1024 and n) and the exact rerank of the real
        ones"""
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        if rerank is not None:
            return self._search_rerank(q, t, p, rerank, candidates)
        if q.shape[0] == 0:
            return np.empty((0, t), np.uint32), np.empty((0, t), np.float32)
        return self._handle().search(q, p, t)

    def _search_rerank(self, q, topk: int, nprobe: int, rerank, candidates, allowed=None):
        """allowed: the row-mask words of a filtered call (IVFFilterMixin) -- the first stage then returns allowed rows
        only, and the reranker needs nothing"""
        from .flat import rerank_candidates

        c = rerank_candidates(len(self), self.dim, topk, rerank, candidates)
        if q.shape[0] == 0:
            return np.empty((0, topk), np.uint32), np.empty((0, topk), np.float32)
        if allowed is None:
            hits, _ = self._handle().search(q, nprobe, c)
        else:
            hits, _ = self._handle().search_masked(q, nprobe, c, allowed)
        return rerank_hits(q, hits, topk, rerank)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, nprobe: int = 8) -> None:
        """device pointers: queries [nq][dim] f32, results [nq][topk] uint32 / f32; asynchronous on the current stream"""
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        n_q = _nq(nq)
        self._handle().search_device(int(dev_queries), n_q, p, t, int(dev_idx), int(dev_dist))

    def close(self) -> None:
        """release the handle and its device state (the next probe or search builds it again); the rows stay"""
        if self._ix is not None:
            if self._host is None:
                self._host = self._stored()
            self._ix.close()
            self._ix = None

    # -- file -------------------------------------------------------------------------------
    def _header(self) -> tuple:
        """the fields of `_HEADER`, the magic first (a subclass's)"""
        raise NotImplementedError

    @classmethod
    def _file(cls, *fields) -> IVFFile:
        """the checks of a header's fields behind the magic's -- ValueError("corrupt index header...") -- and what they
        say of the file (a subclass's)"""
        raise NotImplementedError

    def _file_extra(self) -> tuple:
        """the arrays of `IVFFile.extra`"""
        return ()

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self._HEADER.pack(*self._header()))
            for block in (self._coarse, *self._file_extra()):
                f.write(block.astype("<f4").tobytes())
            f.write(self._lists.astype("<u4").tobytes())
            stored = self._stored()
            f.write(stored.astype(stored.dtype.newbyteorder("<")).tobytes())

    @classmethod
    def load(cls, path):
        """read the class's file; every field, every list id and the payload are checked here, before anything can reach
        the device"""
        with open(path, "rb") as f:
            head = f.read(cls._HEADER.size)
            if len(head) != cls._HEADER.size:
                raise ValueError("truncated index header")
            fields = cls._HEADER.unpack(head)
            if fields[0] not in cls._MAGICS:
                raise ValueError(f"not a {' or '.join(m.decode() for m in cls._MAGICS)} file")
            h = cls._file(*fields)
            dtype, width, what = h.payload
            coarse = _block(f, (h.nlist, h.dim), "<f4", "coarse centroids")
            extra = [_block(f, shape, "<f4", name) for shape, name in h.extra]
            lists = _block(f, (h.n,), "<u4", "list ids")
            payload = _block(f, (h.n, width), dtype, what)
            if f.read(1):
                raise ValueError(f"trailing bytes after the {what}")
        if lists.size and int(lists.max()) >= h.nlist:
            raise ValueError(f"corrupt index: a list id is outside [0, {h.nlist})")
        if h.check is not None:
            h.check(payload)
        self = h.make(coarse, *extra)
        self._lists, self._host = lists, payload
        return self


class IVFEncodedBase(IVFIndexBase):
    """an inverted file that stores codes or words, encodes float rows on the device, and hands its payload over to the
    handle (IVFScalarIndex, IVFScalar4Index, IVFBinaryIndex)"""

    def add_rows(self, list_ids, rows) -> np.ndarray:
        """encode rows (n, dim) floating point, as float32, on the device -- into the stored form that the class's rule
        gives (the codes of ``quantizer.quantize_batch``, packed where the index packs; the bits x >= threshold) -- and
        append them into the lists list_ids (n,) < nlist; returns the new row ids"""
        lid, r = self._add_front(list_ids, rows, "rows", self.dim)
        if r.dtype.kind != "f":
            raise InvalidParameter("rows", f"must be floating point, got {r.dtype}")
        if lid.size:
            with np.errstate(over="ignore"):
                self._handle().add_rows(lid, np.ascontiguousarray(r, dtype=np.float32))
        return self._appended(lid)


class IVFRangeMixin:
    """range search over the probed lists, for an IVFIndexBase whose distances are exact (IVFFlatIndex, IVFScalarIndex, IVFScalar4Index):
    ``S(q)`` and ``D(q, i)`` are `search`'s at the same nprobe"""

    def range_search(self, queries, radius, nprobe: int = 8, max_results: int = DEFAULT_MAX_RESULTS):
        """every row of the nprobe nearest lists within `radius` of each query: row i is a hit of query q iff its list is
        probed and D(q, i) <= radius[q] as a float32 comparison (NaN distances never hit).  `radius` is a scalar or nq
        values.  Returns (lims uint64 (nq + 1,), idx uint32 (total,), dist float32 (total,)): the hits of query q are
        idx[lims[q]:lims[q + 1]], in ascending row id.  More than `max_results` hits in all: FfiError (ERR_UNSUPPORTED)."""
        q = self._queries(queries)
        r = _radii(radius, q.shape[0])
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._handle().range_search(q, p, r, m).read()

    def range_search_device(self, dev_queries: int, nq: int, radius, nprobe: int = 8,
                            max_results: int = DEFAULT_MAX_RESULTS) -> "_lib.RangeResult":
        """`range_search` with the queries [nq][dim] f32 at a device pointer (4-byte aligned) and the result left on the
        device: a RangeResult (.total, .lims, .device_pointers(), .read()).  Returns when the result is complete."""
        n_q = _nq(nq)
        r = _radii(radius, n_q)
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        return self._handle().range_search_device(int(dev_queries), n_q, p, r, m)
