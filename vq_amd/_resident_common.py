"""What ``FlatIndex``, ``ScalarIndex``, ``Scalar4Index``, ``BinaryIndex`` and ``AsymmetricBinaryIndex`` share: the rows of
a caller's array that go to the device on the first search, the checks of queries and ``topk``, and search over the
device handle.  A subclass keeps its constructors, the checks of its own source array, ``_make_handle``, ``__repr__``
and the fields of its file.  ``ExactResidentIndex`` adds the range search and the rerank of the indexes whose distances
are exact (not ``BinaryIndex``, whose range search takes a radius in Hamming bits: ``_hamming_radii``), and the row
mask of their filtered calls (``pack_row_mask``).  ``PackedSourceMixin`` is the packed-words source of the three indexes
that store words (``from_packed`` and the ``add_*`` forms); ``write_index_file`` / ``read_index_file`` are the one writer
and reader of the four resident files.  ``_count`` and ``_nq`` serve the inverted files too."""
from __future__ import annotations

import operator

import numpy as np

from . import _lib
from .distance import Distance
from .errors import DimensionMismatch, EmptyInput, InvalidData, InvalidParameter

MAX_TOPK = 1024
MAX_CANDIDATES = 4096
DEFAULT_MAX_RESULTS = 1 << 28  # hits a range search returns at most by default: 2 GB of idx + dist


def _count(v, name: str) -> int:
    try:
        return operator.index(v)
    except TypeError:
        raise InvalidParameter(name, f"must be an integer, got {v!r}") from None


def _nq(nq) -> int:
    """the query count of a device-form call"""
    n_q = _count(nq, "nq")
    if n_q < 0 or n_q >= 1 << 32:
        raise InvalidParameter("nq", f"must be in [0, 2^32), got {n_q}")
    return n_q


def _radii(radius, nq: int) -> np.ndarray:
    """the per-query radii float32 (nq,) of a range search from a scalar or nq values; NaN is refused"""
    try:
        r = np.asarray(radius, dtype=np.float32)
    except (TypeError, ValueError):
        raise InvalidParameter("radius", f"must be a number or an array of {nq} numbers, got {radius!r}") from None
    if r.ndim == 0:
        r = np.full(nq, r, np.float32)
    if r.ndim != 1:
        raise InvalidParameter("radius", f"must be a scalar or a 1D array, got {r.ndim} dimensions")
    if r.shape[0] != nq:
        raise DimensionMismatch(nq, r.shape[0])
    if bool(np.isnan(r).any()):
        raise InvalidParameter("radius", f"is NaN for query {int(np.flatnonzero(np.isnan(r))[0])}")
    return np.ascontiguousarray(r)


def _hamming_radii(radius, nq: int) -> np.ndarray:
    """the per-query Hamming radii uint32 (nq,) of a binary index's range search from a non-negative integer or nq of
    them; floats that are not integral, negatives and values >= 2^32 are refused"""
    try:
        r = np.asarray(radius)
        if r.dtype.kind not in "iufb":
            raise TypeError
        r = r.astype(np.float64) if r.dtype.kind == "f" else r.astype(object)
    except (TypeError, ValueError):
        raise InvalidParameter("radius", f"must be a non-negative integer or an array of {nq} of them, got {radius!r}") from None
    if r.ndim > 1:
        raise InvalidParameter("radius", f"must be a scalar or a 1D array, got {r.ndim} dimensions")
    flat = r.reshape(-1)
    for j, v in enumerate(flat.tolist()):
        where = "" if r.ndim == 0 else f" for query {j}"
        if isinstance(v, float) and not v.is_integer():  # (NaN and the infinities are not integers either)
            raise InvalidParameter("radius", f"must be an integer number of bits, got {v!r}{where}")
        if not 0 <= int(v) < 1 << 32:
            raise InvalidParameter("radius", f"must be in [0, 2^32), got {int(v)}{where}")
    out = np.array([int(v) for v in flat.tolist()], dtype=np.uint32)
    if r.ndim == 0:
        out = np.full(nq, out[0], np.uint32)
    if out.shape[0] != nq:
        raise InvalidParameter("radius", f"one radius or one per query ({nq}), got {out.shape[0]}")
    return np.ascontiguousarray(out)


def mask_words(n: int) -> int:
    """the uint32 words of a row mask over n rows"""
    return (n + 31) // 32


def _pack_bools(m: np.ndarray) -> np.ndarray:
    """bool (n,) -> uint32 (ceil(n / 32),): row i is bit i & 31 of word i >> 5, the pad bits zero"""
    by = np.packbits(m, bitorder="little")
    out = np.zeros(mask_words(m.shape[0]) * 4, np.uint8)
    out[:by.shape[0]] = by
    return out.view("<u4").astype(np.uint32)


def pack_row_mask(mask_or_ids, n: int) -> np.ndarray:
    """The row mask of an index of `n` rows as uint32 words (ceil(n / 32),), the form ``search(..., allowed=)`` and
    ``range_search(..., allowed=)`` take: row i is allowed iff bit ``i & 31`` of word ``i >> 5`` is set.
    `mask_or_ids` is a bool array (n,) -- True: allowed -- or an integer array of allowed row ids in [0, n), in any
    order, repeats welcome."""
    rows = _count(n, "n")
    if not 1 <= rows < 1 << 32:
        raise InvalidParameter("n", f"must be in [1, 2^32), got {rows}")
    a = np.asarray(mask_or_ids)
    if a.ndim != 1:
        raise InvalidParameter("mask_or_ids", f"must be a 1D array, got {a.ndim} dimensions")
    if a.dtype == np.bool_:
        if a.shape[0] != rows:
            raise DimensionMismatch(rows, a.shape[0])
        return _pack_bools(a)
    if a.dtype.kind not in "iu":
        raise InvalidParameter("mask_or_ids", f"must be a bool array or an integer array of row ids, got {a.dtype}")
    m = np.zeros(rows, np.bool_)
    if a.size:
        lo, hi = int(a.min()), int(a.max())
        if lo < 0 or hi >= rows:
            raise InvalidParameter("mask_or_ids", f"row id {lo if lo < 0 else hi} is outside [0, {rows})")
        m[a.astype(np.int64)] = True
    return _pack_bools(m)


def _allowed(allowed, n: int) -> np.ndarray:
    """the row-mask words uint32 (ceil(n / 32),) of a filtered call from its `allowed` argument: a bool array (n,),
    packed here, or the words themselves"""
    a = np.asarray(allowed)
    if a.dtype != np.bool_ and a.dtype != np.uint32:
        raise InvalidParameter("allowed", f"must be a bool array ({n},) or uint32 words ({mask_words(n)},), got {a.dtype}")
    if a.ndim != 1:
        raise InvalidParameter("allowed", f"must be a 1D array, got {a.ndim} dimensions")
    want = n if a.dtype == np.bool_ else mask_words(n)
    if a.shape[0] != want:
        raise DimensionMismatch(want, a.shape[0])
    return _pack_bools(a) if a.dtype == np.bool_ else np.ascontiguousarray(a)


def _max_results(max_results) -> int:
    m = _count(max_results, "max_results")
    if not 1 <= m < 1 << 64:
        raise InvalidParameter("max_results", f"must be in [1, 2^64), got {m}")
    return m


def _check_distance(distance, default: Distance) -> Distance:
    if distance is None:
        distance = default
    if not isinstance(distance, Distance):
        raise InvalidParameter("distance", f"expected a Distance, got {type(distance).__name__}")
    return distance


def write_index_file(path, header: bytes, payload: np.ndarray) -> None:
    """a resident index file: the packed header, then the payload little endian"""
    with open(path, "wb") as f:
        f.write(header)
        f.write(payload.astype(payload.dtype.newbyteorder("<")).tobytes())


def read_index_file(path, header, magic: bytes, noun: str, fields):
    """Read a resident index file of the struct `header` under `magic`; `noun` names the index in the messages.
    ``fields(*header fields behind the magic)`` is the class's own checks: it returns (n, width, dtype, what, finish)
    -- the payload is n * width items of `dtype`, `what` names it, and ``finish(payload (n, width))`` checks it and
    makes the index.  Truncation and trailing bytes are refused here."""
    with open(path, "rb") as f:
        head = f.read(header.size)
        if len(head) != header.size:
            raise InvalidData(f"truncated {noun} header")
        got = header.unpack(head)
        if got[0] != magic:
            raise InvalidData(f"not a {magic.decode()} file")
        n, width, dtype, what, finish = fields(*got[1:])
        dt = np.dtype(dtype)
        raw = f.read(n * width * dt.itemsize)
        if len(raw) != n * width * dt.itemsize:
            raise InvalidData(f"truncated {what}")
        if f.read(1):
            raise InvalidData(f"trailing bytes after the {what}")
    return finish(np.frombuffer(raw, dtype=dt).astype(dt.newbyteorder("=")).reshape(n, width))


def check_file_rows(n: int) -> None:
    if not 1 <= n < 1 << 32:
        raise InvalidData(f"row count {n} is outside [1, 2^32)")


class ResidentIndex:
    """n rows of `dim` under `distance`; `_src` is the caller's array until the first search, `_ix` the device handle
    from then on (None before)"""

    def _set_source(self, a: np.ndarray, what: str, distance: Distance, dim: int | None = None) -> None:
        """the shared end of every constructor: the shape checks of the source array `a` (`what` names it in errors;
        `dim`: the dimension, where it is not the array's second extent) and the fields of this class"""
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, dim)")
        if a.shape[0] == 0:
            raise EmptyInput()
        d = a.shape[1] if dim is None else dim
        self._distance = distance
        self._check_dim(d, what)
        if a.shape[0] >= 1 << 32:
            raise InvalidParameter(what, f"at most 2^32 - 1 rows, got {a.shape[0]}")
        self._src = np.ascontiguousarray(a)
        self._n, self._dim = int(a.shape[0]), int(d)
        self._ix = None

    def _check_dim(self, d: int, what: str) -> None:
        if d == 0:
            raise InvalidParameter(what, "dimension must be at least 1")

    def __len__(self) -> int:
        return self._n

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def distance(self) -> Distance:
        return self._distance

    def _make_handle(self):
        """the _lib handle over `_src` (a subclass's)"""
        raise NotImplementedError

    def _index(self):
        if self._ix is None:
            self._ix = self._make_handle()
            self._src = None  # on the device now
        return self._ix

    def _queries(self, queries) -> np.ndarray:
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2:
            raise ValueError("expected a 2D array (nq, dim)")
        if q.shape[1] != self._dim:
            raise DimensionMismatch(self._dim, q.shape[1])
        if q.shape[0] >= 1 << 32:
            raise InvalidParameter("queries", f"at most 2^32 - 1 queries, got {q.shape[0]}")
        return q

    def _topk(self, topk, limit: int | None = None, what: str = "min(n, 1024)") -> int:
        k = _count(topk, "topk")
        if not 1 <= k <= (min(self._n, MAX_TOPK) if limit is None else limit):
            raise InvalidParameter("topk", f"must be between 1 and {what}, got {k}")
        return k

    def search(self, queries, topk: int = 10):
        """(nq, d) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first"""
        return self._search(self._queries(queries), self._topk(topk))

    def _search(self, q: np.ndarray, k: int):
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        return self._index().search(q, k)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int) -> None:
        """device pointers: queries [nq][d] f32, results [nq][topk] uint32 / f32 (4-byte aligned); asynchronous on the
        current stream"""
        k = self._topk(topk)
        n_q = _nq(nq)
        self._index().search_device(int(dev_queries), n_q, k, int(dev_idx), int(dev_dist))

    # -- adding and removing rows (include/vqhip.h, "adding and removing rows") ----------------
    # After any sequence of these, every call on the index returns bit for bit what a fresh index over the remaining rows
    # returns.  A mutation first puts the index on the device (there is no host-side twin of the rows); every argument
    # is checked before that, and a call that adds or removes nothing does not touch the device.  They allocate and
    # return synchronised, so they cannot be captured into a graph.

    def _add_form(self):
        """(the entry point of ``add``, the dtype of its rows, what it passes between the source and the count) -- a
        subclass's"""
        raise NotImplementedError

    def _room(self, b: int, what: str) -> None:
        if self._n + b >= 1 << 32:
            raise InvalidParameter(what, f"at most 2^32 - 1 rows in all, got {self._n} + {b}")

    def _added(self, a, dtype, what: str, width: int | None = None) -> np.ndarray:
        """the checks of a host array (b, width) of `dtype` that an add appends (`width`: the dimension by default)"""
        a = a if isinstance(a, np.ndarray) else np.asarray(a)
        if a.dtype != dtype:
            raise InvalidParameter(what, f"dtype must be {np.dtype(dtype).name}, got {a.dtype}")
        if a.ndim != 2:
            raise ValueError(f"expected a 2D array (n, {'dim' if width is None else 'words'})")
        w = self._dim if width is None else width
        if a.shape[1] != w:
            raise DimensionMismatch(w, a.shape[1])
        self._room(a.shape[0], what)
        return np.ascontiguousarray(a)

    def _append(self, name: str, src, b: int, *front) -> np.ndarray:
        """b rows from `src` (a checked host array, or a device pointer) through entry point `name`; their ids"""
        if b == 0:
            return np.empty(0, np.uint32)
        self._index().add(name, src, b, *front)
        ids = np.arange(self._n, self._n + b, dtype=np.uint32)
        self._n += b
        return ids

    def _append_device(self, name: str, dev_src: int, n, *front) -> np.ndarray:
        b = _count(n, "n")
        if b < 0:
            raise InvalidParameter("n", f"must be at least 0, got {b}")
        self._room(b, "n")
        return self._append(name, int(dev_src), b, *front)

    def add(self, rows) -> np.ndarray:
        """append `rows` (b, dim), in the dtype the index was built from rows of; returns their ids uint32 (b,): n .. n +
        b - 1.  What is stored is what the constructor stores for the same rows."""
        name, dtype, front = self._add_form()
        a = self._added(rows, dtype, "rows")
        return self._append(name, a, a.shape[0], *front)

    def add_device(self, dev_rows: int, n: int) -> np.ndarray:
        """``add`` with the rows [n][dim] at a device pointer (4-byte aligned, but for float16 rows); returns their ids"""
        name, _, front = self._add_form()
        return self._append_device(name + "_device", dev_rows, n, *front)

    def remove_rows(self, mask_or_ids) -> np.ndarray:
        """remove the rows of a bool mask (n,) -- True: remove -- or of an integer array of row ids in [0, n), in any
        order, repeats welcome.  The remaining rows keep their order and move up: returns `kept` uint32, the old ids of
        the remaining rows in their new order (``kept[new id] = old id``), for the caller's side tables.  Removing every
        row is refused: an index holds at least one."""
        a = np.asarray(mask_or_ids)
        if a.size == 0 and a.ndim == 1 and a.dtype != np.bool_:
            a = a.astype(np.int64)  # (an empty list of ids)
        words = pack_row_mask(a, self._n)
        gone = np.unpackbits(words.view(np.uint8), bitorder="little")[:self._n].astype(bool)
        kept = np.flatnonzero(~gone).astype(np.uint32)
        if kept.shape[0] == 0:
            raise InvalidParameter("mask_or_ids", f"would leave no row of {self._n}; an index holds at least one")
        if kept.shape[0] == self._n:
            return kept
        self._index().remove(words)
        self._n = int(kept.shape[0])
        return kept

    def remove_rows_device(self, dev_remove: int) -> int:
        """``remove_rows`` with the mask's ceil(n / 32) uint32 words at a device pointer (4-byte aligned; bit set:
        remove); returns the number of rows removed.  A mask of every row is an FfiError (ERR_INVALID_INPUT)."""
        removed = self._index().remove(int(dev_remove))
        self._n -= removed
        return removed


class ExactResidentIndex(ResidentIndex):
    """a ResidentIndex whose distances are exact (FlatIndex, ScalarIndex, Scalar4Index, AsymmetricBinaryIndex): range search, the rerank of candidates, and
    the filtered forms of search and range search.  A filter is one row mask per call, `allowed`: a bool array (n,)
    (True: the row may be returned) or its uint32 words (``pack_row_mask``); None: every row, the unfiltered call."""

    def search(self, queries, topk: int = 10, allowed=None):
        """(nq, d) float32 queries -> (indices uint32 (nq, topk), distances float32 (nq, topk)), nearest first.  With
        `allowed`, the nearest among the allowed rows only; a query with fewer than `topk` of them has the slots behind
        them padded with index 0xFFFFFFFF and distance +inf (`topk` itself stays within 1 .. min(n, 1024))."""
        q = self._queries(queries)
        k = self._topk(topk)
        if allowed is None:
            return self._search(q, k)
        w = _allowed(allowed, self._n)
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        return self._index().search_masked(q, k, w)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, dev_allowed: int | None = None) -> None:
        """device pointers: queries [nq][d] f32, results [nq][topk] uint32 / f32 (4-byte aligned); asynchronous on the
        current stream.  `dev_allowed`: the row mask's ceil(n / 32) uint32 words at a device pointer (4-byte aligned)."""
        k = self._topk(topk)
        n_q = _nq(nq)
        if dev_allowed is None:
            self._index().search_device(int(dev_queries), n_q, k, int(dev_idx), int(dev_dist))
        else:
            self._index().search_masked_device(int(dev_queries), n_q, k, int(dev_allowed), int(dev_idx), int(dev_dist))

    def range_search(self, queries, radius, max_results: int = DEFAULT_MAX_RESULTS, allowed=None):
        """every row within `radius` of each query: row i is a hit of query q iff D(q, i) <= radius[q] as a float32
        comparison (NaN distances never hit).  `radius` is a scalar or nq values.  Returns (lims uint64 (nq + 1,),
        idx uint32 (total,), dist float32 (total,)): the hits of query q are idx[lims[q]:lims[q + 1]], in ascending
        row id.  More than `max_results` hits in all: FfiError (ERR_UNSUPPORTED).  With `allowed`, only allowed rows
        hit."""
        q = self._queries(queries)
        r = _radii(radius, q.shape[0])
        m = _max_results(max_results)
        w = None if allowed is None else _allowed(allowed, self._n)
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        if w is None:
            return self._index().range_search(q, r, m).read()
        return self._index().range_search_masked(q, r, m, w).read()

    def range_search_device(self, dev_queries: int, nq: int, radius, max_results: int = DEFAULT_MAX_RESULTS,
                            dev_allowed: int | None = None) -> "_lib.RangeResult":
        """`range_search` with the queries [nq][d] f32 at a device pointer (4-byte aligned) and the result left on the
        device: a RangeResult (.total, .lims, .device_pointers(), .read()).  Returns when the result is complete.
        `dev_allowed`: the row mask's ceil(n / 32) uint32 words at a device pointer (4-byte aligned)."""
        n_q = _nq(nq)
        r = _radii(radius, n_q)
        m = _max_results(max_results)
        if dev_allowed is None:
            return self._index().range_search_device(int(dev_queries), n_q, r, m)
        return self._index().range_search_masked_device(int(dev_queries), n_q, r, m, int(dev_allowed))

    def rerank(self, queries, candidates, topk: int = 10):
        """per query, the `topk` nearest of its candidate row ids (nq, c), 1 <= c <= 4096, distinct within a query;
        returns (indices uint32 (nq, topk), distances float32 (nq, topk)) in the order of `search`"""
        q = self._queries(queries)
        c = np.asarray(candidates)
        if c.ndim == 1 and q.shape[0] == 1:
            c = c[None, :]
        if c.ndim != 2:
            raise ValueError("expected candidates as a 2D array (nq, c)")
        if c.shape[0] != q.shape[0]:
            raise DimensionMismatch(q.shape[0], c.shape[0])
        if c.dtype.kind not in "iu":
            raise InvalidParameter("candidates", f"row ids must be integers, got {c.dtype}")
        if not 1 <= c.shape[1] <= MAX_CANDIDATES:
            raise InvalidParameter("candidates", f"between 1 and {MAX_CANDIDATES} per query, got {c.shape[1]}")
        k = self._topk(topk, c.shape[1], "the number of candidates")
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        lo, hi = int(c.min()), int(c.max())
        if lo < 0 or hi >= self._n:
            bad = lo if lo < 0 else hi
            raise InvalidParameter("candidates", f"row id {bad} is outside [0, {self._n})")
        s = np.sort(c, axis=1)
        if c.shape[1] > 1 and bool((s[:, 1:] == s[:, :-1]).any()):
            raise InvalidParameter("candidates", "row ids must be distinct within a query")
        return self._index().rerank(q, np.ascontiguousarray(c, dtype=np.uint32), k)


class PackedSourceMixin:
    """in front of a ResidentIndex that stores uint32 words and takes rows in three forms -- float32 rows, u8 codes, the
    words themselves (``BinaryIndex``, ``AsymmetricBinaryIndex``: 32 bits a word; ``Scalar4Index``: 8 nibbles).  A subclass
    states `_F32`, `_U8`, `_PACKED` (the _lib source kinds), `_PAD` (what a pad position is called), `_words(dim)`,
    `_pad_ok(words, dim)`, `_packed_dim(d)` (the check of ``from_packed``'s dim) and, where codes have a limit,
    `_codes_ok(codes)`; its ``_setup(a, kind, quantizer, distance, dim=None)`` ends every constructor."""

    _codes_ok = staticmethod(lambda codes: None)

    @classmethod
    def _from_packed(cls, words, dim, quantizer, distance):
        a = words if isinstance(words, np.ndarray) else np.asarray(words)
        if a.dtype != np.uint32:
            raise InvalidParameter("words", f"dtype must be uint32, got {a.dtype}")
        d = _count(dim, "dim")
        if a.ndim != 2:
            raise ValueError("expected a 2D array (n, words)")
        cls._packed_dim(d)
        if a.shape[1] != cls._words(d):
            raise DimensionMismatch(cls._words(d), a.shape[1])
        if not cls._pad_ok(a, d):
            raise InvalidParameter("words", f"a row has a pad {cls._PAD} (dimension >= {d}) set")
        self = cls.__new__(cls)
        self._setup(a, cls._PACKED, quantizer, distance, dim=d)
        return self

    @property
    def quantizer(self):
        return self._quantizer

    def _add_form(self):
        return "add", np.float32, (self._F32,)  # float32 rows, put into words on the device as the constructor's are

    def add_codes(self, codes) -> np.ndarray:
        """append u8 codes (b, dim) in ``from_codes``'s form and under its limits; returns their ids uint32 (b,)"""
        a = self._added(codes, np.uint8, "codes")
        self._codes_ok(a)
        return self._append("add", a, a.shape[0], self._U8)

    def add_packed(self, words) -> np.ndarray:
        """append packed rows uint32 (b, words of a row) in the index layout, pad positions zero (``from_packed``'s
        form); returns their ids uint32 (b,)"""
        a = self._added(words, np.uint32, "words", self._words(self._dim))
        if not self._pad_ok(a, self._dim):
            raise InvalidParameter("words", f"a row has a pad {self._PAD} (dimension >= {self._dim}) set")
        return self._append("add", a, a.shape[0], self._PACKED)

    def add_packed_device(self, dev_words: int, n: int) -> np.ndarray:
        """``add_packed`` with the words [n][words of a row] at a device pointer (4-byte aligned); a pad position set is
        an FfiError (ERR_INVALID_INPUT) that leaves the index as it was.  Returns their ids."""
        return self._append_device("add_device", dev_words, n, self._PACKED)
