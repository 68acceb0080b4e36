"""``BinaryFilterMixin`` / ``IVFBinaryFilterMixin`` -- the filtered forms of search and Hamming-radius range search of the
two binary indexes (``BinaryIndex``, ``IVFBinaryIndex``).  A filter is one row mask per call,
`allowed`: a bool array (n,) (True: the row may be returned) or its uint32 words (``pack_row_mask``), n being
``len(index)`` at the time of the call.  The unfiltered methods keep their signatures, so the filtered forms are methods of
their own, ``filtered_*``.  Both mixins run one body: the inverted file's adds `nprobe` in front of the handle's arguments
(probing takes no mask: the searched set is the allowed rows of the probed lists).  include/vqhip.h states the results
(vqhip_binary_search_masked, vqhip_ivfbin_search_masked)."""
from __future__ import annotations

import numpy as np

from ._ivf_common import rerank_hits
from ._resident_common import DEFAULT_MAX_RESULTS, _allowed, _hamming_radii, _max_results, _nq
from .errors import InvalidParameter


class BinaryFilterMixin:
    """in front of BinaryIndex: `_filter_handle()` is the device handle, `_filter_check(nprobe)` the checked arguments it
    takes between the query count and topk / the radii -- none here"""

    def _filter_handle(self):
        return self._index()

    # -- the one body of each call ----------------------------------------------------------------
    def _filtered_search(self, queries, allowed, topk, nprobe, rerank, candidates):
        from .flat import rerank_candidates

        q = self._queries(queries)
        front = self._filter_check(nprobe)
        k = self._topk(topk)
        w = _allowed(allowed, len(self))
        c = k
        if rerank is not None:
            c = rerank_candidates(len(self), self.dim, k, rerank, candidates)
        elif candidates is not None:
            raise InvalidParameter("candidates", "only with rerank")
        if q.shape[0] == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        idx, dist = self._filter_handle().search_masked(q, *front, c, w)
        if rerank is None:
            return idx, dist
        return rerank_hits(q, idx, k, rerank)  # (the first stage is allowed rows only, padding behind them)

    def _filtered_search_device(self, dev_queries, nq, topk, dev_idx, dev_dist, dev_allowed, nprobe) -> None:
        front = self._filter_check(nprobe)
        k = self._topk(topk)
        n_q = _nq(nq)
        self._filter_handle().search_masked_device(int(dev_queries), n_q, *front, k, int(dev_allowed), int(dev_idx), int(dev_dist))

    def _filtered_range(self, queries, radius, allowed, nprobe, max_results):
        q = self._queries(queries)
        r = _hamming_radii(radius, q.shape[0])
        front = self._filter_check(nprobe)
        m = _max_results(max_results)
        w = _allowed(allowed, len(self))
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._filter_handle().range_search_masked(q, *front, r, m, w).read()

    def _filtered_range_device(self, dev_queries, nq, radius, dev_allowed, nprobe, max_results):
        n_q = _nq(nq)
        r = _hamming_radii(radius, n_q)
        front = self._filter_check(nprobe)
        m = _max_results(max_results)
        return self._filter_handle().range_search_masked_device(int(dev_queries), n_q, *front, r, m, int(dev_allowed))

    def _filter_check(self, nprobe) -> tuple:
        """the checked arguments in front of topk / the radii, before the device is touched"""
        return ()

    # -- BinaryIndex's four -----------------------------------------------------------------------
    def filtered_search(self, queries, allowed, topk: int = 10, *, rerank=None, candidates=None):
        """`search` over the allowed rows only: per query the first `topk` of them by (H, row id); a query with fewer
        allowed rows has the slots behind them padded with index 0xFFFFFFFF and distance +inf (`topk` itself stays within
        1 .. min(n, 1024)).  With `rerank`, the mask filters the first stage: its candidates are allowed rows."""
        return self._filtered_search(queries, allowed, topk, None, rerank, candidates)

    def filtered_search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, dev_allowed: int) -> None:
        """`search_device` under the row mask at `dev_allowed`: ceil(n / 32) uint32 words at a device pointer (4-byte
        aligned)"""
        self._filtered_search_device(dev_queries, nq, topk, dev_idx, dev_dist, dev_allowed, None)

    def filtered_hamming_range_search(self, queries, radius, allowed, max_results: int = DEFAULT_MAX_RESULTS):
        """`hamming_range_search` in which only allowed rows hit"""
        return self._filtered_range(queries, radius, allowed, None, max_results)

    def filtered_hamming_range_search_device(self, dev_queries: int, nq: int, radius, dev_allowed: int,
                                             max_results: int = DEFAULT_MAX_RESULTS):
        """`hamming_range_search_device` under the row mask's words at the device pointer `dev_allowed` (4-byte aligned)"""
        return self._filtered_range_device(dev_queries, nq, radius, dev_allowed, None, max_results)


class IVFBinaryFilterMixin(BinaryFilterMixin):
    """in front of IVFBinaryIndex: the same four with `nprobe` where the unfiltered method has it"""

    def _filter_handle(self):
        return self._handle()

    def _filter_check(self, nprobe) -> tuple:
        return (self._nprobe(nprobe),)

    def filtered_search(self, queries, allowed, topk: int = 10, nprobe: int = 8, *, rerank=None, candidates=None):
        """`search` over the allowed rows of the probed lists only (probing takes no mask); padding as `search` pads a
        query whose lists are short.  With `rerank`, the mask filters the first stage."""
        return self._filtered_search(queries, allowed, topk, nprobe, rerank, candidates)

    def filtered_search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, dev_allowed: int,
                               nprobe: int = 8) -> None:
        """`search_device` under the row mask at `dev_allowed`: ceil(n / 32) uint32 words at a device pointer (4-byte
        aligned), n the rows in the index now"""
        self._filtered_search_device(dev_queries, nq, topk, dev_idx, dev_dist, dev_allowed, nprobe)

    def filtered_hamming_range_search(self, queries, radius, allowed, nprobe: int = 8, max_results: int = DEFAULT_MAX_RESULTS):
        """`hamming_range_search` in which only allowed rows hit"""
        return self._filtered_range(queries, radius, allowed, nprobe, max_results)

    def filtered_hamming_range_search_device(self, dev_queries: int, nq: int, radius, dev_allowed: int, nprobe: int = 8,
                                             max_results: int = DEFAULT_MAX_RESULTS):
        """`hamming_range_search_device` under the row mask's words at the device pointer `dev_allowed` (4-byte aligned)"""
        return self._filtered_range_device(dev_queries, nq, radius, dev_allowed, nprobe, max_results)
