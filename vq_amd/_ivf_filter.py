"""``IVFFilterMixin`` -- the filtered forms of search and range search of the inverted files whose distances are exact
(``IVFFlatIndex``, ``IVFScalarIndex``, ``IVFScalar4Index``; ``IVFBinaryIndex`` has ``_binary_filter.py``'s methods, ``IVFPQIndex`` its own ``masked_search``).  A
filter is one row mask per call, `allowed`: a bool array (n,) (True: the row may be returned) or its uint32 words
(``pack_row_mask``), n being ``len(index)`` at the time of the call; None: every row, the unfiltered call.  Probing takes no mask: ``P(q)`` is the nprobe nearest lists
whatever they hold, and the searched set is the allowed rows of ``S(q)`` (include/vqhip.h, vqhip_ivfflat_search_masked)."""
from __future__ import annotations

import numpy as np

from ._resident_common import DEFAULT_MAX_RESULTS, _allowed, _max_results, _nq, _radii


class IVFFilterMixin:
    """in front of IVFRangeMixin and IVFIndexBase: every call without a mask is theirs, argument for argument"""

    def search(self, queries, topk: int = 10, nprobe: int = 8, *, rerank=None, candidates: int | None = None, allowed=None):
        """`IVFIndexBase.search`; with `allowed`, the nearest among the allowed rows of the probed lists only -- a query
        with fewer than `topk` of them has the slots behind them padded with 0xFFFFFFFF / +inf (`topk` itself stays within
        1 .. min(n, 1024)).  With `rerank`, the mask filters the first stage: its candidates are allowed rows."""
        if allowed is None:
            return super().search(queries, topk, nprobe, rerank=rerank, candidates=candidates)
        q = self._queries(queries)
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        w = _allowed(allowed, len(self))
        if rerank is not None:
            return self._search_rerank(q, t, p, rerank, candidates, allowed=w)
        if q.shape[0] == 0:
            return np.empty((0, t), np.uint32), np.empty((0, t), np.float32)
        return self._handle().search_masked(q, p, t, w)

    def search_device(self, dev_queries: int, nq: int, topk: int, dev_idx: int, dev_dist: int, nprobe: int = 8,
                      dev_allowed: int | None = None) -> None:
        """`IVFIndexBase.search_device`; `dev_allowed`: the row mask's ceil(n / 32) uint32 words at a device pointer (4-byte
        aligned)"""
        if dev_allowed is None:
            return super().search_device(dev_queries, nq, topk, dev_idx, dev_dist, nprobe)
        p = self._nprobe(nprobe)
        t = self._topk(topk)
        n_q = _nq(nq)
        self._handle().search_masked_device(int(dev_queries), n_q, p, t, int(dev_allowed), int(dev_idx), int(dev_dist))

    def range_search(self, queries, radius, nprobe: int = 8, max_results: int = DEFAULT_MAX_RESULTS, allowed=None):
        """`IVFRangeMixin.range_search`; with `allowed`, only allowed rows hit"""
        if allowed is None:
            return super().range_search(queries, radius, nprobe, max_results)
        q = self._queries(queries)
        r = _radii(radius, q.shape[0])
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        w = _allowed(allowed, len(self))
        if q.shape[0] == 0:
            return np.zeros(1, np.uint64), np.empty(0, np.uint32), np.empty(0, np.float32)
        return self._handle().range_search_masked(q, p, r, m, w).read()

    def range_search_device(self, dev_queries: int, nq: int, radius, nprobe: int = 8, max_results: int = DEFAULT_MAX_RESULTS,
                            dev_allowed: int | None = None):
        """`IVFRangeMixin.range_search_device`; `dev_allowed`: the row mask's words at a device pointer (4-byte aligned)"""
        if dev_allowed is None:
            return super().range_search_device(dev_queries, nq, radius, nprobe, max_results)
        n_q = _nq(nq)
        r = _radii(radius, n_q)
        p = self._nprobe(nprobe)
        m = _max_results(max_results)
        return self._handle().range_search_masked_device(int(dev_queries), n_q, p, r, m, int(dev_allowed))
