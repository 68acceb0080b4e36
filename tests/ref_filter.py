"""numpy statement of the filtered search of include/vqhip.h (vqhip_*_search_masked, vqhip_*_range_search_masked,
``FlatIndex`` / ``ScalarIndex`` ``.search(..., allowed=)`` and ``.range_search(..., allowed=)``).

A row mask of n rows is a bool array m (n,): row i is allowed iff m[i].  Its words are ``pack(m)``: np.packbits in
little bit order, zero-padded to whole uint32 words, read little-endian.
  masked top-k   the distances of tests/ref_knn.py, then ref_knn.topk_of over np.flatnonzero(m) -- (key(D), row) ascending,
                 NaN last as 0x7FC00000, ties to the lower allowed row -- padded with (0xFFFFFFFF, +inf) behind fewer than
                 topk allowed rows
  masked range   row i is a hit iff m[i] and D(q, i) <= radius[q] as a float32 comparison, in ascending row id (CSR as
                 tests/ref_range.py)
The scalar forms decode the codes by tests/ref_sqindex.py first."""
import numpy as np

import ref_knn as K
import ref_range as R
import ref_sqindex as SI

F = np.float32
PAD_IDX = np.uint32(0xFFFFFFFF)


def pack(mask) -> np.ndarray:
    """bool (n,) -> uint32 (ceil(n / 32),)"""
    m = np.asarray(mask, np.bool_)
    by = np.packbits(m, bitorder="little")
    out = np.zeros((m.shape[0] + 31) // 32 * 4, np.uint8)
    out[:by.shape[0]] = by
    return out.view("<u4").astype(np.uint32)


def unpack(words, n) -> np.ndarray:
    """uint32 words -> bool (n,): the bits at or past n are dropped"""
    by = np.asarray(words, "<u4").view(np.uint8)
    return np.unpackbits(by, bitorder="little")[:n].astype(np.bool_)


def search(metric, Q, X, topk, mask):
    """FlatIndex(X).search(Q, topk, allowed=mask): f16 rows are widened by the caller"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    rows = np.flatnonzero(np.asarray(mask, np.bool_))
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    idx = np.full((Q.shape[0], topk), PAD_IDX, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    k = min(topk, rows.size)
    if k:
        for j, q in enumerate(Q):
            idx[j, :k], dist[j, :k] = K.topk_of(K.distances(metric, q, X, xn)[rows], rows, k)
    return idx, dist


def range_search(metric, Q, X, radius, mask):
    """FlatIndex(X).range_search(Q, radius, allowed=mask)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    m = np.asarray(mask, np.bool_)
    r = R.radii(radius, Q.shape[0])
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    lims = np.zeros(Q.shape[0] + 1, np.uint64)
    idx, dist = [], []
    for j, q in enumerate(Q):
        d = K.distances(metric, q, X, xn)
        with np.errstate(invalid="ignore"):
            hit = m & (d <= r[j])
        idx.append(np.flatnonzero(hit).astype(np.uint32))
        dist.append(d[hit])
        lims[j + 1] = lims[j] + np.uint64(idx[-1].size)
    return lims, np.concatenate(idx + [np.empty(0, np.uint32)]), np.concatenate(dist + [np.empty(0, F)])


def sq_search(metric, Q, sq, codes, topk, mask):
    return search(metric, Q, SI.decode(sq, codes), topk, mask)


def sq_range_search(metric, Q, sq, codes, radius, mask):
    return range_search(metric, Q, SI.decode(sq, codes), radius, mask)
