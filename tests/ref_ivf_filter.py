"""numpy statement of the filtered inverted-file searches of include/vqhip.h (vqhip_ivfflat_*_masked, vqhip_ivfsq_*_masked,
``IVFFlatIndex`` / ``IVFScalarIndex`` ``.search(..., allowed=)`` and ``.range_search(..., allowed=)``).

The mask is ref_filter's: a bool array m (n,), row i allowed iff m[i]; its words are ref_filter.pack(m).
P(q)    = ref_ivfflat.probe: the nprobe nearest coarse centroids -- the mask plays no part in it,
S_a(q)  = the allowed rows whose list is in P(q), in ascending row id: ref_ivf.members, then m,
D(q, i) = ref_knn.distances over the rows widened to f32 (the scalar index: over the rows ref_sqindex.decode gives),
top-k   = ref_knn.topk_of over S_a(q): (key(D), row id) ascending, NaN last and canonical, padded with (0xFFFFFFFF, +inf),
range   = ref_range.hits over S_a(q): D(q, i) <= r_q as a float32 comparison, CSR in ascending row id.
It makes no arithmetic of its own."""
import numpy as np

import ref_ivf as I
import ref_ivfflat as IF
import ref_knn as K
import ref_range as R
import ref_sqindex as SI

F = np.float32
PAD_ID = IF.PAD_ID


def allowed_members(lists, probed, mask):
    """S_a(q): the allowed rows of the probed lists, ascending"""
    S = I.members(lists, probed)
    return S[np.asarray(mask, np.bool_)[S]]


def search(metric, coarse, lists, rows, Q, nprobe, topk, mask, queries=None):
    """IVFFlatIndex.search(Q, topk, nprobe, allowed=mask): rows f32 or f16 (widened exactly); queries: the subset of
    query numbers to evaluate (the others' slots are left as padding)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(rows).astype(F)
    lists = np.asarray(lists)
    P = IF.probe(metric, coarse, Q, nprobe)
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in (range(Q.shape[0]) if queries is None else queries):
        S = allowed_members(lists, P[j], mask)
        t = min(topk, S.size)
        if t:
            D = K.distances(metric, Q[j], X[S], None if xn is None else xn[S])
            idx[j, :t], dist[j, :t] = K.topk_of(D, S, t)
    return idx, dist


def range_search(metric, coarse, lists, rows, Q, nprobe, radius, mask):
    """IVFFlatIndex.range_search(Q, radius, nprobe, allowed=mask)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(rows).astype(F)
    lists = np.asarray(lists)
    r = R.radii(radius, Q.shape[0])
    assert r.shape == (Q.shape[0],) and not np.isnan(r).any()
    P = IF.probe(metric, coarse, Q, nprobe) if Q.shape[0] else np.empty((0, nprobe), np.uint32)
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    lims = np.zeros(Q.shape[0] + 1, np.uint64)
    idx, dist = [np.empty(0, np.uint32)], [np.empty(0, F)]
    for j, q in enumerate(Q):
        S = allowed_members(lists, P[j], mask)
        got = 0
        if S.size:
            i, d = R.hits(K.distances(metric, q, X[S], None if xn is None else xn[S]), r[j])
            idx.append(S[i].astype(np.uint32))
            dist.append(d)
            got = idx[-1].size
        lims[j + 1] = lims[j] + np.uint64(got)
    return lims, np.concatenate(idx), np.concatenate(dist)


def sq_search(metric, coarse, lists, sq, codes, Q, nprobe, topk, mask, queries=None):
    """IVFScalarIndex.search for sq = (min, max, levels) and codes uint8 (n, dim): the same over the decoded rows"""
    return search(metric, coarse, lists, SI.decode(sq, codes), Q, nprobe, topk, mask, queries)


def sq_range_search(metric, coarse, lists, sq, codes, Q, nprobe, radius, mask):
    return range_search(metric, coarse, lists, SI.decode(sq, codes), Q, nprobe, radius, mask)
