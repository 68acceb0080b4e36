"""numpy statement of the inverted-file range search of include/vqhip.h (vqhip_ivfflat_range_search,
vqhip_ivfsq_range_search, vq_amd.IVFFlatIndex.range_search, vq_amd.IVFScalarIndex.range_search).

P(q)    = ref_ivfflat.probe: the nprobe nearest coarse centroids,
S(q)    = the rows whose list is in P(q), in ascending row id (ref_ivf.members),
D(q, i) = ref_knn.distances over the rows widened to f32 (the scalar index: over the rows ref_sqindex.decode gives),
hit     = ref_range.hits: D(q, i) <= r_q as a float32 comparison; NaN never hits, -0.0 <= 0.0 holds,
result  = CSR as ref_range.search: lims uint64 (nq + 1,), idx uint32 ROW IDS ascending within a query, dist the bits of D.
It makes no arithmetic of its own."""
import numpy as np

import ref_ivf as I
import ref_ivfflat as IF
import ref_knn as K
import ref_range as R
import ref_sqindex as SI

F = np.float32


def search(metric, coarse, lists, rows, Q, nprobe, radius):
    """IVFFlatIndex.range_search(Q, radius, nprobe): rows f32 or f16 (widened exactly)"""
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
        S = I.members(lists, P[j])
        if S.size:
            i, d = R.hits(K.distances(metric, q, X[S], None if xn is None else xn[S]), r[j])
            idx.append(S[i].astype(np.uint32))
            dist.append(d)
        lims[j + 1] = lims[j] + np.uint64(idx[-1].size if S.size else 0)
    return lims, np.concatenate(idx), np.concatenate(dist)


def sq_search(metric, coarse, lists, sq, codes, Q, nprobe, radius):
    """IVFScalarIndex.range_search for sq = (min, max, levels) and codes uint8 (n, dim): the same over the decoded rows"""
    return search(metric, coarse, lists, SI.decode(sq, codes), Q, nprobe, radius)
