"""numpy statement of the filtered PQ searches of include/vqhip.h (vqhip_ivfpq_search_masked, vqhip_pq_adc_search_masked
and their siblings; ``IVFPQIndex.masked_search``, ``PQIndex.search(..., allowed=)``, ``ProductQuantizer.search(..., allowed=)``).

The mask is ref_filter's: a bool array m (n,), row i allowed iff m[i]; its words are ref_filter.pack(m).
P(q)     = ref_ivf.probe: the nprobe nearest coarse centroids -- the mask plays no part in it,
S_a(q)   = ref_ivf_filter.allowed_members: the allowed rows whose list is in P(q), in ascending row id,
plain    = the oracle's ADC search over codes[S_a(q)], ids mapped back through S_a(q) (ref_ivf.search's argument: the ADC
           order breaks ties by position and S_a(q) is ascending), padded with (0xFFFFFFFF, +inf),
residual = ref_ivf_residual's per-list form over the allowed rows of each probed list, merged by (key, row id),
dense    = the oracle's ADC search over codes[m], ids mapped back through the allowed rows, padded.
`brute_*` restate each without the oracle (ref_ivf.adc_distances / ref_ivf_residual.distances, then (key, row) over the
allowed rows).  It makes no arithmetic of its own."""
import numpy as np

import ref_ivf as R
import ref_ivf_filter as RIF
import ref_ivf_residual as RR
import ref_knn as K

F = np.float32
PAD_ID = R.PAD_ID


def search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask, queries=None):
    """IVFPQIndex(...).masked_search(Q, mask, topk, nprobe); queries: the subset of query numbers to evaluate (the others'
    slots are left as padding)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    codes = np.asarray(codes)
    P = R.probe(metric, coarse, Q, nprobe)
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in (range(Q.shape[0]) if queries is None else queries):
        S = RIF.allowed_members(lists, P[j], mask)
        t = min(topk, S.size)
        if t:
            ii, dd = orc.adc_search(metric, cb, codes[S], Q[j][None, :], t)
            idx[j], dist[j] = R._pad(S[ii[0].astype(np.int64)].astype(np.uint32), dd[0], topk)
    return idx, dist


def brute_search(metric, coarse, cb, lists, codes, Q, nprobe, topk, mask):
    Q = np.atleast_2d(np.asarray(Q, F))
    P = R.probe(metric, coarse, Q, nprobe)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        D = R.adc_distances(metric, cb, codes, q)
        S = RIF.allowed_members(lists, P[j], mask)
        t = min(topk, S.size)
        ii, dd = K.topk_of(D[S], S, t) if t else (np.empty(0, np.uint32), np.empty(0, F))
        idx[j], dist[j] = RR._finish(metric, ii, dd, topk)
    return idx, dist


def residual_search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask, queries=None):
    """IVFPQIndex(..., residual=True).masked_search(Q, mask, topk, nprobe)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    coarse = np.asarray(coarse, F)
    lists = np.asarray(lists)
    codes = np.asarray(codes)
    P = R.probe(metric, coarse, Q, nprobe)
    inner = K.SQUARED_EUCLIDEAN if metric == K.EUCLIDEAN else metric
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in (range(Q.shape[0]) if queries is None else queries):
        rows, ds = [], []
        for l in P[j]:
            S = RIF.allowed_members(lists, [l], mask)
            t = min(topk, S.size)
            if t:
                ii, dd = orc.adc_search(inner, cb, codes[S], RR.residual(Q[j], coarse[l])[None, :], t)
                rows.append(S[ii[0].astype(np.int64)])
                ds.append(dd[0])
        if rows:
            r = np.concatenate(rows)
            ii, dd = K.topk_of(np.concatenate(ds), r, min(topk, r.size))
        else:
            ii, dd = np.empty(0, np.uint32), np.empty(0, F)
        idx[j], dist[j] = RR._finish(metric, ii, dd, topk)
    return idx, dist


def brute_residual_search(metric, coarse, cb, lists, codes, Q, nprobe, topk, mask):
    Q = np.atleast_2d(np.asarray(Q, F))
    P = R.probe(metric, coarse, Q, nprobe)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        S = RIF.allowed_members(lists, P[j], mask)
        t = min(topk, S.size)
        if t:
            ii, dd = K.topk_of(RR.distances(metric, coarse, cb, lists, codes, q, S), S, t)
        else:
            ii, dd = np.empty(0, np.uint32), np.empty(0, F)
        idx[j], dist[j] = RR._finish(metric, ii, dd, topk)
    return idx, dist


def ivf_search(orc, residual, *args, **kw):
    return (residual_search if residual else search)(orc, *args, **kw)


def dense_search(orc, metric, cb, codes, Q, topk, mask):
    """PQIndex(cb, codes).search(Q, topk, allowed=mask)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    S = np.flatnonzero(np.asarray(mask, np.bool_)).astype(np.int64)
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    t = min(topk, S.size)
    if t and Q.shape[0]:
        ii, dd = orc.adc_search(metric, cb, np.asarray(codes)[S], Q, t)
        idx[:, :t] = S[ii.astype(np.int64)].astype(np.uint32)
        dist[:, :t] = dd
    return idx, dist


def brute_dense_search(metric, cb, codes, Q, topk, mask):
    Q = np.atleast_2d(np.asarray(Q, F))
    S = np.flatnonzero(np.asarray(mask, np.bool_)).astype(np.int64)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        t = min(topk, S.size)
        ii, dd = K.topk_of(R.adc_distances(metric, cb, codes, q)[S], S, t) if t else (np.empty(0, np.uint32), np.empty(0, F))
        idx[j], dist[j] = RR._finish(metric, ii, dd, topk)
    return idx, dist
