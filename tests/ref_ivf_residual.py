"""numpy statement of the residual inverted-file PQ search of include/vqhip.h (VQHIP_IVF_RESIDUAL,
vq_amd.IVFPQIndex(..., residual=True)).

P(q) and S(q) are those of the non-residual index (ref_ivf).  A row of list l holds the codes of x - C[l], so its
distance is the ADC distance of its codes to r = q - C[l] (f32, one rounding per element).

`search`       = per probed list l, the oracle's ADC search over that list's rows with r as the query (its topk
                 by (key, position): positions ascend with row ids), merged over the lists by (key, row id) and padded
                 with (0xFFFFFFFF, +inf).  Euclidean is searched as squared Euclidean (the same D) and reported as the
                 root, so that the merge orders by D.
`brute_search` = the same without the oracle: every row of S(q) gets D from numpy tables of its list's residual.
`encode`       = what IVFPQIndex.add stores: the oracle's coarse encode, then pq_encode of X - C[list]."""
import numpy as np

import ref_ivf as R
import ref_knn as K

F = np.float32
PAD_ID = R.PAD_ID
INF_BITS = R.INF_BITS


def residual(q, c):
    """q - c in f32, one rounding per element"""
    with np.errstate(all="ignore"):
        return (np.asarray(q, F) - np.asarray(c, F)).astype(F)


def _finish(metric, idx, dist, topk):
    if metric == K.EUCLIDEAN:
        with np.errstate(all="ignore"):
            dist = K.reported(np.sqrt(dist))  # ordered by the squared sum, reported as the root
    return R._pad(idx, dist, topk)


def search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)) by the oracle's ADC search over each probed list"""
    Q = np.atleast_2d(np.asarray(Q, F))
    coarse = np.asarray(coarse, F)
    lists = np.asarray(lists)
    codes = np.asarray(codes)
    P = R.probe(metric, coarse, Q, nprobe)
    inner = K.SQUARED_EUCLIDEAN if metric == K.EUCLIDEAN else metric
    order = np.argsort(lists, kind="stable")  # the rows of list l: order[off[l]:off[l + 1]], ascending
    off = np.concatenate([[0], np.cumsum(np.bincount(lists, minlength=coarse.shape[0]))])
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        rows, ds = [], []
        for l in P[j]:
            S = order[off[l]:off[l + 1]]
            t = min(topk, S.size)
            if t:
                ii, dd = orc.adc_search(inner, cb, codes[S], residual(q, coarse[l])[None, :], t)
                rows.append(S[ii[0].astype(np.int64)])
                ds.append(dd[0])
        if rows:
            r = np.concatenate(rows)
            ii, dd = K.topk_of(np.concatenate(ds), r, min(topk, r.size))
        else:
            ii, dd = np.empty(0, np.uint32), np.empty(0, F)
        idx[j], dist[j] = _finish(metric, ii, dd, topk)
    return idx, dist


def distances(metric, coarse, cb, lists, codes, q, rows):
    """D(q, i) for the given rows: the tables of r = q - C[list[i]] (ref_ivf.tables), summed in subspace order"""
    coarse = np.asarray(coarse, F)
    lists = np.asarray(lists)
    rows = np.asarray(rows, np.int64)
    D = np.empty(rows.size, F)
    for l in np.unique(lists[rows]):
        at = np.flatnonzero(lists[rows] == l)
        D[at] = R.adc_distances(metric, cb, np.asarray(codes)[rows[at]], residual(q, coarse[l]))
    return D


def brute_search(metric, coarse, cb, lists, codes, Q, nprobe, topk):
    """the same result, restated: every row of S(q) with its list's residual tables, then (key, row)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    P = R.probe(metric, coarse, Q, nprobe)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        S = R.members(lists, P[j])
        t = min(topk, S.size)
        if t:
            D = distances(metric, coarse, cb, lists, codes, q, S)
            ii, dd = K.topk_of(D, S, t)  # (D is the squared sum for Euclidean)
        else:
            ii, dd = np.empty(0, np.uint32), np.empty(0, F)
        idx[j], dist[j] = _finish(metric, ii, dd, topk)
    return idx, dist


def encode(orc, metric, coarse, cb, X):
    """(list ids uint32 (n,), codes (n, m)): the nearest coarse centroid, then the PQ codes of X - C[list]"""
    coarse = np.asarray(coarse, F)
    X = np.asarray(X, F)
    lists, _ = orc.pq_encode(metric, X, coarse[None, :, :], want_f16=False)
    lists = np.asarray(lists).reshape(-1).astype(np.int64)
    codes, _ = orc.pq_encode(metric, residual(X, coarse[lists]), cb, want_f16=False)
    return lists.astype(np.uint32), codes


def reconstruct(coarse, cb, lists, codes):
    """C[list] + the decoded codes, in f32"""
    cb = np.asarray(cb, F)
    m = cb.shape[0]
    codes = np.asarray(codes, np.int64)
    dec = np.concatenate([cb[s][codes[:, s]] for s in range(m)], axis=1)
    return (np.asarray(coarse, F)[np.asarray(lists, np.int64)] + dec).astype(F)
