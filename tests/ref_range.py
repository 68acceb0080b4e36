"""numpy statement of the exact range search of include/vqhip.h (vqhip_flat_range_search, vqhip_sqindex_range_search,
vq_amd.FlatIndex.range_search, vq_amd.ScalarIndex.range_search).

Per query q with radius r: d = the distances of tests/ref_knn.py (Distance::compute bit for bit), row i is a hit iff
d[i] <= r as a float32 comparison -- NaN never hits, -0.0 <= 0.0 holds -- and the hits come in ascending row id.  The
result is CSR: lims uint64 (nq + 1,) with lims[0] = 0, idx uint32 (total,), dist float32 (total,), the bits of d."""
import numpy as np

import ref_knn as K
import ref_sqindex as SI

F = np.float32


def hits(d, r):
    """(idx uint32, dist f32) of one query from its distances d and its radius r"""
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        hit = d <= F(r)
    return np.nonzero(hit)[0].astype(np.uint32), d[hit]


def radii(radius, nq):
    r = np.asarray(radius, F)
    return np.full(nq, r, F) if r.ndim == 0 else r


def search(metric, Q, X, radius):
    """FlatIndex(X).range_search(Q, radius): f16 rows are widened by the caller"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    r = radii(radius, Q.shape[0])
    assert r.shape == (Q.shape[0],) and not np.isnan(r).any()
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    lims = np.zeros(Q.shape[0] + 1, np.uint64)
    idx, dist = [], []
    for j, q in enumerate(Q):
        i, d = hits(K.distances(metric, q, X, xn), r[j])
        idx.append(i)
        dist.append(d)
        lims[j + 1] = lims[j] + np.uint64(i.size)
    return lims, np.concatenate(idx + [np.empty(0, np.uint32)]), np.concatenate(dist + [np.empty(0, F)])


def sq_search(metric, Q, sq, codes, radius):
    """ScalarIndex.from_codes(codes, ScalarQuantizer(*sq)).range_search(Q, radius): the same over the dequantized rows"""
    return search(metric, Q, SI.decode(sq, codes), radius)


def search_kth(metric, Q, X, k):
    """(radii, result) with radii[q] = the k-th smallest distance of query q and result = search(metric, Q, X, radii), from
    one pass over the distances (large cases)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    r = np.empty(Q.shape[0], F)
    lims = np.zeros(Q.shape[0] + 1, np.uint64)
    idx, dist = [], []
    for j, q in enumerate(Q):
        d = K.distances(metric, q, X, xn)
        kk = np.partition(K.key(d), k - 1)[k - 1]
        assert kk != np.uint32(0xFFFFFFFF), "fewer than k distances that are not NaN"
        r[j] = np.array([kk & np.uint32(0x7FFFFFFF) if kk & np.uint32(0x80000000) else ~kk], np.uint32).view(F)[0]  # adc_unkey
        i, dd = hits(d, r[j])
        idx.append(i)
        dist.append(dd)
        lims[j + 1] = lims[j] + np.uint64(i.size)
    return r, (lims, np.concatenate(idx), np.concatenate(dist))


def kth_distance(metric, Q, X, k):
    """per query the k-th smallest distance by key (NaN last), as float32: a radius with ties exactly on the boundary"""
    Q = np.atleast_2d(np.asarray(Q, F))
    _, dist = K.search(metric, Q, X, k)
    return dist[:, k - 1].copy()
