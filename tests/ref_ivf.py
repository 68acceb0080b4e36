"""numpy statement of the inverted-file PQ search of include/vqhip.h (vqhip_ivfpq_*, vq_amd.IVFPQIndex).

P(q)    = the nprobe nearest coarse centroids by the exact k-NN statement (ref_knn: Distance::compute, (key, list id)),
S(q)    = the rows whose list is in P(q), in ascending row id,
result  = the oracle's ADC search over the codes of S(q), ids mapped back through S(q) -- valid because the ADC order
          breaks ties by position and S(q) is ascending, so position order is row order -- then padded with
          (0xFFFFFFFF, +inf) up to topk.
`brute_search` restates the same thing without the oracle (tables and sums in numpy) to check the statement."""
import numpy as np

import ref_knn as K

F = np.float32
PAD_ID = np.uint32(0xFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)


def probe(metric, coarse, Q, nprobe):
    """(nq, nprobe) uint32: P(q) per query, nearest first"""
    return K.search(metric, Q, coarse, nprobe)[0]


def members(lists, P_q):
    """S(q): ascending row ids whose list is one of P_q"""
    return np.flatnonzero(np.isin(np.asarray(lists), np.asarray(P_q, np.int64))).astype(np.int64)


def _pad(idx, dist, topk):
    out_i = np.full(topk, PAD_ID, np.uint32)
    out_d = np.full(topk, np.inf, F)
    out_i[:idx.size] = idx
    out_d[:dist.size] = dist
    return out_i, out_d


def search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)) by the oracle's ADC search over each S(q)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    P = probe(metric, coarse, Q, nprobe)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        S = members(lists, P[j])
        t = min(topk, S.size)
        if t:
            ii, dd = orc.adc_search(metric, cb, np.asarray(codes)[S], q[None, :], t)
            idx[j], dist[j] = _pad(S[ii[0].astype(np.int64)].astype(np.uint32), dd[0], topk)
        else:
            idx[j], dist[j] = _pad(np.empty(0, np.uint32), np.empty(0, F), topk)
    return idx, dist


def tables(metric, cb, q):
    """t[s][j]: the per-subspace term between q's sub-vector s and centroid j (distance2 from -0.0, L1 from 0.0)"""
    cb = np.asarray(cb, F)
    m, k, sd = cb.shape
    q = np.asarray(q, F).reshape(m, sd)
    t = np.empty((m, k), F)
    with np.errstate(all="ignore"):
        for s in range(m):
            acc = np.full(k, 0.0 if metric == K.MANHATTAN else -0.0, F)
            for u in range(sd):
                diff = q[s, u] - cb[s, :, u]
                acc = acc + (np.abs(diff) if metric == K.MANHATTAN else diff * diff)
            t[s] = acc
    return t


def adc_distances(metric, cb, codes, q):
    """D(q, i) for every row of codes (n, m): the table terms summed in subspace order in f32"""
    t = tables(metric, cb, q)
    codes = np.asarray(codes, np.int64)
    with np.errstate(all="ignore"):
        acc = t[0][codes[:, 0]]
        for s in range(1, codes.shape[1]):
            acc = acc + t[s][codes[:, s]]
    return acc.astype(F)


def brute_search(metric, coarse, cb, lists, codes, Q, nprobe, topk):
    """the same result, restated: every row's D and list membership, then (key, row) over S(q)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    P = probe(metric, coarse, Q, nprobe)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        D = adc_distances(metric, cb, codes, q)
        S = members(lists, P[j])
        t = min(topk, S.size)
        ii, dd = K.topk_of(D[S], S, t) if t else (np.empty(0, np.uint32), np.empty(0, F))
        if metric == K.EUCLIDEAN:
            with np.errstate(all="ignore"):
                dd = np.sqrt(dd)  # ordered by the squared sum, reported as the root
            dd = K.reported(dd)
        idx[j], dist[j] = _pad(ii, dd, topk)
    return idx, dist
