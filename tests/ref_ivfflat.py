"""numpy statement of the inverted-file flat search of include/vqhip.h (vqhip_ivfflat_*, vq_amd.IVFFlatIndex).

P(q)    = the nprobe nearest coarse centroids by the exact k-NN statement (ref_ivf.probe: ref_knn's search over C),
S(q)    = the rows whose list is in P(q), in ascending row id,
D(q, i) = ref_knn.distances: Distance::compute over the rows widened to f32, the row norms computed once,
result  = the topk of S(q) by (key(D), row id) (ref_knn.topk_of: NaN last and canonical, ties to the lower row, Euclidean
          ordered by the reported root), padded with (0xFFFFFFFF, +inf) up to topk."""
import numpy as np

import ref_ivf as I
import ref_knn as K

F = np.float32
PAD_ID = I.PAD_ID


def probe(metric, coarse, Q, nprobe):
    """(nq, nprobe) uint32: P(q) per query, nearest first"""
    return I.probe(metric, coarse, Q, nprobe)


def search(metric, coarse, lists, rows, Q, nprobe, topk, queries=None):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)); rows f32 or f16 (widened exactly); queries: the subset of query
    numbers to evaluate (the others' slots are left as padding)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(rows).astype(F)
    lists = np.asarray(lists)
    P = probe(metric, coarse, Q, nprobe)
    xn = K.norms(X) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in (range(Q.shape[0]) if queries is None else queries):
        S = I.members(lists, P[j])
        t = min(topk, S.size)
        if t:
            D = K.distances(metric, Q[j], X[S], None if xn is None else xn[S])
            idx[j, :t], dist[j, :t] = K.topk_of(D, S, t)
    return idx, dist
