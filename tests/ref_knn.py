"""numpy statement of the exact k-NN semantics of include/vqhip.h (vqhip_flat_*, vq_amd.FlatIndex).

D(q, i) = Distance::compute(q, rows[i]): every pair summed sequentially over t = 0..d-1 from -0.0 in f32, one rounding
per operation, no fused multiply-add -- vectorised here over the rows, one column at a time (numpy's f32 scalar-array
operations round once each).  The result of a search is the topk rows by (key(D), row) ascending, key being the ADC
search's order-preserving map (NaN last); a NaN distance is reported as 0x7FC00000."""
import numpy as np

F = np.float32
SQUARED_EUCLIDEAN, EUCLIDEAN, MANHATTAN, COSINE, COSINE_UNCLAMPED = 0, 1, 2, 3, 4
METRICS = (SQUARED_EUCLIDEAN, EUCLIDEAN, MANHATTAN, COSINE, COSINE_UNCLAMPED)
NAN_BITS = np.uint32(0x7FC00000)


def norms(X):
    """sqrtf(sum_t x_t^2) per row, sequential from -0.0"""
    X = np.asarray(X, F)
    s = np.full(X.shape[0], -0.0, F)
    with np.errstate(all="ignore"):
        for t in range(X.shape[1]):
            c = X[:, t]
            s = s + c * c
        return np.sqrt(s)


def cosine_finish(metric, dot, na, nb):
    """vq_cosine_finish, vectorised (the EPSILON rule, then f32::clamp, which keeps NaN)"""
    dot, na, nb = (np.asarray(v, F) for v in (dot, na, nb))
    with np.errstate(all="ignore"):
        v = F(1.0) - dot / (na * nb)
        if metric == COSINE_UNCLAMPED:
            return v.astype(F)
        v = np.where(v < 0, F(0), np.where(v > 1, F(1), v))
        return np.where((na < F(1e-10)) | (nb < F(1e-10)), F(1), v).astype(F)


def distances(metric, q, X, xnorm=None):
    """D(q, i) for every row of X (n, d) f32 (f16 rows: widen first); xnorm: norms(X), computed when None"""
    q = np.asarray(q, F)
    X = np.asarray(X, F)
    acc = np.full(X.shape[0], -0.0, F)
    with np.errstate(all="ignore"):
        for t in range(X.shape[1]):
            if metric in (SQUARED_EUCLIDEAN, EUCLIDEAN):
                diff = q[t] - X[:, t]
                acc = acc + diff * diff
            elif metric == MANHATTAN:
                acc = acc + np.abs(q[t] - X[:, t])
            else:
                acc = acc + q[t] * X[:, t]
        if metric == EUCLIDEAN:
            return np.sqrt(acc)
    if metric in (COSINE, COSINE_UNCLAMPED):
        return cosine_finish(metric, acc, norms(q[None, :])[0], norms(X) if xnorm is None else xnorm)
    return acc


def key(d):
    """the order-preserving uint32 key (topk.hpp adc_key): NaN -> 0xFFFFFFFF"""
    b = np.asarray(d, F).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def reported(d):
    """the distance as the search reports it: NaN canonicalised"""
    b = np.asarray(d, F).view(np.uint32).copy()
    b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = NAN_BITS
    return b.view(F)


def topk_of(d, rows, topk):
    """the topk of distances d over row ids `rows` by (key, row): (idx uint32, dist f32 as reported)"""
    rows = np.asarray(rows, np.uint64)
    comp = (key(d).astype(np.uint64) << np.uint64(32)) | rows  # (key, row) in one word: rows < 2^32
    if topk < comp.size:
        comp = np.partition(comp, topk - 1)[:topk]
    comp = np.sort(comp)[:topk]
    k = (comp >> np.uint64(32)).astype(np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)  # adc_unkey
    b[k == np.uint32(0xFFFFFFFF)] = NAN_BITS
    return (comp & np.uint64(0xFFFFFFFF)).astype(np.uint32), b.view(F)


def search(metric, Q, X, topk):
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    xn = norms(X) if metric in (COSINE, COSINE_UNCLAMPED) else None
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    rows = np.arange(X.shape[0])
    for j, q in enumerate(Q):
        idx[j], dist[j] = topk_of(distances(metric, q, X, xn), rows, topk)
    return idx, dist


def rerank(metric, Q, X, cand, topk):
    Q = np.atleast_2d(np.asarray(Q, F))
    X = np.asarray(X, F)
    idx = np.empty((Q.shape[0], topk), np.uint32)
    dist = np.empty((Q.shape[0], topk), F)
    for j, q in enumerate(Q):
        c = np.asarray(cand[j], np.int64)
        idx[j], dist[j] = topk_of(distances(metric, q, X[c]), c, topk)
    return idx, dist


def special_rows(d, rng):
    """rows that exercise the corners: zeros, NaN, +-inf, huge, tiny, negative zero"""
    rows = [np.zeros(d, F), np.full(d, -0.0, F), np.full(d, F(3e38)), np.full(d, F(1e-30)), np.full(d, F(1e-45))]
    r = rng.standard_normal(d).astype(F)
    r[d // 2] = np.nan
    rows.append(r)
    r = rng.standard_normal(d).astype(F)
    r[0] = np.inf
    rows.append(r)
    r = rng.standard_normal(d).astype(F)
    r[-1] = -np.inf
    rows.append(r)
    return np.stack(rows)
