"""numpy statement of the asymmetric binary index (include/vqhip.h vqhip_abin_*, vq_amd.AsymmetricBinaryIndex): the
packed words unpacked to bits, the bits decoded by the BQ rule v(bit) = float32(high) if bit else float32(low), then the
exact-distance statement of tests/ref_knn.py over the decoded rows.  The queries are f32 and never quantized.

A call's distances are computed once (``distance_matrix``) and shared by the statements of search, filtered search, range
search and rerank over them (``topk``, ``ranged``, ``rerank``)."""
import numpy as np

import ref_knn as K

F = np.float32
METRICS = K.METRICS
PAD_IDX = np.uint32(0xFFFFFFFF)

# (low, high) of the GPU cases: the default, a pair whose squares and sums round, and the widest
LOW_HIGH = [(0, 1), (3, 200), (0, 255)]


def words_per_row(d: int) -> int:
    return (d + 31) // 32


def pack(bits) -> np.ndarray:
    """bool (n, d) -> uint32 (n, W): dimension t is bit t % 32 of word t // 32, pad bits zero"""
    b = np.asarray(bits, np.bool_)
    n, d = b.shape
    padded = np.zeros((n, 32 * words_per_row(d)), np.bool_)
    padded[:, :d] = b
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, words_per_row(d))


def unpack(words, d: int) -> np.ndarray:
    """uint32 (n, W) -> bool (n, d)"""
    w = np.ascontiguousarray(np.asarray(words, "<u4"))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :d].astype(np.bool_)


def decode(words, d: int, low: int, high: int) -> np.ndarray:
    """the dequantized rows, float32 (n, d)"""
    return np.where(unpack(words, d), F(high), F(low)).astype(F)


def distance_matrix(metric, Q, words, d, low, high) -> np.ndarray:
    """D(q, i) for every query and row, float32 (nq, n)"""
    Q = np.atleast_2d(np.asarray(Q, F))
    V = decode(words, d, low, high)
    vn = K.norms(V) if metric in (K.COSINE, K.COSINE_UNCLAMPED) else None
    return np.stack([K.distances(metric, q, V, vn) for q in Q])


def topk(D, k, mask=None):
    """the search over distances D (nq, n): per query the k rows by (key(D), row) among the rows of `mask` (bool (n,);
    None: all), padded with (0xFFFFFFFF, +inf) behind fewer than k of them"""
    rows = np.arange(D.shape[1]) if mask is None else np.flatnonzero(np.asarray(mask, np.bool_))
    idx = np.full((D.shape[0], k), PAD_IDX, np.uint32)
    dist = np.full((D.shape[0], k), np.inf, F)
    kk = min(k, rows.size)
    if kk:
        for j in range(D.shape[0]):
            idx[j, :kk], dist[j, :kk] = K.topk_of(D[j, rows], rows, kk)
    return idx, dist


def ranged(D, radii, mask=None):
    """the range search over distances D (nq, n): CSR (lims, idx, dist), row i a hit of query q iff it is allowed and
    D[q, i] <= radii[q] as a float32 comparison, ascending row id"""
    m = np.ones(D.shape[1], np.bool_) if mask is None else np.asarray(mask, np.bool_)
    lims = np.zeros(D.shape[0] + 1, np.uint64)
    idx, dist = [], []
    for j in range(D.shape[0]):
        with np.errstate(invalid="ignore"):
            hit = m & (D[j] <= F(radii[j]))
        idx.append(np.flatnonzero(hit).astype(np.uint32))
        dist.append(D[j, hit])
        lims[j + 1] = lims[j] + np.uint64(idx[-1].size)
    return lims, np.concatenate(idx + [np.empty(0, np.uint32)]), np.concatenate(dist + [np.empty(0, F)])


def rerank(D, cand, k):
    """per query the k nearest of its candidate rows cand (nq, c) by (key(D), row)"""
    idx = np.empty((D.shape[0], k), np.uint32)
    dist = np.empty((D.shape[0], k), F)
    for j in range(D.shape[0]):
        c = np.asarray(cand[j], np.int64)
        idx[j], dist[j] = K.topk_of(D[j, c], c, k)
    return idx, dist


def search(metric, Q, words, d, low, high, k):
    return topk(distance_matrix(metric, Q, words, d, low, high), k)
