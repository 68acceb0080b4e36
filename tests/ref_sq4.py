"""numpy statement of the 4-bit scalar index (include/vqhip.h vqhip_sq4index_*, vq_amd.Scalar4Index): the packed words
unpacked to codes, the codes decoded by the SQ rule v(c) = min + float32(c) * step (two roundings), then the
exact-distance statement of tests/ref_knn.py over the decoded rows.  The queries are f32 and never quantized.

A call's distances are computed once (``distance_matrix``) and shared by the statements of search, filtered search, range
search and rerank over them (``topk``, ``ranged``, ``rerank``: those of tests/ref_abin.py, which read only distances)."""
import numpy as np

import ref_abin as A
import ref_knn as K

F = np.float32
METRICS = K.METRICS

# (min, max, levels) of the GPU cases: a step that rounds, integer values, few levels with codes far above them, two levels
QUANTIZERS = [(-1.0, 1.0, 16), (0.0, 15.0, 16), (-3.5, 200.0, 5), (0.0, 1.0, 2)]

topk, ranged, rerank = A.topk, A.ranged, A.rerank


def words_per_row(d: int) -> int:
    return (d + 7) // 8


def pack4(codes) -> np.ndarray:
    """uint8 (n, d), each <= 15 -> uint32 (n, W): dimension t is bits 4 (t % 8) .. + 3 of word t // 8, pad nibbles zero"""
    c = np.asarray(codes, np.uint8)
    assert c.ndim == 2 and (c.size == 0 or int(c.max()) <= 15)
    n, d = c.shape
    out = np.zeros((n, words_per_row(d)), np.uint32)
    for t in range(d):
        out[:, t // 8] |= c[:, t].astype(np.uint32) << np.uint32(4 * (t % 8))
    return out


def unpack4(words, d: int) -> np.ndarray:
    """uint32 (n, W) -> uint8 (n, d)"""
    w = np.asarray(words, np.uint32)
    out = np.empty((w.shape[0], d), np.uint8)
    for t in range(d):
        out[:, t] = (w[:, t // 8] >> np.uint32(4 * (t % 8))) & np.uint32(15)
    return out


def step_of(mn, mx, levels) -> np.float32:
    """(max - min) / (levels - 1) in f32, as ScalarQuantizer::new computes it"""
    return F((F(mx) - F(mn)) / F(levels - 1))


def dequantize(codes, mn, mx, levels) -> np.ndarray:
    """v(c) = min + float32(c) * step for every code value, codes >= levels included; float32, two roundings"""
    t = np.asarray(codes).astype(F) * step_of(mn, mx, levels)
    return (F(mn) + t).astype(F)


def decode(words, d: int, mn, mx, levels) -> np.ndarray:
    """the dequantized rows, float32 (n, d)"""
    return dequantize(unpack4(words, d), mn, mx, levels)


def matrix_over(metric, Q, V) -> np.ndarray:
    """D(q, i) for every query and row of V (n, d) f32, float32 (nq, n): ref_knn.distances, every query at once -- each
    pair still summed over t ascending from -0.0, one rounding per operation"""
    Q = np.atleast_2d(np.asarray(Q, F))
    V = np.asarray(V, F)
    acc = np.full((Q.shape[0], V.shape[0]), -0.0, F)
    with np.errstate(all="ignore"):
        for t in range(V.shape[1]):
            q, v = Q[:, t, None], V[None, :, t]
            if metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN):
                diff = q - v
                acc = acc + diff * diff
            elif metric == K.MANHATTAN:
                acc = acc + np.abs(q - v)
            else:
                acc = acc + q * v
        if metric == K.EUCLIDEAN:
            return np.sqrt(acc)
    if metric in (K.COSINE, K.COSINE_UNCLAMPED):
        return K.cosine_finish(metric, acc, K.norms(Q)[:, None], K.norms(V)[None, :])
    return acc


def distance_matrix(metric, Q, words, d, mn, mx, levels) -> np.ndarray:
    return matrix_over(metric, Q, decode(words, d, mn, mx, levels))


def search(metric, Q, words, d, mn, mx, levels, k):
    return topk(distance_matrix(metric, Q, words, d, mn, mx, levels), k)
