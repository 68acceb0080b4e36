"""numpy statement of the binary index (include/vqhip.h vqhip_binary_*, vq_amd.BinaryIndex): the bit rules, the packed
layout, the Hamming distance H, the S tables and the result order."""
import numpy as np

F = np.float32
SQ, EUC, MAN = 0, 1, 2  # VQHIP_SQUARED_EUCLIDEAN, VQHIP_EUCLIDEAN, VQHIP_MANHATTAN
METRICS = (SQ, EUC, MAN)
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)


def bits_f32(X, threshold):
    """x >= threshold (NaN -> False, -0.0 == 0.0)"""
    return np.asarray(X, F) >= F(threshold)


def bits_u8(codes, high):
    return np.asarray(codes, np.uint8) >= np.uint8(high)


def pack(bits):
    """bool (n, d) -> uint32 (n, ceil(d / 32)): np.packbits, little bit order, padded to 32 bits, viewed as <u4"""
    b = np.asarray(bits, bool)
    n, d = b.shape
    w = (d + 31) // 32
    padded = np.zeros((n, 32 * w), bool)
    padded[:, :d] = b
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, w)


def hamming(qwords, words):
    """H [nq][n] of packed queries against packed rows"""
    w = np.ascontiguousarray(words, dtype="<u4")
    H = np.empty((qwords.shape[0], w.shape[0]), np.int64)
    for i, q in enumerate(np.asarray(qwords, "<u4")):
        H[i] = _POP[np.bitwise_xor(w, q).view(np.uint8)].sum(axis=1, dtype=np.int64)
    return H


def table(d, low, high, metric):
    """S [d + 1] in sequential f32: S(0) = +0.0, S(j) = fl(S(j - 1) + t); t = a * a or a, a = f32(high) - f32(low);
    Euclidean reports sqrtf(S)"""
    a = F(high) - F(low)
    t = a if metric == MAN else F(a * a)
    S = np.empty(d + 1, F)
    s = F(0.0)
    S[0] = s
    for j in range(1, d + 1):
        s = F(s + t)
        S[j] = s
    return S


def reported(d, low, high, metric):
    """the distance reported for each H: S, or sqrtf(S) for Euclidean"""
    S = table(d, low, high, metric)
    return np.sqrt(S).astype(F) if metric == EUC else S


def search(qwords, words, d, low, high, metric, topk):
    """per query the topk rows by (H, row) ascending -- the (D, row) order, since every table is strictly increasing"""
    H = hamming(qwords, words)
    order = np.argsort(H, axis=1, kind="stable")[:, :topk]  # stable: ties keep row order
    D = reported(d, low, high, metric)
    idx = order.astype(np.uint32)
    return idx, D[np.take_along_axis(H, order, axis=1)]


def search_rows(Q, X, threshold, low, high, metric, topk):
    d = X.shape[1]
    return search(pack(bits_f32(Q, threshold)), pack(bits_f32(X, threshold)), d, low, high, metric, topk)
