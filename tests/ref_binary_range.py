"""numpy statement of the Hamming-radius range search of include/vqhip.h (vqhip_binary_range_search,
vqhip_ivfbin_range_search, vq_amd.BinaryIndex.hamming_range_search, vq_amd.IVFBinaryIndex.hamming_range_search).

Per query q with radius h (an integer number of bits): H = the Hamming distances of tests/ref_binary.py, row i is a hit
iff H[i] <= h, the hits come in ascending row id and carry the distance tests/ref_binary.py reports for their H.  The
inverted-file form keeps the rows whose list tests/ref_ivf.py probes.  The result is tests/ref_range.py's CSR.  It makes
no arithmetic of its own."""
import numpy as np

import ref_binary as B
import ref_ivf as I
import ref_ivfbin as IB

F = np.float32


def hradii(radius, nq):
    """the radii as Python integers, one per query"""
    r = np.asarray(radius, dtype=object)
    out = [int(r)] * nq if r.ndim == 0 else [int(v) for v in r]
    assert len(out) == nq and all(0 <= v < 1 << 32 for v in out)
    return out


def clamped(h, d):
    """the cut the dense kernels compare H with: any h >= d admits every row"""
    return min(int(h), int(d))


def float_radius(h, d, low, high, metric):
    """the f32 radius the inverted-file form hands the range stage: the distance reported for H = min(h, d)"""
    return B.reported(d, low, high, metric)[clamped(h, d)]


def _csr(per_query):
    lims = np.zeros(len(per_query) + 1, np.uint64)
    for j, (i, _) in enumerate(per_query):
        lims[j + 1] = lims[j] + np.uint64(i.size)
    idx = np.concatenate([i for i, _ in per_query] + [np.empty(0, np.uint32)]).astype(np.uint32)
    dist = np.concatenate([d for _, d in per_query] + [np.empty(0, F)]).astype(F)
    return lims, idx, dist


def search(qwords, words, d, low, high, metric, radius):
    """BinaryIndex.from_packed(words, d, ...).hamming_range_search over packed queries: (lims, idx, dist)"""
    qwords = np.asarray(qwords, np.uint32).reshape(-1, (d + 31) // 32)
    h = hradii(radius, qwords.shape[0])
    D = B.reported(d, low, high, metric)
    H = B.hamming(qwords, words) if qwords.shape[0] else np.empty((0, len(words)), np.int64)
    out = []
    for j in range(qwords.shape[0]):
        rows = np.nonzero(H[j] <= h[j])[0]
        out.append((rows.astype(np.uint32), D[H[j][rows]]))
    return _csr(out)


def search_rows(Q, X, threshold, low, high, metric, radius):
    d = X.shape[1]
    Q = np.asarray(Q, F).reshape(-1, d)
    return search(B.pack(B.bits_f32(Q, threshold)), B.pack(B.bits_f32(X, threshold)), d, low, high, metric, radius)


def ivf_search(metric, coarse_metric, coarse, lists, bq, words, dim, Q, nprobe, radius, P=None):
    """IVFBinaryIndex.hamming_range_search for bq = (threshold, low, high) and words uint32 (n, W): statement `search`
    over the members of the probed lists, which are ascending row ids"""
    thr, low, high = bq
    Q = np.asarray(Q, F).reshape(-1, dim)
    words = np.asarray(words, np.uint32).reshape(-1, (dim + 31) // 32)
    h = hradii(radius, Q.shape[0])
    P = IB.probe(coarse_metric, coarse, Q, nprobe) if P is None and Q.shape[0] else P
    qw = B.pack(B.bits_f32(Q, thr))
    D = B.reported(dim, low, high, metric)
    out = []
    for j in range(Q.shape[0]):
        S = I.members(lists, P[j])
        if S.size == 0:
            out.append((np.empty(0, np.uint32), np.empty(0, F)))
            continue
        H = B.hamming(qw[j:j + 1], words[S])[0]
        keep = np.nonzero(H <= h[j])[0]
        out.append((S[keep].astype(np.uint32), D[H[keep]]))
    return _csr(out)


def same(a, b):
    """equality of two results: lims, idx and the distance bits"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].dtype == F and b[2].dtype == F
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))
