"""numpy statement of the inverted-file binary search of include/vqhip.h (vqhip_ivfbin_*, vq_amd.IVFBinaryIndex): the probe
and the members of the inverted-file statement (tests/ref_ivf.py) around the Hamming distance and the reported distance
of the binary statement (tests/ref_binary.py).  It makes no arithmetic of its own."""
import numpy as np

import ref_binary as B
import ref_ivf as I

F = np.float32
PAD_ID = I.PAD_ID
METRICS = B.METRICS
LOW_HIGH = [(0, 1), (0, 255), (254, 255), (3, 200)]  # tests/test_binary_host.py's


def probe(coarse_metric, coarse, Q, nprobe):
    """P(q) for the f32 queries, never binarised"""
    return I.probe(coarse_metric, coarse, Q, nprobe)


def search(metric, coarse_metric, coarse, lists, bq, words, dim, Q, nprobe, topk, P=None):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)) for bq = (threshold, low, high) and words uint32 (n, W): per query
    the topk rows of S(q) by (H, row id) -- S(q) is ascending, so a stable sort by H is that order -- reported as D[H].  P: probe(...)'s result where the caller has it already"""
    thr, low, high = bq
    Q = np.atleast_2d(np.asarray(Q, F))
    words = np.asarray(words, np.uint32)
    P = probe(coarse_metric, coarse, Q, nprobe) if P is None else P
    qw = B.pack(B.bits_f32(Q, thr))
    D = B.reported(dim, low, high, metric)
    idx = np.full((Q.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((Q.shape[0], topk), np.inf, F)
    for j in range(Q.shape[0]):
        S = I.members(lists, P[j])
        if S.size == 0:
            continue
        H = B.hamming(qw[j:j + 1], words[S])[0]
        order = np.argsort(H, kind="stable")[:topk]
        idx[j, :order.size] = S[order].astype(np.uint32)
        dist[j, :order.size] = D[H[order]]
    return idx, dist
