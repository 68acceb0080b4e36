"""numpy statement of the filtered search of the two binary indexes (include/vqhip.h vqhip_binary_*_masked and
vqhip_ivfbin_*_masked; vq_amd.BinaryIndex / IVFBinaryIndex ``filtered_search`` and ``filtered_hamming_range_search``).

A row mask of n rows is a bool array m (n,), its words ``pack(m)`` (tests/ref_filter.py).  Every filtered result is the
unfiltered statement over the allowed rows alone, their ids mapped back:
  masked top-k   tests/ref_binary.py's search over words[rows], rows = np.flatnonzero(m) -- ascending, so the stable order
                 (H, position) is the order (H, row id) -- padded with (0xFFFFFFFF, +inf) behind fewer than topk rows
  masked range   tests/ref_binary_range.py's search over words[rows]
  inverted file  tests/ref_ivfbin.py / ref_binary_range.py over (lists[rows], words[rows]) with the probe of the f32
                 queries, which takes no mask
It makes no arithmetic of its own."""
import numpy as np

import ref_binary as B
import ref_binary_range as BR
import ref_filter as RF
import ref_ivfbin as IB

F = np.float32
PAD_ID = np.uint32(0xFFFFFFFF)
pack, unpack = RF.pack, RF.unpack


def _rows(mask):
    return np.flatnonzero(np.asarray(mask, np.bool_))


def _back(idx, rows):
    """positions among the allowed rows -> row ids, padding kept"""
    out = np.full(idx.shape, PAD_ID, np.uint32)
    real = idx != PAD_ID
    out[real] = rows[idx[real].astype(np.int64)].astype(np.uint32)
    return out


def search(qwords, words, d, low, high, metric, topk, mask):
    """BinaryIndex.from_packed(words, d, ...).filtered_search over packed queries"""
    qwords = np.asarray(qwords, np.uint32).reshape(-1, (d + 31) // 32)
    rows = _rows(mask)
    idx = np.full((qwords.shape[0], topk), PAD_ID, np.uint32)
    dist = np.full((qwords.shape[0], topk), np.inf, F)
    k = min(topk, rows.size)
    if k and qwords.shape[0]:
        i, dd = B.search(qwords, np.asarray(words, np.uint32)[rows], d, low, high, metric, k)
        idx[:, :k], dist[:, :k] = _back(i, rows), dd
    return idx, dist


def search_rows(Q, X, threshold, low, high, metric, topk, mask):
    d = X.shape[1]
    return search(B.pack(B.bits_f32(np.asarray(Q, F).reshape(-1, d), threshold)), B.pack(B.bits_f32(X, threshold)), d, low, high,
                  metric, topk, mask)


def range_search(qwords, words, d, low, high, metric, radius, mask):
    """BinaryIndex.from_packed(words, d, ...).filtered_hamming_range_search over packed queries: (lims, idx, dist)"""
    rows = _rows(mask)
    lims, idx, dist = BR.search(qwords, np.asarray(words, np.uint32)[rows], d, low, high, metric, radius)
    return lims, _back(idx, rows), dist


def range_search_rows(Q, X, threshold, low, high, metric, radius, mask):
    d = X.shape[1]
    return range_search(B.pack(B.bits_f32(np.asarray(Q, F).reshape(-1, d), threshold)), B.pack(B.bits_f32(X, threshold)), d, low,
                        high, metric, radius, mask)


def ivf_search(metric, coarse_metric, coarse, lists, bq, words, dim, Q, nprobe, topk, mask):
    """IVFBinaryIndex.filtered_search: the probe of the unfiltered index, then its search over the allowed rows' lists"""
    Q = np.asarray(Q, F).reshape(-1, dim)
    rows = _rows(mask)
    P = IB.probe(coarse_metric, coarse, Q, nprobe)
    words = np.asarray(words, np.uint32).reshape(-1, (dim + 31) // 32)
    idx, dist = IB.search(metric, coarse_metric, coarse, np.asarray(lists)[rows], bq, words[rows], dim, Q, nprobe, topk, P=P)
    return _back(idx, rows), dist


def ivf_range_search(metric, coarse_metric, coarse, lists, bq, words, dim, Q, nprobe, radius, mask):
    """IVFBinaryIndex.filtered_hamming_range_search"""
    Q = np.asarray(Q, F).reshape(-1, dim)
    rows = _rows(mask)
    P = IB.probe(coarse_metric, coarse, Q, nprobe) if Q.shape[0] else None
    words = np.asarray(words, np.uint32).reshape(-1, (dim + 31) // 32)
    lims, idx, dist = BR.ivf_search(metric, coarse_metric, coarse, np.asarray(lists)[rows], bq, words[rows], dim, Q, nprobe,
                                    radius, P=P)
    return lims, _back(idx, rows), dist
