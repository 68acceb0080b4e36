"""numpy statement of the scalar index (include/vqhip.h vqhip_sqindex_*, vq_amd.ScalarIndex): the codes decoded by the SQ
rule of tests/ref_sqbq.py, v(c) = min + f32(c) * step for every byte value, then the exact k-NN statement of
tests/ref_knn.py over the decoded rows.  The queries are f32 and never quantized."""
import numpy as np

import ref_knn as K
import ref_sqbq as S

F = np.float32
METRICS = K.METRICS

# the quantizers of the GPU cases; the last has step = inf, so v(0) = 0 * inf = NaN and v(c > 0) = +inf
QUANTIZERS = [(-1.0, 1.0, 256), (0.0, 1.0, 2), (-3.0, 5.0, 17), (-3e38, 3e38, 2)]


def decode(sq, codes) -> np.ndarray:
    """v(codes) for sq = (min, max, levels); codes >= levels decode by the same formula"""
    return S.sq_decode(sq[0], sq[1], sq[2], codes)


def table(sq) -> np.ndarray:
    """v(c) for c = 0 .. 255"""
    return decode(sq, np.arange(256, dtype=np.uint8))


def distances(metric, q, sq, codes):
    return K.distances(metric, q, decode(sq, codes))


def search(metric, Q, sq, codes, topk):
    return K.search(metric, Q, decode(sq, codes), topk)


def rerank(metric, Q, sq, codes, cand, topk):
    return K.rerank(metric, Q, decode(sq, codes), cand, topk)
