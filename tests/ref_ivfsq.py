"""numpy statement of the inverted-file scalar search of include/vqhip.h (vqhip_ivfsq_*, vq_amd.IVFScalarIndex): the
inverted-file flat statement (tests/ref_ivfflat.py) over the codes decoded by the SQ rule (tests/ref_sqindex.py).  It
makes no arithmetic of its own."""
import ref_ivfflat as R
import ref_sqindex as S

PAD_ID = R.PAD_ID
QUANTIZERS = S.QUANTIZERS


def probe(metric, coarse, Q, nprobe):
    return R.probe(metric, coarse, Q, nprobe)


def search(metric, coarse, lists, sq, codes, Q, nprobe, topk, queries=None):
    """(idx uint32 (nq, topk), dist f32 (nq, topk)) for sq = (min, max, levels) and codes uint8 (n, dim)"""
    return R.search(metric, coarse, lists, S.decode(sq, codes), Q, nprobe, topk, queries=queries)
