"""numpy statement of the inverted-file 4-bit scalar search of include/vqhip.h (vqhip_ivfsq4_*, vq_amd.IVFScalar4Index):
the inverted-file flat statements (tests/ref_ivfflat.py, ref_ivf_range.py, ref_ivf_filter.py) over the unpacked codes
decoded by the 4-bit rule (tests/ref_sq4.py: v(c) = min + float32(c) * step, two roundings, every nibble value).  It
makes no arithmetic of its own.  sq = (min, max, levels); codes uint8 (n, dim), each <= 15."""
import ref_ivf_filter as FI
import ref_ivf_range as RG
import ref_ivfflat as R
import ref_sq4 as S4

PAD_ID = R.PAD_ID
QUANTIZERS = S4.QUANTIZERS


def decode(sq, codes):
    """the dequantized rows float32 (n, dim), through the packed words: what the index keeps"""
    return S4.decode(S4.pack4(codes), codes.shape[1], *sq)


def probe(metric, coarse, Q, nprobe):
    return R.probe(metric, coarse, Q, nprobe)


def search(metric, coarse, lists, sq, codes, Q, nprobe, topk, queries=None):
    """(idx uint32 (nq, topk), dist f32 (nq, topk))"""
    return R.search(metric, coarse, lists, decode(sq, codes), Q, nprobe, topk, queries=queries)


def search_masked(metric, coarse, lists, sq, codes, Q, nprobe, topk, mask, queries=None):
    return FI.search(metric, coarse, lists, decode(sq, codes), Q, nprobe, topk, mask, queries)


def range_search(metric, coarse, lists, sq, codes, Q, nprobe, radius):
    """(lims uint64 (nq + 1,), idx uint32, dist f32): CSR, ascending row id within a query"""
    return RG.search(metric, coarse, lists, decode(sq, codes), Q, nprobe, radius)


def range_search_masked(metric, coarse, lists, sq, codes, Q, nprobe, radius, mask):
    return FI.range_search(metric, coarse, lists, decode(sq, codes), Q, nprobe, radius, mask)
