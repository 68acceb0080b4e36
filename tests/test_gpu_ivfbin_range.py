"""Hamming-radius range search of the inverted-file binary index on the MI355X (IVFBinaryIndex.hamming_range_search,
vqhip_ivfbin_range_search: the range stage of vq_amd/csrc/ivf_range.hpp behind k_ivfbin.hip's distances).  Every
comparison is equality of lims, idx and the distance bits: against the numpy statement (tests/ref_binary_range.py) at
nprobe 1, 2 and nlist, and against BinaryIndex.hamming_range_search over the words in add order at nprobe == nlist --
an integer cut in a fused scan against a float comparison on stored distances.  The three metrics, the three loaders,
batches that take the tile kernel and batches that take the per-query scan, empty lists, an index without rows, an add
between two calls, a cosine coarse distance, the cap and the device form."""
import numpy as np
import pytest

import ref_binary as B
import ref_binary_range as BR
import ref_ivfbin as R
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
U32_MAX = (1 << 32) - 1
THRESHOLDS = {(0, 1): 0.0, (0, 255): 0.0, (254, 255): -0.5, (3, 200): 0.25}


def _assert_same(got, want):
    gl, gi, gd = got
    wl, wi, wd = want
    assert gl.dtype == np.uint64 and gi.dtype == np.uint32 and gd.dtype == F
    assert gl.shape == wl.shape and np.array_equal(gl, wl), f"lims differ: {gl[:8]} != {wl[:8]}"
    assert gi.shape == wi.shape
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[bad[0]]} != {wi[bad[0]]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _case(rng, n, nlist, dim, nq):
    """rows in an order unrelated to their lists, duplicates in the same list, a query equal to a duplicated row"""
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[n - 7:] = rows[:7]
    lists[n - 7:] = lists[:7]
    Q = rng.standard_normal((nq, dim)).astype(F)
    Q[0] = rows[3]
    return coarse, lists, rows, Q


def _radii(dim, nq, rng):
    """around the mass of H (dim / 2 for random bits), with 0, dim, dim + 1 and 2^32 - 1 among them"""
    r = rng.integers(max(dim // 2 - dim // 8 - 2, 0), dim // 2 + 1, nq).astype(np.uint64)
    r[0] = 0
    for j, v in zip(range(1, nq), (dim, U32_MAX, dim + 1, 1)):
        r[j] = v
    return r


def _index(coarse, metric, bq, coarse_metric=K.EUCLIDEAN):
    import vq_amd

    return vq_amd.IVFBinaryIndex(coarse, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]),
                                 vq_amd.Distance(NAMES[coarse_metric]))


def _dense(words, dim, metric, bq):
    import vq_amd

    return vq_amd.BinaryIndex.from_packed(words, dim, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]))


# (n, nlist, dim, nq): nq = 40 puts lists on the tile kernel (16 queries or more probe them) and on the scan, nq = 3
# leaves every list to the scan; W = 4 / 3 / 6 words are the 16-, 4- and 8-byte loaders; 256 lists are mostly empty
SHAPES = [(3001, 7, 128, 40), (2500, 256, 96, 40), (2000, 7, 192, 40), (1500, 7, 33, 3), (900, 5, 1056, 40)]


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_statement_and_dense_index(metric, shape):
    n, nlist, dim, nq = shape
    rng = np.random.default_rng(n + dim + metric)
    low, high = R.LOW_HIGH[(dim + metric) % 4]
    bq = (THRESHOLDS[(low, high)], low, high)
    coarse, lists, rows, Q = _case(rng, n, nlist, dim, nq)
    words = B.pack(B.bits_f32(rows, bq[0]))
    radius = _radii(dim, nq, rng)
    ix = _index(coarse, metric, bq)
    ix.add_packed(lists, words)
    for nprobe in (1, 2, nlist):
        want = BR.ivf_search(metric, K.EUCLIDEAN, coarse, lists, bq, words, dim, Q, nprobe, radius)
        assert want[0][-1] > 0
        _assert_same(ix.hamming_range_search(Q, radius, nprobe=nprobe), want)
    full = ix.hamming_range_search(Q, radius, nprobe=nlist)
    assert int(full[0][2] - full[0][1]) == n  # radius dim over every list: every row
    _assert_same(full, _dense(words, dim, metric, bq).hamming_range_search(Q, radius))  # the identity


def test_sources_add_between_calls_and_no_rows():
    """an index without rows answers with empty ranges; rows added as f32 rows, as u8 codes and as words between calls"""
    rng = np.random.default_rng(5)
    dim, nlist = 70, 6
    bq = (0.25, 3, 200)
    coarse, lists, rows, Q = _case(rng, 1200, nlist, dim, 20)
    words = B.pack(B.bits_f32(rows, bq[0]))
    radius = _radii(dim, 20, rng)
    ix = _index(coarse, B.EUC, bq)
    got = ix.hamming_range_search(Q, radius, nprobe=3)
    assert got[0].tolist() == [0] * 21 and got[1].size == 0 and got[2].size == 0
    a, b = 400, 800
    ix.add_rows(lists[:a], rows[:a])
    _assert_same(ix.hamming_range_search(Q, radius, nprobe=3),
                 BR.ivf_search(B.EUC, K.EUCLIDEAN, coarse, lists[:a], bq, words[:a], dim, Q, 3, radius))
    ix.add_codes(lists[a:b], np.where(B.bits_f32(rows[a:b], bq[0]), np.uint8(200), np.uint8(3)))
    _assert_same(ix.hamming_range_search(Q, radius, nprobe=3),
                 BR.ivf_search(B.EUC, K.EUCLIDEAN, coarse, lists[:b], bq, words[:b], dim, Q, 3, radius))
    ix.add_packed(lists[b:], words[b:])
    assert np.array_equal(ix.packed(), words)
    got = ix.hamming_range_search(Q, radius, nprobe=nlist)
    _assert_same(got, BR.ivf_search(B.EUC, K.EUCLIDEAN, coarse, lists, bq, words, dim, Q, nlist, radius))
    _assert_same(got, _dense(words, dim, B.EUC, bq).hamming_range_search(Q, radius))
    _assert_same(ix.hamming_range_search(Q, radius, nprobe=nlist), got)  # the same call again: identical arrays


def test_cosine_coarse_distance():
    rng = np.random.default_rng(6)
    dim, nlist = 48, 9
    bq = (0.0, 0, 1)
    coarse, lists, rows, Q = _case(rng, 1500, nlist, dim, 24)
    words = B.pack(B.bits_f32(rows, bq[0]))
    radius = _radii(dim, 24, rng)
    ix = _index(coarse, B.MAN, bq, coarse_metric=K.COSINE)
    ix.add_packed(lists, words)
    for nprobe in (1, 4):  # nprobe 1: the hits of a list are in row order already, no sort pass runs
        _assert_same(ix.hamming_range_search(Q, radius, nprobe=nprobe),
                     BR.ivf_search(B.MAN, K.COSINE, coarse, lists, bq, words, dim, Q, nprobe, radius))


def _read_device(ptr, count, dtype):
    import torch

    from vq_amd import _lib

    t = torch.zeros(max(count, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if count:
        _lib.memcpy_device(t.data_ptr(), ptr, count * np.dtype(dtype).itemsize)
    _lib.synchronize()
    return t.cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype)


def test_cap_and_device_form():
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(8)
    dim, nlist, nq = 64, 4, 12
    bq = (0.0, 0, 255)
    coarse, lists, rows, Q = _case(rng, 2000, nlist, dim, nq)
    words = B.pack(B.bits_f32(rows, bq[0]))
    ix = _index(coarse, B.SQ, bq)
    ix.add_packed(lists, words)
    want = BR.ivf_search(B.SQ, K.EUCLIDEAN, coarse, lists, bq, words, dim, Q, nlist, dim)
    total = int(want[0][-1])
    assert total == nq * 2000
    with pytest.raises(vq_amd.FfiError) as e:
        ix.hamming_range_search(Q, dim, nprobe=nlist, max_results=total - 1)
    assert e.value.status == _lib.ERR_UNSUPPORTED and str(total) in str(e.value) and str(total - 1) in str(e.value)
    _assert_same(ix.hamming_range_search(Q, dim, nprobe=nlist, max_results=total), want)  # usable afterwards
    radius = _radii(dim, nq, rng)
    want = BR.ivf_search(B.SQ, K.EUCLIDEAN, coarse, lists, bq, words, dim, Q, 2, radius)
    qb = torch.zeros(nq * dim + 9, dtype=torch.float32, device="cuda:0")
    qb[1:1 + nq * dim] = torch.from_numpy(Q.ravel()).to("cuda:0")
    torch.cuda.synchronize()
    res = ix.hamming_range_search_device(qb.data_ptr() + 4, nq, radius, nprobe=2)
    assert isinstance(res, vq_amd.RangeResult) and res.nq == nq and res.total == int(want[0][-1])
    _assert_same(res.read(), want)
    pl, pi, pd = res.device_pointers()
    got = (_read_device(pl, nq + 1, np.uint64), _read_device(pi, res.total, np.uint32), _read_device(pd, res.total, F))
    _assert_same(got, want)
    empty = ix.hamming_range_search_device(qb.data_ptr() + 4, 0, np.empty(0, np.uint32), nprobe=2)
    assert empty.total == 0 and empty.lims.tolist() == [0]
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.hamming_range_search_device(qb.data_ptr() + 2, nq, radius, nprobe=2)
