"""Inverted-file range search on the MI355X (vq_amd.IVFFlatIndex.range_search, vq_amd.IVFScalarIndex.range_search,
vqhip_ivfflat_range_search, vqhip_ivfsq_range_search; vq_amd/csrc/ivf_range.hpp) against the numpy statement of
include/vqhip.h (tests/ref_ivf_range.py): lims and row ids equal, distances equal as uint32 bits.  All five metrics, f32 and
f16 rows and every SQ loader, dim 1 / 5 / 33 / 128 (36: the 4-byte SQ loader), an empty list, rows added in two adds,
nprobe 1 / 3 / nlist; radii on a tied boundary, +inf and -1; nprobe == nlist against FlatIndex / ScalarIndex, the scalar
index against the flat one over the dequantized rows; batches on both sides of the count (16 queries per list) from which
the tile kernel takes a list; the ordering stage with three radix passes, segments spanning several blocks, empty segments
and ragged lengths; short queries behind a long one's finite distances in W on both load paths; two batches with two
buffer growths; the cap; determinism; the device form; an add between two calls; an index without rows; consistency
with search."""
import os
import re

import numpy as np
import pytest

import ref_ivf_range as RR
import ref_ivfflat as IF
import ref_knn as K
import ref_sqindex as SI

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_INIT_CAP = 1024  # kRangeInitCap (vq_amd/csrc/range.hpp): the growth test assumes it and checks it


def _bits(a):
    return a.view(np.uint32) if a.dtype == F else a


def _assert_same(got, want):
    gl, gi, gd = got
    wl, wi, wd = want
    assert gl.dtype == np.uint64 and gi.dtype == np.uint32 and gd.dtype == F
    assert gl.shape == wl.shape and np.array_equal(gl, wl), f"lims differ: {gl[:8]} != {wl[:8]}"
    assert gi.shape == wi.shape
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[bad[0]]} != {wi[bad[0]]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _dist(metric):
    import vq_amd

    return vq_amd.Distance(NAMES[metric])


def _lists(rng, n, nlist, empty):
    """list ids in an order unrelated to the rows', unequal list sizes, list `empty` without rows"""
    w = rng.random(nlist) + 0.2
    w[empty] = 0.0
    return rng.choice(nlist, n, p=w / w.sum()).astype(np.uint32)


def _case(rng, n, nlist, dim, dtype, nq):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = _lists(rng, n, nlist, empty=nlist // 2)
    rows = (coarse[lists] + F(0.5) * rng.standard_normal((n, dim)).astype(F)).astype(dtype)
    rows[n - 7:] = rows[:7]    # duplicate rows ...
    lists[n - 7:] = lists[:7]  # ... in the same lists: equal distances
    Q = rng.standard_normal((nq, dim)).astype(F)
    Q[0] = rows[3].astype(F)
    return coarse, lists, rows, Q


def _tied_radii(metric, Q, X, special=True):
    """r_q = D(q, row q), row q being one of the duplicated rows: where its list is probed, two equal distances lie exactly
    on the boundary.  The last two queries get +inf and -1."""
    X = np.asarray(X).astype(F)
    r = np.array([K.distances(metric, Q[j], X[j % 7:j % 7 + 1])[0] for j in range(Q.shape[0])], F)
    r[np.isnan(r)] = 1.0
    if special:
        r[-2] = np.inf
        r[-1] = -1.0
    return r


def _flat_index(coarse, metric, lists, rows, pieces=2):
    import vq_amd

    ix = vq_amd.IVFFlatIndex(coarse, _dist(metric), rows.dtype)
    for a in np.array_split(np.arange(len(lists)), pieces):
        ix.add_rows(lists[a], rows[a])
    return ix


def _sq_index(coarse, metric, lists, sq, codes, pieces=2):
    import vq_amd

    ix = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*sq), _dist(metric))
    for a in np.array_split(np.arange(len(lists)), pieces):
        ix.add_codes(lists[a], codes[a])
    return ix


def test_initial_capacity_is_the_one_assumed():
    text = open(os.path.join(ROOT, "vq_amd", "csrc", "range.hpp")).read()
    assert int(re.search(r"kRangeInitCap\s*=\s*(\d+)", text).group(1)) == RANGE_INIT_CAP


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", [1, 5, 33, 128])
def test_flat_matches_statement_and_flat_index(metric, d, dtype):
    import vq_amd

    n, nlist, nq = 5003 + 97 * d % 1000, 11, 7
    rng = np.random.default_rng(1000 * metric + d)
    coarse, lists, rows, Q = _case(rng, n, nlist, d, dtype, nq)
    assert np.bincount(lists, minlength=nlist)[nlist // 2] == 0
    r = _tied_radii(metric, Q, rows)
    ix = _flat_index(coarse, metric, lists, rows)
    for nprobe in (1, 3, nlist):
        got = ix.range_search(Q, r, nprobe=nprobe)
        _assert_same(got, RR.search(metric, coarse, lists, rows, Q, nprobe, r))
    _assert_same(vq_amd.FlatIndex(rows, _dist(metric)).range_search(Q, r), got)  # nprobe == nlist: bit identity
    assert int(got[0][-2] - got[0][-3]) >= n - 1 and got[0][-1] == got[0][-2]  # +inf: (nearly) all rows; -1: none
    ix.close()


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", [1, 5, 33, 36, 128])  # the byte loader, the 4-byte one (36) and the 16-byte one (128)
def test_scalar_matches_statement_flat_and_scalar_index(metric, d):
    import vq_amd

    n, nlist, nq = 5200 + 31 * d, 9, 7
    rng = np.random.default_rng(2000 * metric + d)
    sq = SI.QUANTIZERS[0] if d != 5 else SI.QUANTIZERS[2]
    coarse = rng.uniform(-1, 1, (nlist, d)).astype(F)
    lists = _lists(rng, n, nlist, empty=4)
    codes = rng.integers(0, sq[2], (n, d), dtype=np.uint8)
    codes[n - 7:] = codes[:7]
    lists[n - 7:] = lists[:7]
    X = SI.decode(sq, codes)
    Q = rng.uniform(-1, 1, (nq, d)).astype(F)
    Q[0] = X[3]
    r = _tied_radii(metric, Q, X)
    ix = _sq_index(coarse, metric, lists, sq, codes)
    flat = _flat_index(coarse, metric, lists, X)
    for nprobe in (1, 3, nlist):
        got = ix.range_search(Q, r, nprobe=nprobe)
        _assert_same(got, RR.sq_search(metric, coarse, lists, sq, codes, Q, nprobe, r))
        _assert_same(flat.range_search(Q, r, nprobe=nprobe), got)  # the flat index over the dequantized rows
    dense = vq_amd.ScalarIndex.from_codes(codes, vq_amd.ScalarQuantizer(*sq), _dist(metric))
    _assert_same(dense.range_search(Q, r), got)  # nprobe == nlist: bit identity
    ix.close()
    flat.close()


def test_scalar_index_from_rows_and_degenerate_quantizer():
    """add_rows (encoded on the device), and the quantizer whose decoded rows are NaN and +inf: NaN never hits"""
    import vq_amd

    rng = np.random.default_rng(77)
    n, d, nlist = 3001, 8, 5
    coarse = rng.uniform(-1, 1, (nlist, d)).astype(F)
    lists = _lists(rng, n, nlist, empty=1)
    sq = SI.QUANTIZERS[0]
    codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    rows = SI.decode(sq, codes)  # rows that encode back to these codes
    Q = rng.uniform(-1, 1, (5, d)).astype(F)
    ix = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*sq))
    ix.add_rows(lists[:1000], rows[:1000])
    ix.add_rows(lists[1000:], rows[1000:])
    assert np.array_equal(ix.codes, codes)
    r = _tied_radii(K.EUCLIDEAN, Q, rows)
    _assert_same(ix.range_search(Q, r, nprobe=2), RR.sq_search(K.EUCLIDEAN, coarse, lists, sq, codes, Q, 2, r))
    deg = SI.QUANTIZERS[3]
    c2 = rng.integers(0, 2, (n, d), dtype=np.uint8)
    c2[::3] = 1  # rows of +inf only: distance +inf, a hit at +inf
    ix2 = _sq_index(coarse, K.MANHATTAN, lists, deg, c2)
    want = RR.sq_search(K.MANHATTAN, coarse, lists, deg, c2, Q, nlist, np.inf)
    assert 0 < want[0][-1] < 5 * n
    _assert_same(ix2.range_search(Q, np.inf, nprobe=nlist), want)


@pytest.fixture(scope="module")
def one_list():
    """129 queries around one centroid of 6 (nprobe 2: its list and a neighbour's), the statement computed once"""
    rng = np.random.default_rng(21)
    n, d, nlist = 5000, 33, 6
    coarse = (4.0 * rng.standard_normal((nlist, d))).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = (coarse[lists] + rng.standard_normal((n, d)).astype(F)).astype(F)
    Q = (coarse[2] + F(0.05) * rng.standard_normal((129, d)).astype(F)).astype(F)
    P = IF.probe(K.EUCLIDEAN, coarse, Q, 2)
    assert (P == P[0]).all()  # every query probes the same two lists
    r = np.full(129, np.sqrt(F(d)) * F(1.0), F)
    return coarse, lists, rows, Q, r, RR.search(K.EUCLIDEAN, coarse, lists, rows, Q, 2, r)


@pytest.mark.parametrize("which", ["flat", "scalar"])
def test_scan_and_tile_kernels_feed_the_stage(one_list, which):
    """1 and 15 queries per list: the scan kernel; 16, 17 and 129: the tile kernel (129: two query tiles)"""
    coarse, lists, rows, Q, r, want = one_list
    if which == "flat":
        ix = _flat_index(coarse, K.EUCLIDEAN, lists, rows)
    else:
        sq = (-16.0, 16.0, 256)
        import ref_sqbq as S

        codes = S.sq_encode(sq[0], sq[1], sq[2], rows)
        ix = _sq_index(coarse, K.EUCLIDEAN, lists, sq, codes)
        want = RR.sq_search(K.EUCLIDEAN, coarse, lists, sq, codes, Q, 2, r)
    assert 100 < int(np.diff(want[0].astype(np.int64)).min())
    first = None
    for nq in (1, 15, 16, 17, 129):
        got = ix.range_search(Q[:nq], r[:nq], nprobe=2)
        e = int(want[0][nq])
        _assert_same(got, (want[0][:nq + 1], want[1][:e], want[2][:e]))
        one = (got[1][:int(got[0][1])], got[2][:int(got[0][1])])
        if first is None:
            first = one
        assert np.array_equal(one[0], first[0]) and np.array_equal(_bits(one[1]), _bits(first[1]))  # both kernels: the same


@pytest.fixture(scope="module")
def big_ids():
    """70 000 x 4 in 8 lists of unequal sizes (one empty): ids of 17 bits, three radix passes"""
    rng = np.random.default_rng(31)
    n, d, nlist = 70_000, 4, 8
    coarse = (3.0 * rng.standard_normal((nlist, d))).astype(F)
    lists = _lists(rng, n, nlist, empty=5)
    rows = (coarse[lists] + rng.standard_normal((n, d)).astype(F)).astype(F)
    Q = np.concatenate([coarse[[0, 1, 2, 3, 4, 6, 7]], rng.standard_normal((2, d)).astype(F)]).astype(F)
    return coarse, lists, rows, Q


@pytest.mark.parametrize("nprobe", [1, 3, 8])
def test_ordering_stage(big_ids, nprobe):
    """+inf: every position a hit, segments spanning several 4096-position blocks with every lane emitting; queries
    without hits between full ones; |S(q)| differs per query (unequal lists), so most are shorter than wstride"""
    coarse, lists, rows, Q = big_ids
    r = np.array([np.inf, -1.0, np.inf, np.inf, -1.0, -1.0, np.inf, 2.0, np.inf], F)
    want = RR.search(K.SQUARED_EUCLIDEAN, coarse, lists, rows, Q, nprobe, r)
    per = np.diff(want[0].astype(np.int64))
    assert per[0] > 4096 and per[1] == 0 and per[4] == 0 and per[5] == 0
    if nprobe < 8:
        sizes = np.sort(np.bincount(lists, minlength=8))[::-1]
        assert per[[0, 2, 3, 6, 8]].min() < sizes[:nprobe].sum()  # a query shorter than wstride beside the longest
    else:
        assert per[0] == 70_000
    ix = _flat_index(coarse, K.SQUARED_EUCLIDEAN, lists, rows)
    got = ix.range_search(Q, r, nprobe=nprobe)
    _assert_same(got, want)
    for j in range(Q.shape[0]):
        assert (np.diff(got[1][int(got[0][j]):int(got[0][j + 1])].astype(np.int64)) > 0).all()
    _assert_same(ix.range_search(Q, r, nprobe=nprobe), got)  # determinism
    ix.close()


@pytest.mark.parametrize("longest", [4100, 4101])  # wstride 4100 / 4108: a float4 per lane; 4101 / 4109: scalar loads
def test_short_queries_behind_a_long_one(longest):
    """The bound of the count and fill passes: |S(q)| % 4 in {1, 2, 3} on both load paths, with FINITE distances of an
    earlier call behind |S(q)| in W.  The first call's queries probe the long list and fill their rows of W; the second
    call's, on the same index with the same nq and nprobe, probe lists of 5, 6, 11 and 13 rows.  A position at or past
    |S(q)| must not hit under +inf, nor under a radius just above the largest true distance (the stale ones are smaller)."""
    rng = np.random.default_rng(4100)
    sizes = np.array([longest, 8, 5, 6])
    coarse = np.zeros((4, 4), F)
    coarse[:, 0] = [0.0, 120.0, 200.0, 210.0]  # list 1's second neighbour is list 2, list 2's and 3's are each other
    lists = rng.permutation(np.repeat(np.arange(4), sizes)).astype(np.uint32)
    rows = (coarse[lists] + F(0.01) * rng.standard_normal((lists.size, 4)).astype(F)).astype(F)
    assert np.array_equal(np.bincount(lists, minlength=4), sizes)
    ix = _flat_index(coarse, K.SQUARED_EUCLIDEAN, lists, rows)
    long_q = (coarse[[0, 0, 0]] + F(0.01) * rng.standard_normal((3, 4)).astype(F)).astype(F)
    short_q = (coarse[[2, 3, 1]] + F([1.0, 0.0, 0.0, 0.0])).astype(F)  # a unit off the centroid: true distances near 1
    inf = np.full(3, np.inf, F)
    for nprobe, per_long, per_short in ((1, [longest] * 3, [5, 6, 8]), (2, [longest + 8] * 3, [11, 11, 13])):
        assert (longest + 8 * (nprobe - 1)) % 4 == longest % 4  # wstride: the nprobe largest lists
        first = ix.range_search(long_q, inf, nprobe=nprobe)
        assert np.diff(first[0].astype(np.int64)).tolist() == per_long
        # what stays in W: finite, and the long list's positions, the first of every query, below every radius used next
        assert np.isfinite(first[2]).all() and int((first[2] < 0.1).sum()) == 3 * longest
        want = RR.search(K.SQUARED_EUCLIDEAN, coarse, lists, rows, short_q, nprobe, inf)
        assert np.diff(want[0].astype(np.int64)).tolist() == per_short
        probed = ([2], [3], [1]) if nprobe == 1 else ([2, 3], [3, 2], [1, 2])
        for j in range(3):  # exactly the rows of its lists, in ascending id
            assert np.array_equal(want[1][int(want[0][j]):int(want[0][j + 1])], np.flatnonzero(np.isin(lists, probed[j])))
        _assert_same(ix.range_search(short_q, inf, nprobe=nprobe), want)
        tight = np.array([np.nextafter(want[2][int(want[0][j]):int(want[0][j + 1])].max(), F(np.inf)) for j in range(3)], F)
        assert tight.min() > 0.5
        _assert_same(ix.range_search(short_q, tight, nprobe=nprobe), want)
    ix.close()


@pytest.fixture(scope="module")
def two_batches():
    """1030 queries (batches of 1024 and 6) over 6000 x 4 in 8 lists, nprobe 2, a radius with some tens of hits per query"""
    rng = np.random.default_rng(41)
    n, d, nlist = 6000, 4, 8
    coarse = (3.0 * rng.standard_normal((nlist, d))).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = (coarse[lists] + rng.standard_normal((n, d)).astype(F)).astype(F)
    Q = (coarse[rng.integers(0, nlist, 1030)] + rng.standard_normal((1030, d)).astype(F)).astype(F)
    r = np.full(1030, 0.7, F)
    return coarse, lists, rows, Q, r, RR.search(K.EUCLIDEAN, coarse, lists, rows, Q, 2, r)


def test_two_batches_and_two_growths(two_batches):
    coarse, lists, rows, Q, r, want = two_batches
    first, total = int(want[0][1024]), int(want[0][-1])
    # the buffers grow after the first batch (to `first` hits) and again after the second
    assert first > 2 * RANGE_INIT_CAP and total > first
    ix = _flat_index(coarse, K.EUCLIDEAN, lists, rows)
    got = ix.range_search(Q, r, nprobe=2)
    _assert_same(got, want)
    _assert_same(ix.range_search(Q, r, nprobe=2), got)  # the same call again: identical arrays


def test_cap(two_batches):
    import vq_amd
    from vq_amd import _lib

    coarse, lists, rows, Q, r, want = two_batches
    total = int(want[0][-1])
    ix = _flat_index(coarse, K.EUCLIDEAN, lists, rows)
    with pytest.raises(vq_amd.FfiError) as e:
        ix.range_search(Q, r, nprobe=2, max_results=total - 1)
    assert e.value.status == _lib.ERR_UNSUPPORTED and str(total) in str(e.value) and str(total - 1) in str(e.value)
    _assert_same(ix.range_search(Q, r, nprobe=2, max_results=total), want)  # exactly at the cap
    with pytest.raises(vq_amd.FfiError) as e:
        ix.range_search(Q, r, nprobe=2, max_results=1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    got = ix.search(Q[:9], topk=10, nprobe=2)  # the index is usable afterwards
    wi, wd = IF.search(K.EUCLIDEAN, coarse, lists, rows, Q[:9], 2, 10)
    assert np.array_equal(got[0], wi) and np.array_equal(_bits(got[1]), _bits(wd))


def test_add_between_calls_and_an_index_without_rows():
    import vq_amd

    rng = np.random.default_rng(51)
    coarse, lists, rows, Q = _case(rng, 4000, 6, 5, np.float32, 5)
    ix = vq_amd.IVFFlatIndex(coarse, _dist(K.MANHATTAN))
    lims, idx, dist = ix.range_search(Q, np.inf, nprobe=6)  # no rows yet
    assert lims.tolist() == [0] * 6 and idx.size == 0 and dist.size == 0
    r = _tied_radii(K.MANHATTAN, Q, rows)
    ix.add_rows(lists[:1500], rows[:1500])
    _assert_same(ix.range_search(Q, r, nprobe=2), RR.search(K.MANHATTAN, coarse, lists[:1500], rows[:1500], Q, 2, r))
    ix.add_rows(lists[1500:], rows[1500:])  # the device state is rebuilt by the next call
    _assert_same(ix.range_search(Q, r, nprobe=2), RR.search(K.MANHATTAN, coarse, lists, rows, Q, 2, r))
    sx = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(-1.0, 1.0, 256))
    assert sx.range_search(Q, np.inf, nprobe=1)[0].tolist() == [0] * 6


def _read_device(ptr, count, dtype):
    import torch

    from vq_amd import _lib

    t = torch.zeros(max(count, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if count:
        _lib.memcpy_device(t.data_ptr(), ptr, count * np.dtype(dtype).itemsize)
    _lib.synchronize()
    return t.cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype)


@pytest.mark.parametrize("which", ["flat", "scalar"])
def test_device_form_at_an_offset_pointer(which):
    """queries at a device pointer offset by 4 bytes from an allocation; the RangeResult's device arrays are what read()
    returns"""
    import torch

    import vq_amd

    rng = np.random.default_rng(12)
    n, d, nq, nlist = 3001, 37, 9, 7
    sq = SI.QUANTIZERS[0]
    if which == "flat":
        coarse, lists, rows, Q = _case(rng, n, nlist, d, np.float32, nq)
        ix = _flat_index(coarse, K.COSINE, lists, rows)
    else:
        coarse = rng.uniform(-1, 1, (nlist, d)).astype(F)
        lists = _lists(rng, n, nlist, empty=2)
        codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
        codes[n - 7:], lists[n - 7:] = codes[:7], lists[:7]
        rows = SI.decode(sq, codes)
        Q = rng.uniform(-1, 1, (nq, d)).astype(F)
        ix = _sq_index(coarse, K.COSINE, lists, sq, codes)
    r = _tied_radii(K.COSINE, Q, rows)
    want = RR.search(K.COSINE, coarse, lists, rows, Q, 3, r)
    qb = torch.zeros(nq * d + 9, dtype=torch.float32, device="cuda:0")
    qb[1:1 + nq * d] = torch.from_numpy(Q.ravel()).to("cuda:0")
    torch.cuda.synchronize()
    res = ix.range_search_device(qb.data_ptr() + 4, nq, r, nprobe=3)
    assert isinstance(res, vq_amd.RangeResult) and res.nq == nq and res.total == int(want[0][-1])
    assert np.array_equal(res.lims, want[0])
    _assert_same(res.read(), want)
    pl, pi, pd = res.device_pointers()
    got = (_read_device(pl, nq + 1, np.uint64), _read_device(pi, res.total, np.uint32), _read_device(pd, res.total, F))
    _assert_same(got, want)
    empty = ix.range_search_device(qb.data_ptr() + 4, 0, np.empty(0, F), nprobe=3)
    assert empty.total == 0 and empty.lims.tolist() == [0]
    assert all(a.size == b for a, b in zip(empty.read(), (1, 0, 0)))
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.range_search_device(qb.data_ptr() + 2, nq, r, nprobe=3)


@pytest.mark.parametrize("metric", K.METRICS)
def test_consistent_with_search(metric):
    """radius = the 10th reported distance of search at the same nprobe: sorted by (key, row), the range result starts
    with search's ten"""
    rng = np.random.default_rng(30 + metric)
    coarse, lists, rows, Q = _case(rng, 5003, 8, 24, np.float32, 6)
    rows[40:45], lists[40:45] = rows[41], lists[41]
    rows[4000] = np.nan  # a NaN row, never among the first ten
    Q[2] = rows[41]
    ix = _flat_index(coarse, metric, lists, rows)
    for nprobe in (1, 3):
        si, sd = ix.search(Q, topk=10, nprobe=nprobe)
        assert not np.isnan(sd).any() and (si != IF.PAD_ID).all()
        lims, idx, dist = ix.range_search(Q, sd[:, 9].copy(), nprobe=nprobe)
        for j in range(6):
            a, b = int(lims[j]), int(lims[j + 1])
            assert b - a >= 10
            order = np.lexsort((idx[a:b], K.key(dist[a:b])))
            assert np.array_equal(idx[a:b][order][:10], si[j])
            assert np.array_equal(dist[a:b][order][:10].view(np.uint32), sd[j].view(np.uint32))
