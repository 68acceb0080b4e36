"""Exact range search on the MI355X (FlatIndex.range_search, ScalarIndex.range_search, vqhip_*_range_search, the range
stage of vq_amd/csrc/range.hpp) against the numpy statement of include/vqhip.h (tests/ref_range.py).  Every comparison
is exact: lims equal, idx equal, dist equal as uint32 bits.  All five metrics, f32 and f16 rows, radii exactly on a
boundary with ties, +inf and negative radii, n around the stage's 4096-row blocks and the 64-lane waves with every lane
emitting, dense and empty results, several query batches with the result buffers growing, the cap, determinism, the
device form, the scalar index on each of its loaders, and consistency with search."""
import os
import re

import numpy as np
import pytest

import ref_knn as K
import ref_range as R
import ref_sqindex as SI

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# hits the result buffers hold before they first grow (kRangeInitCap, vq_amd/csrc/range.hpp); the growth tests assume
# this value and check that the library still has it
RANGE_INIT_CAP = 1024


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


def _data(n, d, rng, nq=5):
    """the data of tests/test_gpu_knn.py: special rows, exact duplicates, a query equal to a duplicated row, the zero query"""
    X = (rng.standard_normal((n, d)) * 1.5).astype(F)
    sp = K.special_rows(d, rng)
    X[7:7 + len(sp)] = sp
    X[n - 3:] = X[20:23]  # exact duplicates of rows 20..22
    X[100 % n] = X[7 % n] if n > 100 else X[100 % n]
    Q = (rng.standard_normal((nq, d))).astype(F)
    Q[0] = X[21]  # a query equal to a duplicated row
    if nq > 3:
        Q[3] = 0.0  # the zero query (cosine: the EPSILON rule)
    return Q, X


def _boundary_radii(metric, Q, X, k=17):
    """per query the distance of its k-th nearest row -- the <= boundary, ties included; query 3 (the zero query) gets
    +inf and query 4 gets -1"""
    r = R.kth_distance(metric, Q, X, k)
    r[3] = np.inf
    r[4] = -1.0
    assert not np.isnan(r).any()
    return r


def test_initial_capacity_is_the_one_assumed():
    text = open(os.path.join(ROOT, "vq_amd", "csrc", "range.hpp")).read()
    assert int(re.search(r"kRangeInitCap\s*=\s*(\d+)", text).group(1)) == RANGE_INIT_CAP


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [1, 5, 33, 128])
def test_range_matches_statement(metric, dtype, d):
    import vq_amd

    rng = np.random.default_rng(1000 * metric + d)
    Q, X = _data(1037, d, rng)
    with np.errstate(over="ignore"):
        Xt = X.astype(dtype)
    Xw = Xt.astype(F)
    r = _boundary_radii(metric, Q, Xw)
    want = R.search(metric, Q, Xw, r)
    per = np.diff(want[0].astype(np.int64))
    assert (per[:3] >= 17).all() and per[4] == 0 or metric == K.COSINE_UNCLAMPED
    if d >= 5:  # the duplicated pair (21, n - 2) of query 0 sits on or inside the boundary together
        h0 = want[1][:per[0]]
        assert 21 in h0 and 1035 in h0
    got = vq_amd.FlatIndex(Xt, _dist(metric)).range_search(Q, r)
    _assert_same(got, want)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4095, 4096, 4097, 8193, 8196])
def test_block_and_wave_edges(n):
    """radius +inf: every lane position of every block emits, in row order; radius 0 at a query planted at row n - 1: one
    hit, in the last block's last row.  n % 4 == 0 takes the float4 loads, every other n the scalar ones."""
    import vq_amd

    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 8)).astype(F)
    Q = rng.standard_normal((2, 8)).astype(F)
    Q[1] = X[n - 1]
    r = np.array([np.inf, 0.0], F)
    for metric in (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN):
        got = vq_amd.FlatIndex(X, _dist(metric)).range_search(Q, r)
        assert got[0].tolist() == [0, n, n + 1] and np.array_equal(got[1][:n], np.arange(n, dtype=np.uint32))
        assert got[1][n] == n - 1 and got[2][n] == 0.0
        _assert_same(got, R.search(metric, Q, X, r))


def test_hits_in_scattered_lanes_keep_row_order():
    """a third of the rows hit, scattered over lanes, waves, strides and three blocks"""
    import vq_amd

    rng = np.random.default_rng(17)
    n = 3 * 4096 + 2048
    X = rng.random((n, 4)).astype(F)
    Q = np.zeros((3, 4), F)
    r = np.array([0.9, 0.2, 1.5], F)  # Manhattan distance = the sum of four uniforms
    got = vq_amd.FlatIndex(X, _dist(K.MANHATTAN)).range_search(Q, r)
    want = R.search(K.MANHATTAN, Q, X, r)
    assert 0 < want[0][1] < n and 0 < want[0][2] - want[0][1] < want[0][1]
    _assert_same(got, want)


def test_dense_ties_and_nothing_just_below():
    """20 000 equal rows and a NaN row (the data of test_dense_ties): the common distance as radius takes n - 1 rows, the
    float below it none"""
    import vq_amd

    X = np.ones((20_000, 16), F)
    X[5] = np.nan
    Q = np.zeros((2, 16), F)
    ix = vq_amd.FlatIndex(X, _dist(K.MANHATTAN))
    r = np.array([16.0, np.nextafter(F(16.0), F(0.0))], F)
    got = ix.range_search(Q, r)
    assert got[0].tolist() == [0, 19_999, 19_999] and 5 not in got[1]
    _assert_same(got, R.search(K.MANHATTAN, Q, X, r))


def test_all_nan_distances_give_nothing():
    import vq_amd

    X = np.full((300, 8), np.nan, F)
    got = vq_amd.FlatIndex(X).range_search(np.zeros((3, 8), F), np.inf)
    assert got[0].tolist() == [0, 0, 0, 0] and got[1].size == 0 and got[2].size == 0


@pytest.fixture(scope="module")
def several_batches():
    """1100 queries over 300 007 x 4 (768 queries per batch, as test_several_batches), the radius at each query's 5th
    neighbour: the statement, computed once"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300_007, 4)).astype(F)
    Q = rng.standard_normal((1100, 4)).astype(F)
    r, want = R.search_kth(K.SQUARED_EUCLIDEAN, Q, X, 5)
    return X, Q, r, want


def test_several_batches_and_two_growths(several_batches):
    import vq_amd

    X, Q, r, want = several_batches
    first, total = int(want[0][768]), int(want[0][-1])
    # the buffers grow after the first batch (to `first` hits) and again after the second
    assert first > 2 * RANGE_INIT_CAP and total > first
    ix = vq_amd.FlatIndex(X, vq_amd.Distance.squared_euclidean())
    got = ix.range_search(Q, r)
    _assert_same(got, want)
    _assert_same(ix.range_search(Q, r), got)  # the same call again: identical arrays


@pytest.fixture(scope="module")
def dense_case():
    """40 queries over 5000 x 8 at +inf: 200 000 hits in one batch"""
    rng = np.random.default_rng(4)
    X = rng.standard_normal((5000, 8)).astype(F)
    Q = rng.standard_normal((40, 8)).astype(F)
    return X, Q, R.search(K.EUCLIDEAN, Q, X, np.inf)


def test_two_hundred_thousand_hits(dense_case):
    import vq_amd

    X, Q, want = dense_case
    assert want[0][-1] == 200_000 > 2 * RANGE_INIT_CAP
    got = vq_amd.FlatIndex(X).range_search(Q, np.inf)
    _assert_same(got, want)


def test_cap(dense_case):
    import vq_amd
    from vq_amd import _lib

    X, Q, want = dense_case
    ix = vq_amd.FlatIndex(X)
    with pytest.raises(vq_amd.FfiError) as e:
        ix.range_search(Q, np.inf, max_results=199_999)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "200000" in str(e.value) and "199999" in str(e.value)
    _assert_same(ix.range_search(Q, np.inf, max_results=200_000), want)
    with pytest.raises(vq_amd.FfiError) as e:
        ix.range_search(Q, np.inf, max_results=1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    gi, gd = ix.search(Q, 10)  # the index is usable afterwards
    wi, wd = K.search(K.EUCLIDEAN, Q, X, 10)
    assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def test_determinism():
    import vq_amd

    rng = np.random.default_rng(6)
    Q, X = _data(9001, 24, rng, 7)
    ix = vq_amd.FlatIndex(X, _dist(K.COSINE))
    r = R.kth_distance(K.COSINE, Q, X, 300)
    a = ix.range_search(Q, r)
    b = ix.range_search(Q, r)
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
               for x, y in zip(a, b))
    _assert_same(a, R.search(K.COSINE, Q, X, r))


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
    d, nq = 37, 9
    sq = SI.QUANTIZERS[0]
    if which == "flat":
        Q, X = _data(2001, d, rng, nq)
        ix = vq_amd.FlatIndex(X, _dist(K.COSINE))
    else:
        codes = rng.integers(0, 256, (2001, d), dtype=np.uint8)
        codes[1998:] = codes[20:23]
        X = SI.decode(sq, codes)
        Q = rng.uniform(-1, 1, (nq, d)).astype(F)
        Q[0] = X[21]
        ix = vq_amd.ScalarIndex.from_codes(codes, vq_amd.ScalarQuantizer(*sq), _dist(K.COSINE))
    r = _boundary_radii(K.COSINE, Q, X)
    want = R.search(K.COSINE, Q, X, r)
    qb = torch.zeros(nq * d + 9, dtype=torch.float32, device="cuda:0")
    qb[1:1 + nq * d] = torch.from_numpy(Q.ravel()).to("cuda:0")
    torch.cuda.synchronize()
    res = ix.range_search_device(qb.data_ptr() + 4, nq, r)
    assert isinstance(res, vq_amd.RangeResult) and res.nq == nq and res.total == int(want[0][-1])
    assert np.array_equal(res.lims, want[0])
    _assert_same(res.read(), want)
    pl, pi, pd = res.device_pointers()
    got = (_read_device(pl, nq + 1, np.uint64), _read_device(pi, res.total, np.uint32), _read_device(pd, res.total, F))
    _assert_same(got, want)
    empty = ix.range_search_device(qb.data_ptr() + 4, 0, np.empty(0, F))
    assert empty.total == 0 and empty.lims.tolist() == [0]
    assert all(a.size == b for a, b in zip(empty.read(), (1, 0, 0)))
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.range_search_device(qb.data_ptr() + 2, nq, r)


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", [3, 16, 100])  # the byte, the 16-byte and the 4-byte loader of SqRows (k_knn_dist)
def test_scalar_index_matches_statement_and_flat(metric, d):
    import vq_amd

    rng = np.random.default_rng(50 * metric + d)
    for sq in (SI.QUANTIZERS[0], SI.QUANTIZERS[2]):
        codes = rng.integers(0, sq[2], (1037, d), dtype=np.uint8)
        codes[1034:] = codes[20:23]
        X = SI.decode(sq, codes)
        mn, mx = max(sq[0], -4.0), min(sq[1], 4.0)
        Q = (mn + (mx - mn) * rng.random((5, d))).astype(F)
        Q[0] = X[21]
        Q[3] = 0.0
        r = _boundary_radii(metric, Q, X)
        want = R.sq_search(metric, Q, sq, codes, r)
        got = vq_amd.ScalarIndex.from_codes(codes, vq_amd.ScalarQuantizer(*sq), _dist(metric)).range_search(Q, r)
        _assert_same(got, want)
        _assert_same(vq_amd.FlatIndex(X, _dist(metric)).range_search(Q, r), got)


def test_scalar_index_unaligned_host_buffers_and_rows_source():
    """codes offset by one byte and queries by one element on the host; an index built from f32 rows"""
    import vq_amd

    rng = np.random.default_rng(8)
    sq = SI.QUANTIZERS[0]
    n, d, nq = 777, 36, 5
    buf = np.zeros(n * d + 1, np.uint8)
    codes = buf[1:].reshape(n, d)
    codes[:] = rng.integers(0, 256, (n, d), dtype=np.uint8)
    qbuf = np.zeros(nq * d + 1, F)
    Q = qbuf[1:].reshape(nq, d)
    Q[:] = rng.uniform(-1, 1, (nq, d)).astype(F)
    q = vq_amd.ScalarQuantizer(*sq)
    r = R.kth_distance(K.EUCLIDEAN, Q, SI.decode(sq, codes), 17)
    want = R.sq_search(K.EUCLIDEAN, Q, sq, codes, r)
    _assert_same(vq_amd.ScalarIndex.from_codes(codes, q).range_search(Q, r), want)
    rows = SI.decode(sq, codes)  # rows that encode back to these codes
    ix = vq_amd.ScalarIndex(rows, q)
    assert np.array_equal(ix.codes(), codes)
    _assert_same(ix.range_search(Q, r), want)


@pytest.mark.parametrize("metric", K.METRICS)
def test_consistent_with_search(metric):
    """radius = the 10th reported distance of search: sorted by (key, row), the range result starts with search's ten"""
    import vq_amd

    rng = np.random.default_rng(30 + metric)
    X = rng.standard_normal((5003, 24)).astype(F)
    X[40:45] = X[41]
    X[4000] = np.nan  # a NaN row, never among the first ten
    Q = rng.standard_normal((6, 24)).astype(F)
    Q[2] = X[41]
    ix = vq_amd.FlatIndex(X, _dist(metric))
    si, sd = ix.search(Q, 10)
    assert not np.isnan(sd).any()
    lims, idx, dist = ix.range_search(Q, sd[:, 9].copy())
    for j in range(6):
        a, b = int(lims[j]), int(lims[j + 1])
        assert b - a >= 10
        order = np.lexsort((idx[a:b], K.key(dist[a:b])))
        assert np.array_equal(idx[a:b][order][:10], si[j])
        assert np.array_equal(dist[a:b][order][:10].view(np.uint32), sd[j].view(np.uint32))
