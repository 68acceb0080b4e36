"""Range search without a GPU: the numpy statement (tests/ref_range.py) against a brute-force double loop and at the
special radii, and the argument checks of the C ABI and of the Python classes, all of which come before any device work."""
import ctypes
import math

import numpy as np
import pytest

import ref_knn as K
import ref_range as R
import ref_sqindex as SI

F = np.float32


def _brute(metric, Q, X, r):
    """one pair at a time through the statement of a single distance"""
    lims, idx, dist = [0], [], []
    for j in range(Q.shape[0]):
        for i in range(X.shape[0]):
            d = K.distances(metric, Q[j], X[i:i + 1])[0]
            if not math.isnan(float(d)) and float(d) <= float(r[j]):
                idx.append(i)
                dist.append(d)
        lims.append(len(idx))
    return np.array(lims, np.uint64), np.array(idx, np.uint32), np.array(dist, F)


@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_matches_double_loop(metric):
    rng = np.random.default_rng(metric)
    X = rng.standard_normal((23, 3)).astype(F)
    X[4] = np.nan
    X[9] = X[2]
    Q = rng.standard_normal((4, 3)).astype(F)
    Q[1] = X[2]
    r = R.kth_distance(metric, Q, X, 6)
    r[3] = np.inf
    got = R.search(metric, Q, X, r)
    want = _brute(metric, Q, X, r)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert got[0][0] == 0 and got[0][-1] == got[1].size == got[2].size
    per = np.diff(got[0].astype(np.int64))
    assert (per[:3] >= 6).all() and per[3] == 22  # ties may add to the six; +inf takes all but the NaN row
    for j in range(4):
        assert (np.diff(got[1][int(got[0][j]):int(got[0][j + 1])].astype(np.int64)) > 0).all()  # ascending row id


def test_statement_special_radii():
    X = np.array([[0.0], [-0.0], [1.0], [np.nan], [np.inf], [2.0]], F)
    q = np.zeros((1, 1), F)
    man = K.MANHATTAN  # distances 0, 0, 1, NaN, inf, 2
    assert R.search(man, q, X, 0.0)[1].tolist() == [0, 1]
    assert R.search(man, q, X, -0.0)[1].tolist() == [0, 1]  # -0.0 <= 0.0 and 0.0 <= -0.0: floats, not keys
    assert R.search(man, q, X, np.inf)[1].tolist() == [0, 1, 2, 4, 5]  # every row that is not NaN, +inf included
    assert R.search(man, q, X, -1.0)[1].size == 0
    assert R.search(man, q, X, -np.inf)[1].size == 0
    assert R.search(man, q, X, 1.0)[1].tolist() == [0, 1, 2]
    assert R.search(man, q, X, np.nextafter(F(1.0), F(0.0)))[1].tolist() == [0, 1]
    # a distance of +0.0 is a hit at radius -0.0
    lims, idx, dist = R.search(K.SQUARED_EUCLIDEAN, q, X, -0.0)
    assert idx.tolist() == [0, 1] and lims.tolist() == [0, 2]
    # where D can be negative, a negative radius has hits
    Xc = np.array([[1.0, 1e-4], [1.0, 0.0], [-1.0, 0.0]], F)
    qc = np.array([[1.0, 1e-4]], F)
    d = K.distances(K.COSINE_UNCLAMPED, qc[0], Xc)
    neg = d < 0
    assert np.array_equal(R.search(K.COSINE_UNCLAMPED, qc, Xc, -1e-30)[1], np.nonzero(neg)[0].astype(np.uint32))
    assert R.search(K.COSINE, qc, Xc, -1e-30)[1].size == 0  # clamped at 0
    # no queries
    lims, idx, dist = R.search(man, np.empty((0, 1), F), X, np.empty(0, F))
    assert lims.tolist() == [0] and idx.size == 0 and dist.size == 0


def test_scalar_statement_is_the_flat_one_over_decoded_rows():
    rng = np.random.default_rng(5)
    sq = SI.QUANTIZERS[2]
    codes = rng.integers(0, 17, (40, 5)).astype(np.uint8)
    Q = rng.standard_normal((3, 5)).astype(F)
    a = R.sq_search(K.EUCLIDEAN, Q, sq, codes, 4.0)
    b = R.search(K.EUCLIDEAN, Q, SI.decode(sq, codes), 4.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and 0 < a[1].size < 120


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


@pytest.mark.parametrize("name", ["vqhip_flat_range_search", "vqhip_flat_range_search_device", "vqhip_sqindex_range_search",
                                  "vqhip_sqindex_range_search_device"])
def test_cabi_argument_checks_need_no_device(lib, name):
    """out, the pointers, max_results and the radii are checked before the index handle is looked at"""
    fn = getattr(lib.load(), name)
    f32p = ctypes.POINTER(ctypes.c_float)
    q = np.zeros((2, 4), F)
    qp = q.ctypes.data_as(f32p) if not name.endswith("_device") else ctypes.c_void_p(q.ctypes.data)
    good = np.array([1.0, np.inf], F)
    bad = np.array([1.0, np.nan], F)
    out = ctypes.c_void_p(1)
    assert fn(None, qp, 2, good.ctypes.data_as(f32p), 10, None) == lib.ERR_NULL_PTR
    assert fn(None, None, 2, good.ctypes.data_as(f32p), 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert fn(None, qp, 2, None, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert fn(None, qp, 2, good.ctypes.data_as(f32p), 0, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert fn(None, qp, 2, bad.ctypes.data_as(f32p), 10, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "NaN" in lib.last_error() and "query 1" in lib.last_error()
    assert fn(None, qp, 2, good.ctypes.data_as(f32p), 10, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None


def test_cabi_range_object_checks(lib):
    L = lib.load()
    assert L.vqhip_range_info(None, None, None) == lib.ERR_NULL_PTR
    assert L.vqhip_range_read(None, None, None, None) == lib.ERR_NULL_PTR
    assert L.vqhip_range_device(None, None, None, None) == lib.ERR_NULL_PTR
    assert L.vqhip_range_destroy(None) == lib.OK


def _indexes():
    import vq_amd

    rows = np.zeros((6, 3), F)
    return [vq_amd.FlatIndex(rows), vq_amd.ScalarIndex(rows, vq_amd.ScalarQuantizer(-1.0, 1.0, 256)),
            vq_amd.ScalarIndex.from_codes(np.zeros((6, 3), np.uint8), vq_amd.ScalarQuantizer(-1.0, 1.0, 256))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_python_argument_checks_need_no_device(which):
    import vq_amd

    ix = _indexes()[which]
    Q = np.zeros((2, 3), F)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search(Q, np.nan)
    with pytest.raises(vq_amd.InvalidParameter, match="query 1"):
        ix.range_search(Q, [1.0, np.nan])
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.range_search(Q, [1.0, 2.0, 3.0])
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.range_search(Q, np.empty(0, F))
    with pytest.raises(vq_amd.InvalidParameter, match="radius"):
        ix.range_search(Q, np.ones((2, 1), F))
    with pytest.raises(vq_amd.InvalidParameter, match="radius"):
        ix.range_search(Q, "near")
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.range_search(Q, 1.0, max_results=0)
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.range_search(Q, 1.0, max_results=2.5)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.range_search(np.zeros((2, 4), F), 1.0)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search_device(0, 2, [np.nan, 1.0])
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.range_search_device(0, 2, [1.0])
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.range_search_device(0, 2, 1.0, max_results=0)
    with pytest.raises(vq_amd.InvalidParameter, match="nq"):
        ix.range_search_device(0, -1, 1.0)
    # no queries: an empty result, and no device either
    lims, idx, dist = ix.range_search(np.empty((0, 3), F), 1.0)
    assert lims.dtype == np.uint64 and lims.tolist() == [0]
    assert idx.dtype == np.uint32 and idx.size == 0 and dist.dtype == F and dist.size == 0


def test_exports():
    import vq_amd

    assert "RangeResult" in vq_amd.__all__ and vq_amd.RangeResult is vq_amd._lib.RangeResult
