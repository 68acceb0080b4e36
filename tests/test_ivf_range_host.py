"""Inverted-file range search without a GPU: the numpy statement (tests/ref_ivf_range.py) against a literal double loop
and at the special radii, and every argument check of the new C ABI calls and Python methods that is decided before any
device work."""
import ctypes
import math

import numpy as np
import pytest

import ref_ivf_range as RR
import ref_ivfflat as IF
import ref_knn as K
import ref_sqindex as SI

F = np.float32
NAMES = ["vqhip_ivfflat_range_search", "vqhip_ivfflat_range_search_device", "vqhip_ivfsq_range_search",
         "vqhip_ivfsq_range_search_device"]


def _brute(metric, coarse, lists, X, Q, nprobe, r):
    """one (query, row) pair at a time: is the row's list probed, is its distance within the radius"""
    P = IF.probe(metric, coarse, Q, nprobe)
    lims, idx, dist = [0], [], []
    for j in range(Q.shape[0]):
        for i in range(X.shape[0]):
            if int(lists[i]) not in [int(l) for l in P[j]]:
                continue
            d = K.distances(metric, Q[j], X[i:i + 1])[0]
            if not math.isnan(float(d)) and float(d) <= float(r[j]):
                idx.append(i)
                dist.append(d)
        lims.append(len(idx))
    return np.array(lims, np.uint64), np.array(idx, np.uint32), np.array(dist, F)


@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_matches_double_loop(metric):
    rng = np.random.default_rng(metric)
    coarse = rng.standard_normal((5, 3)).astype(F)
    lists = rng.integers(0, 4, 31).astype(np.uint32)  # list 4 stays empty
    X = (coarse[lists] + F(0.3) * rng.standard_normal((31, 3)).astype(F)).astype(F)
    X[4] = np.nan
    X[9], lists[9] = X[2], lists[2]
    Q = rng.standard_normal((4, 3)).astype(F)
    Q[1] = X[2]
    r = np.array([K.distances(metric, Q[j], X[j + 1:j + 2])[0] for j in range(4)], F)
    r[1] = K.distances(metric, Q[1], X[2:3])[0]  # rows 2 and 9 tie on the boundary
    r[3] = np.inf
    for nprobe in (1, 2, 5):
        got = RR.search(metric, coarse, lists, X, Q, nprobe, r)
        want = _brute(metric, coarse, lists, X, Q, nprobe, r)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        assert got[0][0] == 0 and got[0][-1] == got[1].size == got[2].size
        for j in range(4):
            assert (np.diff(got[1][int(got[0][j]):int(got[0][j + 1])].astype(np.int64)) > 0).all()  # ascending row id
    full = RR.search(metric, coarse, lists, X, Q, 5, r)
    assert int(full[0][4] - full[0][3]) == 30  # +inf over every list: all but the NaN row
    import ref_range as R

    dense = R.search(metric, Q, X, r)  # nprobe == nlist is the dense statement
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b)
               for a, b in zip(full, dense))


def test_statement_special_radii():
    coarse = np.array([[0.0], [10.0]], F)
    X = np.array([[0.0], [-0.0], [1.0], [np.nan], [np.inf], [2.0], [9.0]], F)
    lists = np.array([0, 0, 0, 0, 0, 0, 1], np.uint32)
    q = np.zeros((1, 1), F)
    man = K.MANHATTAN  # list 0: distances 0, 0, 1, NaN, inf, 2; list 1: 9

    def ids(radius, nprobe=1):
        return RR.search(man, coarse, lists, X, q, nprobe, radius)[1].tolist()

    assert ids(0.0) == [0, 1] and ids(-0.0) == [0, 1]  # -0.0 <= 0.0 and 0.0 <= -0.0: floats, not keys
    assert ids(np.inf) == [0, 1, 2, 4, 5]  # every row of S(q) that is not NaN, +inf included; row 6 is not probed
    assert ids(np.inf, 2) == [0, 1, 2, 4, 5, 6]
    assert ids(-1.0) == [] and ids(-np.inf, 2) == []
    assert ids(9.0) == [0, 1, 2, 5] and ids(9.0, 2) == [0, 1, 2, 5, 6]
    assert ids(np.nextafter(F(1.0), F(0.0))) == [0, 1]
    lims, idx, dist = RR.search(man, coarse, lists, X, np.empty((0, 1), F), 1, np.empty(0, F))
    assert lims.tolist() == [0] and idx.size == 0 and dist.size == 0  # no queries
    lims, idx, _ = RR.search(man, coarse, np.empty(0, np.uint32), np.empty((0, 1), F), q, 2, np.inf)
    assert lims.tolist() == [0, 0] and idx.size == 0  # no rows


def test_scalar_statement_is_the_flat_one_over_decoded_rows():
    rng = np.random.default_rng(5)
    sq = SI.QUANTIZERS[2]
    coarse = rng.standard_normal((3, 5)).astype(F)
    lists = rng.integers(0, 3, 40).astype(np.uint32)
    codes = rng.integers(0, 17, (40, 5)).astype(np.uint8)
    Q = rng.standard_normal((3, 5)).astype(F)
    a = RR.sq_search(K.EUCLIDEAN, coarse, lists, sq, codes, Q, 2, 4.0)
    b = RR.search(K.EUCLIDEAN, coarse, lists, SI.decode(sq, codes), Q, 2, 4.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and 0 < a[1].size < 120


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


def _handle(lib, name, nlist=3, dim=4):
    L = lib.load()
    f32p = ctypes.POINTER(ctypes.c_float)
    coarse = np.arange(nlist * dim, dtype=F)
    h = ctypes.c_void_p()
    if "ivfflat" in name:
        assert L.vqhip_ivfflat_create(coarse.ctypes.data_as(f32p), nlist, dim, 0, 1, ctypes.byref(h)) == lib.OK
        return h, L.vqhip_ivfflat_destroy
    assert L.vqhip_ivfsq_create(-1.0, 1.0, 256, coarse.ctypes.data_as(f32p), nlist, dim, 1, ctypes.byref(h)) == lib.OK
    return h, L.vqhip_ivfsq_destroy


@pytest.mark.parametrize("name", NAMES)
def test_cabi_argument_checks_need_no_device(lib, name):
    """out, the pointers, max_results and the radii are checked before the index handle is looked at; nprobe right after"""
    fn = getattr(lib.load(), name)
    f32p = ctypes.POINTER(ctypes.c_float)
    q = np.zeros((2, 4), F)
    qp = q.ctypes.data_as(f32p) if not name.endswith("_device") else ctypes.c_void_p(q.ctypes.data)
    good = np.array([1.0, np.inf], F)
    bad = np.array([1.0, np.nan], F)
    gp = good.ctypes.data_as(f32p)
    out = ctypes.c_void_p(1)
    assert fn(None, qp, 2, 1, gp, 10, None) == lib.ERR_NULL_PTR
    assert fn(None, None, 2, 1, gp, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert fn(None, qp, 2, 1, None, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert fn(None, qp, 2, 1, gp, 0, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert fn(None, qp, 2, 1, bad.ctypes.data_as(f32p), 10, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "NaN" in lib.last_error() and "query 1" in lib.last_error()
    assert fn(None, qp, 2, 1, gp, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None
    h, destroy = _handle(lib, name)
    try:
        for nprobe in (0, 4, 1025):  # nlist = 3
            out = ctypes.c_void_p(1)
            assert fn(h, qp, 2, nprobe, gp, 10, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
            assert "nprobe" in lib.last_error() and out.value is None
        assert fn(h, qp, 0, 0, None, 10, ctypes.byref(out)) == lib.ERR_INVALID_INPUT  # nprobe is checked with no queries too
        assert "nprobe" in lib.last_error()
        if name.endswith("_device"):
            assert fn(h, ctypes.c_void_p(q.ctypes.data + 2), 2, 1, gp, 10, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
            assert "aligned" in lib.last_error()
    finally:
        assert destroy(h) == lib.OK


def _indexes():
    import vq_amd

    coarse = np.arange(12, dtype=F).reshape(3, 4)
    flat = vq_amd.IVFFlatIndex(coarse)
    flat.add_rows([0, 2], np.zeros((2, 4), F))
    sq = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(-1.0, 1.0, 256))
    sq.add_codes([0, 2], np.zeros((2, 4), np.uint8))
    return flat, sq


@pytest.mark.parametrize("which", [0, 1])
def test_python_argument_checks_need_no_device(lib, which):
    import vq_amd
    from vq_amd.errors import DimensionMismatch, InvalidParameter

    ix = _indexes()[which]
    Q = np.zeros((2, 4), F)
    for call in (lambda **kw: ix.range_search(Q, **kw), lambda **kw: ix.range_search_device(256, 2, **kw)):
        with pytest.raises(InvalidParameter, match="NaN"):
            call(radius=[1.0, np.nan])
        with pytest.raises(InvalidParameter, match="NaN"):
            call(radius=np.nan)
        with pytest.raises(DimensionMismatch):
            call(radius=[1.0, 2.0, 3.0])  # wrong radius count
        with pytest.raises(InvalidParameter, match="radius"):
            call(radius=np.zeros((2, 1), F))
        with pytest.raises(InvalidParameter, match="radius"):
            call(radius="x")
        for nprobe in (0, 4, 1025, 1.5):
            with pytest.raises(InvalidParameter, match="nprobe"):
                call(radius=1.0, nprobe=nprobe)
        for m in (0, -1, 1 << 64, 2.5):
            with pytest.raises(InvalidParameter, match="max_results"):
                call(radius=1.0, nprobe=1, max_results=m)
    with pytest.raises(DimensionMismatch):
        ix.range_search(np.zeros((2, 5), F), 1.0)
    with pytest.raises(InvalidParameter, match="nq"):
        ix.range_search_device(256, -1, 1.0, nprobe=1)
    lims, idx, dist = ix.range_search(np.empty((0, 4), F), np.empty(0, F), nprobe=1)  # no queries: no device either
    assert lims.tolist() == [0] and lims.dtype == np.uint64 and idx.dtype == np.uint32 and dist.dtype == F
    assert idx.size == 0 and dist.size == 0
    assert ix._ix is None  # none of this created the device handle


def test_ivfpq_has_no_range_search():
    import vq_amd
    from vq_amd import _lib

    assert not hasattr(vq_amd.IVFPQIndex, "range_search") and not hasattr(vq_amd.IVFPQIndex, "range_search_device")
    assert not hasattr(_lib.IVFPQ, "range_search") and not hasattr(_lib.IVFPQ, "range_search_device")
    assert not any(n.startswith("vqhip_ivfpq_range") for n in _lib.SIGNATURES)
    assert all(n in _lib.SIGNATURES for n in NAMES)
    for cls in (vq_amd.IVFFlatIndex, vq_amd.IVFScalarIndex):
        assert callable(cls.range_search) and callable(cls.range_search_device)
