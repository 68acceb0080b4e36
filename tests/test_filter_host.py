"""Filtered search without a GPU: ``vq_amd.pack_row_mask`` against np.packbits, the numpy statement (tests/ref_filter.py)
against a brute-force loop, and the argument checks of the Python classes and of the eight C entry points, all of which
come before any device work."""
import ctypes

import numpy as np
import pytest

import ref_filter as RF
import ref_knn as K

F = np.float32
SIZES = (1, 31, 32, 33, 64, 65, 1037)


def _packbits_words(m):
    by = np.packbits(m, bitorder="little")
    pad = np.zeros((len(m) + 31) // 32 * 4, np.uint8)
    pad[:len(by)] = by
    return pad.view("<u4")


@pytest.mark.parametrize("n", SIZES)
def test_pack_row_mask_is_little_endian_packbits(n):
    import vq_amd

    rng = np.random.default_rng(n)
    for m in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
        w = vq_amd.pack_row_mask(m, n)
        assert w.dtype == np.uint32 and w.shape == ((n + 31) // 32,)
        assert np.array_equal(w, _packbits_words(m)) and np.array_equal(w, RF.pack(m))
        assert np.array_equal(RF.unpack(w, n), m)
        for i in np.flatnonzero(m)[:5]:
            assert (int(w[i >> 5]) >> (i & 31)) & 1
        if n % 32:  # the pad bits are zero
            assert int(w[-1]) >> (n % 32) == 0
        ids = np.flatnonzero(m)
        assert np.array_equal(vq_amd.pack_row_mask(ids, n), w)
        assert np.array_equal(vq_amd.pack_row_mask(np.concatenate([ids[::-1], ids]).astype(np.uint32), n), w)  # any order, repeats
        assert np.array_equal(vq_amd.pack_row_mask(ids.tolist() if ids.size else np.empty(0, np.int64), n), w)


def test_pack_row_mask_checks():
    import vq_amd

    for bad in ([5], [-1], [0, 1, 7]):
        with pytest.raises(vq_amd.InvalidParameter, match="outside"):
            vq_amd.pack_row_mask(np.array(bad), 5)
    with pytest.raises(vq_amd.DimensionMismatch):
        vq_amd.pack_row_mask(np.ones(6, bool), 5)
    with pytest.raises(vq_amd.InvalidParameter):
        vq_amd.pack_row_mask(np.ones(5, F), 5)
    with pytest.raises(vq_amd.InvalidParameter):
        vq_amd.pack_row_mask(np.ones((5, 1), bool), 5)
    with pytest.raises(vq_amd.InvalidParameter, match="n"):
        vq_amd.pack_row_mask(np.ones(0, bool), 0)
    assert "pack_row_mask" in vq_amd.__all__


@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_matches_a_loop_over_allowed_rows(metric):
    rng = np.random.default_rng(metric)
    X = rng.standard_normal((41, 3)).astype(F)
    X[4] = np.nan
    X[9] = X[2]
    X[30] = X[2]
    Q = rng.standard_normal((3, 3)).astype(F)
    Q[1] = X[2]
    m = rng.random(41) < 0.4
    m[[2, 4, 30]] = True
    m[9] = False
    idx, dist = RF.search(metric, Q, X, 20, m)
    na = int(m.sum())
    for j in range(3):
        d = K.distances(metric, Q[j], X)
        order = sorted(np.flatnonzero(m), key=lambda i: (int(K.key(d[i:i + 1])[0]), i))
        assert idx[j, :na].tolist() == order[:20] and (idx[j, na:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, na:]).all()
        assert np.array_equal(dist[j, :min(na, 20)].view(np.uint32), K.reported(d[order[:20]]).view(np.uint32))
        assert 9 not in idx[j]
    lims, ridx, rdist = RF.range_search(metric, Q, X, np.inf, m)
    for j in range(3):
        d = K.distances(metric, Q[j], X)
        want = [i for i in range(41) if m[i] and not np.isnan(d[i])]
        assert ridx[int(lims[j]):int(lims[j + 1])].tolist() == want
    # all ones: the unmasked statements
    ones = np.ones(41, bool)
    a, b = RF.search(metric, Q, X, 7, ones), K.search(metric, Q, X, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    # all zeros
    z = RF.search(metric, Q, X, 7, ~ones)
    assert (z[0] == 0xFFFFFFFF).all() and np.isposinf(z[1]).all()
    assert RF.range_search(metric, Q, X, np.inf, ~ones)[0].tolist() == [0, 0, 0, 0]


def _indexes(n=70, d=3):
    import vq_amd

    rows = np.zeros((n, d), F)
    sq = vq_amd.ScalarQuantizer(-1.0, 1.0, 256)
    return [vq_amd.FlatIndex(rows), vq_amd.FlatIndex(rows.astype(np.float16)), vq_amd.ScalarIndex(rows, sq),
            vq_amd.ScalarIndex.from_codes(np.zeros((n, d), np.uint8), sq)]


def _no_device(monkeypatch):
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "Flat", boom)
    monkeypatch.setattr(_lib, "SQIndex", boom)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_python_mask_checks_need_no_device(monkeypatch, which):
    import vq_amd

    _no_device(monkeypatch)
    ix = _indexes()[which]
    n = len(ix)
    Q = np.zeros((2, 3), F)
    calls = [lambda a: ix.search(Q, 5, allowed=a), lambda a: ix.range_search(Q, 1.0, allowed=a)]
    for call in calls:
        for bad in (np.ones(n, np.uint8), np.ones(n, np.int64), np.ones(n, F), np.ones(3, np.uint64), [1.5] * n):
            with pytest.raises(vq_amd.InvalidParameter, match="allowed"):
                call(bad)
        for bad in (np.ones(n + 1, bool), np.ones(n - 1, bool), np.ones(2, np.uint32), np.ones(4, np.uint32), np.ones(0, bool)):
            with pytest.raises(vq_amd.DimensionMismatch):
                call(bad)
        for bad in (np.ones((n, 1), bool), np.ones((1, 3), np.uint32), np.ones((2, n), bool)):
            with pytest.raises(vq_amd.InvalidParameter, match="allowed"):
                call(bad)
    # the other arguments keep their checks
    ok = np.ones(n, bool)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search(Q, n + 1, allowed=ok)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.search(np.zeros((2, 4), F), 5, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search(Q, np.nan, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.range_search(Q, 1.0, max_results=0, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search_device(0, 2, 0, 0, 0, dev_allowed=4)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search_device(0, 2, np.nan, dev_allowed=4)
    # no queries: the empty results, after the mask has been checked, and no device either
    for a in (ok, vq_amd.pack_row_mask(ok, n)):
        i, d = ix.search(np.zeros((0, 3), F), 5, allowed=a)
        assert i.shape == (0, 5) and i.dtype == np.uint32 and d.shape == (0, 5) and d.dtype == F
        lims, idx, dist = ix.range_search(np.zeros((0, 3), F), 1.0, allowed=a)
        assert lims.tolist() == [0] and idx.size == 0 and dist.size == 0
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.search(np.zeros((0, 3), F), 5, allowed=np.ones(n + 1, bool))
    with pytest.raises(vq_amd.InvalidParameter):
        ix.range_search(np.zeros((0, 3), F), 1.0, allowed=np.ones(n, np.int8))


def test_binary_index_keeps_its_signatures():
    import inspect

    import vq_amd

    for fn in (vq_amd.BinaryIndex.search, vq_amd.BinaryIndex.search_device, vq_amd.BinaryIndex.hamming_range_search):
        assert not {"allowed", "dev_allowed"} & set(inspect.signature(fn).parameters)
    assert "allowed" in inspect.signature(vq_amd.FlatIndex.search).parameters
    assert "dev_allowed" in inspect.signature(vq_amd.ScalarIndex.range_search_device).parameters


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


@pytest.mark.parametrize("prefix", ["vqhip_flat", "vqhip_sqindex"])
def test_cabi_search_masked_checks_need_no_device(lib, prefix):
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    idx, dist = np.zeros(2, np.uint32), np.zeros(2, F)
    qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
    host = getattr(L, prefix + "_search_masked")
    assert host(None, qp, 2, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the handle
    fake = ctypes.c_void_p(8)  # never dereferenced: a NULL pointer is found first
    assert host(fake, qp, 2, 1, None, ip, dp) == lib.ERR_NULL_PTR  # the mask
    assert host(fake, None, 2, 1, wp, ip, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, 1, wp, None, dp) == lib.ERR_NULL_PTR
    dev = getattr(L, prefix + "_search_masked_device")
    v = ctypes.c_void_p
    assert dev(None, v(q.ctypes.data), 2, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, v(q.ctypes.data), 2, 1, None, v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, None, 2, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    for off in (1, 2, 3):  # a mask pointer that is not 4-byte aligned, found before the handle is looked at
        assert dev(None, v(q.ctypes.data), 2, 1, v(w.ctypes.data + off), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()


@pytest.mark.parametrize("name", ["vqhip_flat_range_search_masked", "vqhip_flat_range_search_masked_device",
                                  "vqhip_sqindex_range_search_masked", "vqhip_sqindex_range_search_masked_device"])
def test_cabi_range_masked_checks_need_no_device(lib, name):
    """out, the pointers, max_results, the radii and the mask are checked before the index handle is looked at"""
    fn = getattr(lib.load(), name)
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    device = name.endswith("_device")
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    qp = ctypes.c_void_p(q.ctypes.data) if device else q.ctypes.data_as(f32p)
    wp = ctypes.c_void_p(w.ctypes.data) if device else w.ctypes.data_as(u32p)
    good = np.array([1.0, np.inf], F).ctypes.data_as(f32p)
    bad = np.array([1.0, np.nan], F).ctypes.data_as(f32p)
    out = ctypes.c_void_p(1)
    assert fn(None, qp, 2, good, 10, wp, None) == lib.ERR_NULL_PTR
    assert fn(None, None, 2, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert fn(None, qp, 2, None, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert fn(None, qp, 2, good, 0, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert fn(None, qp, 2, bad, 10, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "NaN" in lib.last_error()
    assert fn(ctypes.c_void_p(8), qp, 2, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the mask, before the handle
    assert fn(ctypes.c_void_p(8), qp, 0, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # with no queries too
    if device:
        assert fn(None, qp, 2, good, 10, ctypes.c_void_p(w.ctypes.data + 2), ctypes.byref(out)) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()
    assert fn(None, qp, 2, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None
