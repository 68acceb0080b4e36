"""Filtered inverted-file search without a GPU: the numpy statement (tests/ref_ivf_filter.py) against a plain loop, the
argument checks of ``IVFFlatIndex`` / ``IVFScalarIndex`` ``search(..., allowed=)`` and ``range_search(..., allowed=)`` --
all before a device is touched --, the unchanged signatures of ``IVFPQIndex`` / ``IVFBinaryIndex``, and the NULL and
invalid-argument statuses of the eight C entry points."""
import ctypes
import inspect

import numpy as np
import pytest

import ref_filter as RF
import ref_ivf_filter as RIF
import ref_ivf_range as RR
import ref_ivfflat as RI
import ref_knn as K

F = np.float32


def _case(rng, n=61, nlist=5, d=3):
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    lists[lists == 2] = 3  # an empty list
    X = (coarse[lists] + F(0.5) * rng.standard_normal((n, d)).astype(F)).astype(F)
    X[4] = np.nan
    X[9] = X[2]
    X[30] = X[2]
    lists[[9, 30]] = lists[2]
    Q = rng.standard_normal((4, d)).astype(F)
    Q[1] = X[2]
    Q[2] = coarse[2]  # its nearest list is the empty one
    m = rng.random(n) < 0.4
    m[[2, 4, 30]] = True
    m[9] = False
    return coarse, lists, X, Q, m


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("nprobe", [1, 2, 5])
def test_statement_matches_a_plain_loop(metric, nprobe):
    rng = np.random.default_rng(10 * metric + nprobe)
    coarse, lists, X, Q, m = _case(rng)
    n, topk = len(lists), 12
    P = RI.probe(metric, coarse, Q, nprobe)
    idx, dist = RIF.search(metric, coarse, lists, X, Q, nprobe, topk, m)
    lims, ridx, rdist = RIF.range_search(metric, coarse, lists, X, Q, nprobe, np.inf, m)
    for j in range(Q.shape[0]):
        d = K.distances(metric, Q[j], X)
        sa = [i for i in range(n) if m[i] and lists[i] in P[j]]  # S_a(q), by the definition
        order = sorted(sa, key=lambda i: (int(K.key(d[i:i + 1])[0]), i))[:topk]
        t = len(order)
        assert idx[j, :t].tolist() == order and (idx[j, t:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, t:]).all()
        assert np.array_equal(dist[j, :t].view(np.uint32), K.reported(d[order]).view(np.uint32))
        assert 9 not in idx[j]
        want = [i for i in sa if not np.isnan(d[i])]
        assert ridx[int(lims[j]):int(lims[j + 1])].tolist() == want
        assert np.array_equal(rdist[int(lims[j]):int(lims[j + 1])].view(np.uint32), d[want].view(np.uint32))
    # all ones: the unmasked statements; all zeros: padding only / lims == 0
    ones = np.ones(n, bool)
    a, b = RIF.search(metric, coarse, lists, X, Q, nprobe, 7, ones), RI.search(metric, coarse, lists, X, Q, nprobe, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    a, b = RIF.range_search(metric, coarse, lists, X, Q, nprobe, 1.5, ones), RR.search(metric, coarse, lists, X, Q, nprobe, 1.5)
    assert all(np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y) for x, y in zip(a, b))
    z = RIF.search(metric, coarse, lists, X, Q, nprobe, 7, ~ones)
    assert (z[0] == 0xFFFFFFFF).all() and np.isposinf(z[1]).all()
    assert RIF.range_search(metric, coarse, lists, X, Q, nprobe, np.inf, ~ones)[0].tolist() == [0] * 5
    if nprobe == 5:  # every list probed: the exact filtered statements
        a, b = RIF.search(metric, coarse, lists, X, Q, 5, topk, m), RF.search(metric, Q, X, topk, m)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        a, b = RIF.range_search(metric, coarse, lists, X, Q, 5, 1.5, m), RF.range_search(metric, Q, X, 1.5, m)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _indexes(n=70, d=3, nlist=4):
    import vq_amd

    coarse = np.arange(nlist * d, dtype=F).reshape(nlist, d)
    lists = (np.arange(n) % nlist).astype(np.uint32)
    flat = vq_amd.IVFFlatIndex(coarse)
    flat.add_rows(lists, np.zeros((n, d), F))
    half = vq_amd.IVFFlatIndex(coarse, dtype=np.float16)
    half.add_rows(lists, np.zeros((n, d), F))
    sq = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(-1.0, 1.0, 256))
    sq.add_codes(lists, np.zeros((n, d), np.uint8))
    return [flat, half, sq]


def _grow(ix, k):
    """k more rows, without a device"""
    import vq_amd

    lists = np.zeros(k, np.uint32)
    if isinstance(ix, vq_amd.IVFScalarIndex):
        ix.add_codes(lists, np.zeros((k, ix.dim), np.uint8))
    else:
        ix.add_rows(lists, np.zeros((k, ix.dim), F))


def _no_device(monkeypatch):
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "IVFFlat", boom)
    monkeypatch.setattr(_lib, "IVFSQ", boom)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_python_mask_checks_need_no_device(monkeypatch, which):
    import vq_amd

    _no_device(monkeypatch)
    ix = _indexes()[which]
    n = len(ix)
    Q = np.zeros((2, 3), F)
    calls = [lambda a: ix.search(Q, 5, 2, allowed=a), lambda a: ix.range_search(Q, 1.0, 2, allowed=a)]
    if which == 2:
        calls.append(lambda a: ix.search(Q, 5, 2, rerank=object(), allowed=a))  # the mask is checked before the reranker
    for call in calls:
        for bad in (np.ones(n, np.uint8), np.ones(n, np.int64), np.ones(n, F), np.ones(3, np.uint64), [1.5] * n):
            with pytest.raises(vq_amd.InvalidParameter, match="allowed"):  # wrong dtype
                call(bad)
        for bad in (np.ones(n + 1, bool), np.ones(n - 1, bool), np.ones(2, np.uint32), np.ones(4, np.uint32), np.ones(0, bool)):
            with pytest.raises(vq_amd.DimensionMismatch):  # wrong length
                call(bad)
        for bad in (np.ones((n, 1), bool), np.ones((1, 3), np.uint32), np.ones((2, n), bool)):
            with pytest.raises(vq_amd.InvalidParameter, match="allowed"):  # 2-D
                call(bad)
    # a word count for a stale n after add: 70 rows are 3 words, 100 rows 4
    stale_bool, stale_words = np.ones(n, bool), vq_amd.pack_row_mask(np.ones(n, bool), n)
    _grow(ix, 30)
    assert len(ix) == n + 30 and stale_words.shape == (3,)
    for call in calls[:2]:
        for stale in (stale_bool, stale_words):
            with pytest.raises(vq_amd.DimensionMismatch):
                call(stale)
    n = len(ix)
    # the other arguments keep their checks
    ok = np.ones(n, bool)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search(Q, n + 1, 2, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
        ix.search(Q, 5, 5, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
        ix.range_search(Q, 1.0, 0, allowed=ok)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.search(np.zeros((2, 4), F), 5, 2, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search(Q, np.nan, 2, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.range_search(Q, 1.0, 2, max_results=0, allowed=ok)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search_device(0, 2, 0, 0, 0, nprobe=2, dev_allowed=4)
    with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
        ix.search_device(0, 2, 5, 0, 0, nprobe=9, dev_allowed=4)
    with pytest.raises(vq_amd.InvalidParameter, match="NaN"):
        ix.range_search_device(0, 2, np.nan, nprobe=2, dev_allowed=4)
    # no queries: the empty results, after the mask has been checked, and no device either
    for a in (ok, vq_amd.pack_row_mask(ok, n)):
        i, d = ix.search(np.zeros((0, 3), F), 5, 2, allowed=a)
        assert i.shape == (0, 5) and i.dtype == np.uint32 and d.shape == (0, 5) and d.dtype == F
        lims, idx, dist = ix.range_search(np.zeros((0, 3), F), 1.0, 2, allowed=a)
        assert lims.tolist() == [0] and idx.size == 0 and dist.size == 0
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.search(np.zeros((0, 3), F), 5, 2, allowed=np.ones(n + 1, bool))
    with pytest.raises(vq_amd.InvalidParameter):
        ix.range_search(np.zeros((0, 3), F), 1.0, 2, allowed=np.ones(n, np.int8))


def test_pq_and_binary_indexes_reject_allowed():
    import vq_amd

    coarse = np.zeros((2, 4), F)
    pq = vq_amd.IVFPQIndex(coarse, np.zeros((2, 4, 2), F))
    bq = vq_amd.IVFBinaryIndex(coarse)
    Q = np.zeros((1, 4), F)
    for ix in (pq, bq):
        with pytest.raises(TypeError, match="allowed"):
            ix.search(Q, 1, 1, allowed=np.ones(1, bool))
        with pytest.raises(TypeError, match="dev_allowed"):
            ix.search_device(0, 1, 1, 0, 0, nprobe=1, dev_allowed=4)
    with pytest.raises(TypeError, match="allowed"):
        bq.hamming_range_search(Q, 1, 1, allowed=np.ones(1, bool))
    for cls in (vq_amd.IVFPQIndex, vq_amd.IVFBinaryIndex):
        for name in ("search", "search_device", "probe"):
            assert not {"allowed", "dev_allowed"} & set(inspect.signature(getattr(cls, name)).parameters)
    for cls in (vq_amd.IVFFlatIndex, vq_amd.IVFScalarIndex):
        assert "allowed" in inspect.signature(cls.search).parameters
        assert "allowed" in inspect.signature(cls.range_search).parameters
        assert "dev_allowed" in inspect.signature(cls.search_device).parameters
        assert "dev_allowed" in inspect.signature(cls.range_search_device).parameters
        assert not {"allowed", "dev_allowed"} & set(inspect.signature(cls.probe).parameters)  # probing takes no mask


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


@pytest.mark.parametrize("prefix", ["vqhip_ivfflat", "vqhip_ivfsq"])
def test_cabi_search_masked_checks_need_no_device(lib, prefix):
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    idx, dist = np.zeros(2, np.uint32), np.zeros(2, F)
    qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
    host = getattr(L, prefix + "_search_masked")
    assert host(None, qp, 2, 1, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the handle
    fake = ctypes.c_void_p(8)  # never dereferenced: a NULL pointer is found first
    assert host(fake, qp, 2, 1, 1, None, ip, dp) == lib.ERR_NULL_PTR  # the mask
    assert host(fake, None, 2, 1, 1, wp, ip, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, 1, 1, wp, None, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, 1, 1, wp, ip, None) == lib.ERR_NULL_PTR
    assert host(fake, qp, 0, 1, 1, None, ip, dp) == lib.ERR_NULL_PTR  # with no queries too
    dev = getattr(L, prefix + "_search_masked_device")
    v = ctypes.c_void_p
    assert dev(None, v(q.ctypes.data), 2, 1, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, v(q.ctypes.data), 2, 1, 1, None, v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, None, 2, 1, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    for off in (1, 2, 3):  # a mask pointer that is not 4-byte aligned, found before the handle is looked at
        assert dev(None, v(q.ctypes.data), 2, 1, 1, v(w.ctypes.data + off), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()


def _real_handle(lib, prefix):
    """an index with 40 rows in 3 lists: create and add are host-only"""
    coarse = np.zeros((3, 4), F)
    lists = (np.arange(40) % 3).astype(np.uint32)
    if prefix == "vqhip_ivfflat":
        ix = lib.IVFFlat(coarse, K.EUCLIDEAN, np.float32)
        ix.add(lists, np.zeros((40, 4), F))
    else:
        ix = lib.IVFSQ(coarse, -1.0, 1.0, 256, K.EUCLIDEAN)
        ix.add_codes(lists, np.zeros((40, 4), np.uint8))
    return ix


@pytest.mark.parametrize("prefix", ["vqhip_ivfflat", "vqhip_ivfsq"])
def test_cabi_masked_argument_ranges_need_no_device(lib, prefix):
    """nprobe and topk are held to the unmasked calls' bounds on a real handle, before any device work"""
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    ix = _real_handle(lib, prefix)
    try:
        q = np.zeros((2, 4), F)
        w = np.ones(2, np.uint32)
        idx, dist = np.zeros(2 * 41, np.uint32), np.zeros(2 * 41, F)
        qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
        host = getattr(L, prefix + "_search_masked")
        for nprobe, topk, what in ((0, 1, "nprobe"), (4, 1, "nprobe"), (1, 0, "topk"), (1, 41, "topk")):
            assert host(ix.raw, qp, 2, nprobe, topk, wp, ip, dp) == lib.ERR_INVALID_INPUT
            assert what in lib.last_error()
        rng = getattr(L, prefix + "_range_search_masked")
        out = ctypes.c_void_p(1)
        r = np.ones(2, F).ctypes.data_as(f32p)
        for nprobe in (0, 4):
            assert rng(ix.raw, qp, 2, nprobe, r, 10, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
            assert "nprobe" in lib.last_error() and out.value is None
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["vqhip_ivfflat_range_search_masked", "vqhip_ivfflat_range_search_masked_device",
                                  "vqhip_ivfsq_range_search_masked", "vqhip_ivfsq_range_search_masked_device"])
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
    assert fn(None, qp, 2, 1, good, 10, wp, None) == lib.ERR_NULL_PTR
    assert fn(None, None, 2, 1, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert fn(None, qp, 2, 1, None, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert fn(None, qp, 2, 1, good, 0, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert fn(None, qp, 2, 1, bad, 10, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "NaN" in lib.last_error()
    assert fn(ctypes.c_void_p(8), qp, 2, 1, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the mask, before the handle
    assert fn(ctypes.c_void_p(8), qp, 0, 1, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # with no queries too
    if device:
        assert fn(None, qp, 2, 1, good, 10, ctypes.c_void_p(w.ctypes.data + 2), ctypes.byref(out)) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()
    assert fn(None, qp, 2, 1, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None
