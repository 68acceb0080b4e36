"""Filtered PQ search without a GPU: the numpy statement (tests/ref_pq_filter.py) against its brute restatement and against
ref_ivf / ref_ivf_residual under an all-ones mask, the argument checks of ``PQIndex.search(allowed=)``,
``ProductQuantizer.search(allowed=)`` and ``IVFPQIndex.masked_search[_device]`` -- all before a device is touched --, the
new signatures, and the NULL / misaligned / invalid-argument statuses of the five C entry points."""
import ctypes
import inspect

import numpy as np
import pytest

import ref_ivf as R
import ref_ivf_residual as RR
import ref_knn as K
import ref_pq_filter as RPF

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _case(rng, n=83, nlist=5, m=3, k=7, sd=2):
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    lists[lists == 2] = 3  # an empty list
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    codes[[9, 30, 31]] = codes[2]  # ties by row id, on both sides of the mask
    lists[[9, 30, 31]] = lists[2]
    Q = rng.standard_normal((5, m * sd)).astype(F)
    Q[1, 2] = np.nan
    Q[2] = coarse[2]  # its nearest list is the empty one
    Q[3, 0] = np.inf
    mask = rng.random(n) < 0.4
    mask[[2, 30]] = True
    mask[[9, 31]] = False
    return coarse, cb, lists, codes, Q, mask


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nprobe", [1, 2, 5])
def test_statement_matches_its_restatement(oracle, metric, nprobe):
    rng = np.random.default_rng(10 * metric + nprobe)
    coarse, cb, lists, codes, Q, mask = _case(rng)
    n = len(lists)
    ones = np.ones(n, bool)
    for topk in (1, 12, n):
        a = RPF.search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask)
        _same(a, RPF.brute_search(metric, coarse, cb, lists, codes, Q, nprobe, topk, mask))
        assert not np.isin(a[0], np.flatnonzero(~mask)).any()
        r = RPF.residual_search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask)
        _same(r, RPF.brute_residual_search(metric, coarse, cb, lists, codes, Q, nprobe, topk, mask))
        assert not np.isin(r[0], np.flatnonzero(~mask)).any()
        # all ones: the unfiltered statements; all zeros: padding only
        _same(RPF.search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk, ones),
              R.search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk))
        _same(RPF.residual_search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk, ones),
              RR.search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk))
        for fn in (RPF.search, RPF.residual_search):
            z = fn(oracle, metric, coarse, cb, lists, codes, Q, nprobe, topk, ~ones)
            assert (z[0] == 0xFFFFFFFF).all() and np.isposinf(z[1]).all()
        d = RPF.dense_search(oracle, metric, cb, codes, Q, topk, mask)
        _same(d, RPF.brute_dense_search(metric, cb, codes, Q, topk, mask))
        if topk < n:
            _same(RPF.dense_search(oracle, metric, cb, codes, Q, topk, ones), oracle.adc_search(metric, cb, codes, Q, topk))
        if nprobe == 5:  # every list probed: the dense filtered statement
            _same(a, d)
    # a subset of the queries: the others stay padding
    a = RPF.search(oracle, metric, coarse, cb, lists, codes, Q, nprobe, 4, mask, queries=[3])
    assert (a[0][[0, 1, 2, 4]] == 0xFFFFFFFF).all()


def _pq_index(n=70, m=2, k=4, sd=2):
    from vq_amd.store import PQIndex

    return PQIndex(np.zeros((m, k, sd), F), np.zeros((n, m), np.uint8))


def _ivfpq_index(n=70, residual=False):
    import vq_amd

    ix = vq_amd.IVFPQIndex(np.arange(12, dtype=F).reshape(3, 4), np.zeros((2, 4, 2), F), residual=residual)
    ix.add_codes((np.arange(n) % 3).astype(np.uint32), np.zeros((n, 2), np.uint8))
    return ix


def _no_device(monkeypatch):
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "IVFPQ", boom)
    monkeypatch.setattr(_lib, "PQEncoder", boom)


def _bad_masks(vq_amd, call, n):
    for bad in (np.ones(n, np.uint8), np.ones(n, np.int64), np.ones(n, F), np.ones(3, np.uint64), [1.5] * n):
        with pytest.raises(vq_amd.InvalidParameter, match="allowed"):  # wrong dtype
            call(bad)
    for bad in (np.ones(n + 1, bool), np.ones(n - 1, bool), np.ones(2, np.uint32), np.ones(4, np.uint32), np.ones(0, bool)):
        with pytest.raises(vq_amd.DimensionMismatch):  # wrong length
            call(bad)
    for bad in (np.ones((n, 1), bool), np.ones((1, 3), np.uint32), np.ones((2, n), bool)):
        with pytest.raises(vq_amd.InvalidParameter, match="allowed"):  # 2-D
            call(bad)


@pytest.mark.parametrize("residual", [False, True])
def test_ivfpq_mask_checks_need_no_device(monkeypatch, residual):
    import vq_amd

    _no_device(monkeypatch)
    ix = _ivfpq_index(residual=residual)
    n = len(ix)
    Q = np.zeros((2, 4), F)
    calls = [lambda a: ix.masked_search(Q, a, 5, 2),
             lambda a: ix.masked_search(Q, a, 5, 2, rerank=object())]  # the mask is checked before the reranker
    for call in calls:
        _bad_masks(vq_amd, call, n)
    with pytest.raises((vq_amd.InvalidParameter, TypeError)):
        ix.masked_search(Q, None, 5, 2)
    # a word count for a stale n after add_codes: 70 rows are 3 words, 100 rows 4
    stale_bool, stale_words = np.ones(n, bool), vq_amd.pack_row_mask(np.ones(n, bool), n)
    ix.add_codes(np.zeros(30, np.uint32), np.zeros((30, 2), np.uint8))
    assert len(ix) == n + 30 and stale_words.shape == (3,)
    for stale in (stale_bool, stale_words):
        with pytest.raises(vq_amd.DimensionMismatch):
            ix.masked_search(Q, stale, 5, 2)
    n = len(ix)
    ok = np.ones(n, bool)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.masked_search(Q, ok, n + 1, 2)
    with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
        ix.masked_search(Q, ok, 5, 4)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.masked_search(np.zeros((2, 5), F), ok, 5, 2)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.masked_search_device(0, 2, 0, 0, 0, 4, nprobe=2)
    with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
        ix.masked_search_device(0, 2, 5, 0, 0, 4, nprobe=9)
    with pytest.raises(vq_amd.InvalidParameter, match="nq"):
        ix.masked_search_device(0, -1, 5, 0, 0, 4, nprobe=2)
    with pytest.raises(vq_amd.InvalidParameter, match="dev_allowed"):
        ix.masked_search_device(0, 2, 5, 0, 0, None, nprobe=2)
    for a in (ok, vq_amd.pack_row_mask(ok, n)):  # no queries: the empty result, after the mask has been checked
        i, d = ix.masked_search(np.zeros((0, 4), F), a, 5, 2)
        assert i.shape == (0, 5) and i.dtype == np.uint32 and d.shape == (0, 5) and d.dtype == F
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.masked_search(np.zeros((0, 4), F), np.ones(n + 1, bool), 5, 2)


def test_pqindex_mask_checks_need_no_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = _pq_index()
    n = len(ix)
    Q = np.zeros((2, 4), F)
    for call in (lambda a: ix.search(Q, 5, allowed=a), lambda a: ix.search(Q, 5, rerank=object(), allowed=a)):
        _bad_masks(vq_amd, call, n)
    stale_bool, stale_words = np.ones(n, bool), vq_amd.pack_row_mask(np.ones(n, bool), n)
    ix.codes = np.zeros((100, 2), np.uint8)  # a word count for a stale n: 70 rows are 3 words, 100 rows 4
    for stale in (stale_bool, stale_words):
        with pytest.raises(vq_amd.DimensionMismatch):
            ix.search(Q, 5, allowed=stale)
    ok = np.ones(100, bool)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search(Q, 101, allowed=ok)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.search(np.zeros((2, 5), F), 5, allowed=ok)


def test_product_quantizer_mask_checks_need_no_device(monkeypatch):
    import vq_amd
    from vq_amd.pq import ProductQuantizer

    pq = ProductQuantizer.__new__(ProductQuantizer)  # the search's checks read these fields only
    pq._dim, pq._m, pq._k = 4, 2, 4
    pq._distance = vq_amd.Distance.euclidean()

    class Boom:
        def adc_search(self, *a, **k):
            raise AssertionError("the device was touched before the arguments were checked")

    pq._enc = Boom()
    n = 70
    codes = np.zeros((n, 2), np.uint8)
    Q = np.zeros((2, 4), F)
    for call in (lambda a: pq.search(codes, Q, 5, allowed=a), lambda a: pq.search(codes, Q, 5, rerank=object(), allowed=a)):
        _bad_masks(vq_amd, call, n)
    stale = vq_amd.pack_row_mask(np.ones(n, bool), n)
    with pytest.raises(vq_amd.DimensionMismatch):
        pq.search(np.zeros((100, 2), np.uint8), Q, 5, allowed=stale)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        pq.search(codes, Q, n + 1, allowed=np.ones(n, bool))


def test_signatures():
    import vq_amd
    from vq_amd import _lib
    from vq_amd.pq import ProductQuantizer
    from vq_amd.store import PQIndex

    p = inspect.signature(vq_amd.IVFPQIndex.masked_search).parameters
    assert list(p) == ["self", "queries", "allowed", "topk", "nprobe", "rerank", "candidates"]
    assert p["topk"].default == 10 and p["nprobe"].default == 8 and p["allowed"].default is inspect.Parameter.empty
    assert p["rerank"].kind is inspect.Parameter.KEYWORD_ONLY and p["candidates"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(vq_amd.IVFPQIndex.masked_search_device).parameters
    assert list(p) == ["self", "dev_queries", "nq", "topk", "dev_idx", "dev_dist", "dev_allowed", "nprobe"] and p["nprobe"].default == 8
    for cls, first in ((PQIndex, ["self", "queries", "topk"]), (ProductQuantizer, ["self", "codes", "queries", "topk"])):
        p = inspect.signature(cls.search).parameters
        assert list(p) == first + ["rerank", "candidates", "allowed"]
        assert p["allowed"].kind is inspect.Parameter.KEYWORD_ONLY and p["allowed"].default is None
    # the unfiltered calls of IVFPQIndex take no mask, and the class has no range or filtered_* methods
    for name in ("search", "search_device", "probe"):
        assert not {"allowed", "dev_allowed"} & set(inspect.signature(getattr(vq_amd.IVFPQIndex, name)).parameters)
    assert not [a for a in dir(vq_amd.IVFPQIndex) if a.startswith("filtered_") or "range" in a]
    assert "allowed" in inspect.signature(_lib.PQEncoder.adc_search).parameters
    assert hasattr(_lib.IVFPQ, "search_masked") and hasattr(_lib.IVFPQ, "search_masked_device")
    assert not [a for a in dir(_lib.IVFPQ) if "range" in a]
    for cls in (_lib.IVFFlat, _lib.IVFSQ, _lib.IVFBin):  # the split leaves the other handles what they had
        assert all(hasattr(cls, a) for a in ("search_masked", "search_masked_device", "range_search_masked", "range_search_masked_device"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


def test_cabi_ivfpq_search_masked_checks_need_no_device(lib):
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    idx, dist = np.zeros(2, np.uint32), np.zeros(2, F)
    qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
    host = L.vqhip_ivfpq_search_masked
    assert host(None, qp, 2, 1, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the handle
    fake = ctypes.c_void_p(8)  # never dereferenced: a NULL pointer is found first
    assert host(fake, qp, 2, 1, 1, None, ip, dp) == lib.ERR_NULL_PTR  # the mask
    assert host(fake, None, 2, 1, 1, wp, ip, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, 1, 1, wp, None, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, 1, 1, wp, ip, None) == lib.ERR_NULL_PTR
    assert host(fake, qp, 0, 1, 1, None, ip, dp) == lib.ERR_NULL_PTR  # with no queries too
    dev = L.vqhip_ivfpq_search_masked_device
    v = ctypes.c_void_p
    assert dev(None, v(q.ctypes.data), 2, 1, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, v(q.ctypes.data), 2, 1, 1, None, v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    assert dev(fake, None, 2, 1, 1, v(w.ctypes.data), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_NULL_PTR
    for off in (1, 2, 3):  # a mask pointer that is not 4-byte aligned, found before the handle is looked at
        assert dev(None, v(q.ctypes.data), 2, 1, 1, v(w.ctypes.data + off), v(idx.ctypes.data), v(dist.ctypes.data)) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()


@pytest.mark.parametrize("flags", [0, 1])
def test_cabi_ivfpq_masked_argument_ranges_need_no_device(lib, flags):
    """nprobe and topk are held to the unmasked calls' bounds on a real handle (create and add are host-only)"""
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    ix = lib.IVFPQ(np.zeros((3, 4), F), np.zeros((2, 4, 2), F), K.EUCLIDEAN, flags)
    try:
        ix.add((np.arange(40) % 3).astype(np.uint32), np.zeros((40, 2), np.uint8))
        q = np.zeros((2, 4), F)
        w = np.ones(2, np.uint32)
        idx, dist = np.zeros(2 * 41, np.uint32), np.zeros(2 * 41, F)
        qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
        v = ctypes.c_void_p
        for nprobe, topk, what in ((0, 1, "nprobe"), (4, 1, "nprobe"), (1, 0, "topk"), (1, 41, "topk")):
            assert L.vqhip_ivfpq_search_masked(ix.raw, qp, 2, nprobe, topk, wp, ip, dp) == lib.ERR_INVALID_INPUT
            assert what in lib.last_error()
            assert L.vqhip_ivfpq_search_masked_device(ix.raw, v(q.ctypes.data), 2, nprobe, topk, v(w.ctypes.data), v(idx.ctypes.data),
                                                      v(dist.ctypes.data)) == lib.ERR_INVALID_INPUT
            assert what in lib.last_error()
        assert L.vqhip_ivfpq_search_masked(ix.raw, qp, 0, 1, 1, wp, ip, dp) == lib.OK  # no queries: nothing to do
    finally:
        ix.close()


def test_cabi_pq_adc_masked_checks_need_no_device(lib):
    """a NULL pointer -- the mask among them -- is reported before the encoder is looked at, in all three forms"""
    L = lib.load()
    f32p, u32p, u8p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    c = np.zeros((70, 2), np.uint8)
    idx, dist = np.zeros(2, np.uint32), np.zeros(2, F)
    qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
    fake = ctypes.c_void_p(8)  # never dereferenced: a NULL pointer is found first
    for fn, codes in ((L.vqhip_pq_adc_search_masked, (c.ctypes.data_as(u8p), 70)),
                      (L.vqhip_pq_adc_search_masked_device, (ctypes.c_void_p(c.ctypes.data), 70)),
                      (L.vqhip_pq_adc_search_resident_masked, ())):
        assert fn(None, *codes, qp, 2, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the encoder
        assert fn(fake, *codes, qp, 2, 1, None, ip, dp) == lib.ERR_NULL_PTR  # the mask
        assert fn(fake, *codes, None, 2, 1, wp, ip, dp) == lib.ERR_NULL_PTR
        assert fn(fake, *codes, qp, 2, 1, wp, None, dp) == lib.ERR_NULL_PTR
        assert fn(fake, *codes, qp, 2, 1, wp, ip, None) == lib.ERR_NULL_PTR
        assert fn(fake, *codes, qp, 0, 1, None, ip, dp) == lib.ERR_NULL_PTR  # with no queries too
        if codes:
            assert fn(fake, None, 70, qp, 2, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the codes

