"""CPU checks of the exact k-NN search (vq_amd.FlatIndex, include/vqhip.h vqhip_flat_*): the numpy statement of
D(q, i) (tests/ref_knn.py) against the oracle's Distance::compute pair by pair -- NaN, +-inf, zero rows, ties -- and
FlatIndex's argument checks, which all raise before any device is touched."""
import numpy as np
import pytest

import ref_knn as K

F = np.float32


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _pairs(d, rng):
    X = (rng.standard_normal((60, d)) * 2).astype(F)
    X = np.concatenate([X, K.special_rows(d, rng), X[:3]])  # exact duplicates: equal distances
    Q = np.concatenate([(rng.standard_normal((3, d))).astype(F), K.special_rows(d, rng)[[0, 5, 6]]])
    return Q, X


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", [1, 3, 8, 33])
def test_statement_equals_oracle_distance(orc, metric, d):
    rng = np.random.default_rng(100 + d)
    Q, X = _pairs(d, rng)
    for q in Q:
        got = K.distances(metric, q, X)
        want = np.array([orc.distance(metric, q, x) for x in X], F)
        nan_g, nan_w = np.isnan(got), np.isnan(want)
        assert np.array_equal(nan_g, nan_w)
        assert np.array_equal(got[~nan_g].view(np.uint32), want[~nan_w].view(np.uint32))


def test_statement_f16_rows_widen_exactly(orc):
    rng = np.random.default_rng(7)
    X16 = (rng.standard_normal((50, 12))).astype(np.float16)
    q = rng.standard_normal(12).astype(F)
    for metric in K.METRICS:
        got = K.distances(metric, q, X16.astype(F))
        want = np.array([orc.distance(metric, q, x.astype(F)) for x in X16], F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_key_order_and_ties():
    d = np.array([np.nan, 1.0, -0.0, 0.0, np.inf, 1.0, -np.inf, np.nan], F)
    idx, dist = K.topk_of(d, np.arange(d.size), d.size)
    assert idx.tolist() == [6, 2, 3, 1, 5, 4, 0, 7]  # -inf, -0, +0, ties by row, inf, NaN last by row
    assert dist.view(np.uint32)[-1] == K.NAN_BITS and dist.view(np.uint32)[1] == np.float32(-0.0).view(np.uint32)


def test_euclidean_orders_by_reported_root():
    """squared sums 4 + ulp (row 0) and 4 (row 1) both have the root 2.0: a tie under Euclidean, won by the lower
    row -- while squared Euclidean puts row 1 first"""
    X = np.array([[2.0, 2.0 ** -10.5], [2.0, 0.0]], F)
    q = np.zeros(2, F)
    sq = K.distances(K.SQUARED_EUCLIDEAN, q, X)
    assert sq[0] == np.nextafter(F(4), F(5)) and sq[1] == F(4)
    assert K.search(K.EUCLIDEAN, q, X, 2)[0][0].tolist() == [0, 1]
    assert K.search(K.SQUARED_EUCLIDEAN, q, X, 2)[0][0].tolist() == [1, 0]


# ---- FlatIndex argument checks: no device needed (the rows go to the device on the first search) ----------------
def test_flatindex_constructs_without_a_device():
    import vq_amd

    ix = vq_amd.FlatIndex(np.zeros((5, 3), F))
    assert len(ix) == 5 and ix.dim == 3 and ix.distance == vq_amd.Distance.euclidean()
    ix16 = vq_amd.FlatIndex(np.zeros((2, 7), np.float16), vq_amd.Distance.cosine())
    assert ix16.dtype == np.float16 and "float16" in repr(ix16)


@pytest.mark.parametrize("rows, exc", [
    (np.zeros((0, 4), F), "EmptyInput"),
    (np.zeros((4, 0), F), "InvalidParameter"),
    (np.zeros((4, 3), np.float64), "InvalidParameter"),
    (np.zeros((4, 3), np.int32), "InvalidParameter"),
    (np.zeros(4, F), ValueError),
])
def test_flatindex_rejects_bad_rows(rows, exc):
    import vq_amd

    e = getattr(vq_amd, exc) if isinstance(exc, str) else exc
    with pytest.raises(e):
        vq_amd.FlatIndex(rows)


def test_flatindex_rejects_bad_distance():
    import vq_amd

    with pytest.raises(vq_amd.InvalidParameter):
        vq_amd.FlatIndex(np.zeros((4, 3), F), "euclidean")


def _no_device(monkeypatch):
    """any attempt to reach the library fails the test"""
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "Flat", boom)


def test_search_checks_before_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = vq_amd.FlatIndex(np.zeros((20, 4), F))
    with pytest.raises(vq_amd.DimensionMismatch, match="expected 4, found 5"):
        ix.search(np.zeros((2, 5), F), 3)
    for k in (0, 21, -1):
        with pytest.raises(vq_amd.InvalidParameter, match="topk"):
            ix.search(np.zeros((2, 4), F), k)
    big = vq_amd.FlatIndex(np.zeros((2000, 4), F))
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        big.search(np.zeros((1, 4), F), 1025)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search(np.zeros((1, 4), F), 2.5)
    i, d = ix.search(np.zeros((0, 4), F), 3)
    assert i.shape == (0, 3) and d.shape == (0, 3)


def test_rerank_checks_before_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = vq_amd.FlatIndex(np.zeros((20, 4), F))
    q = np.zeros((2, 4), F)
    with pytest.raises(vq_amd.InvalidParameter, match="outside"):
        ix.rerank(q, np.array([[0, 1, 20], [2, 3, 4]]), 2)
    with pytest.raises(vq_amd.InvalidParameter, match="outside"):
        ix.rerank(q, np.array([[0, 1, -1], [2, 3, 4]]), 2)
    with pytest.raises(vq_amd.InvalidParameter, match="distinct"):
        ix.rerank(q, np.array([[0, 1, 1], [2, 3, 4]]), 2)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.rerank(q, np.array([[0, 1, 2], [2, 3, 4]]), 4)
    with pytest.raises(vq_amd.InvalidParameter, match="candidates"):
        ix.rerank(q, np.zeros((2, 0), np.int64), 1)
    with pytest.raises(vq_amd.InvalidParameter, match="candidates"):
        vq_amd.FlatIndex(np.zeros((5000, 4), F)).rerank(q, np.tile(np.arange(4097), (2, 1)), 1)
    with pytest.raises(vq_amd.InvalidParameter, match="integers"):
        ix.rerank(q, np.zeros((2, 3), F), 1)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.rerank(q, np.array([[0, 1, 2]]), 1)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.rerank(np.zeros((2, 3), F), np.array([[0, 1, 2], [2, 3, 4]]), 1)


def test_pq_search_rerank_checks(monkeypatch):
    """the rerank keyword checks its FlatIndex and candidate count before any search runs"""
    import vq_amd
    from vq_amd.flat import adc_then_rerank

    def adc(q, c):
        raise AssertionError("ADC ran before the arguments were checked")

    q = np.zeros((1, 4), F)
    with pytest.raises(vq_amd.InvalidParameter, match="rerank"):
        adc_then_rerank(adc, 20, 4, q, 2, object(), None)
    with pytest.raises(vq_amd.DimensionMismatch):
        adc_then_rerank(adc, 21, 4, q, 2, vq_amd.FlatIndex(np.zeros((20, 4), F)), None)
    with pytest.raises(vq_amd.DimensionMismatch):
        adc_then_rerank(adc, 20, 8, q, 2, vq_amd.FlatIndex(np.zeros((20, 4), F)), None)
    with pytest.raises(vq_amd.InvalidParameter, match="candidates"):
        adc_then_rerank(adc, 20, 4, q, 5, vq_amd.FlatIndex(np.zeros((20, 4), F)), 3)


def test_cabi_flat_checks_without_device():
    """vqhip_flat_create rejects bad parameters before it looks for a device"""
    import ctypes as C

    from vq_amd import _lib

    lib = _lib.load()
    rows = np.zeros((4, 3), F)
    h = C.c_void_p()
    p = rows.ctypes.data_as(C.c_void_p)
    for args in [(p, 0, 3, 0, 1), (p, 4, 0, 0, 1), (p, 4, 3, 2, 1), (p, 4, 3, 0, 7), (p, 1 << 32, 3, 0, 1)]:
        assert lib.vqhip_flat_create(*args, C.byref(h)) == _lib.ERR_INVALID_INPUT, args
        assert not h.value
    assert lib.vqhip_flat_create(None, 4, 3, 0, 1, C.byref(h)) == _lib.ERR_NULL_PTR
    assert lib.vqhip_flat_search(None, None, 1, 1, None, None) == _lib.ERR_NULL_PTR
