"""Hamming-radius range search without a GPU: the numpy statement (tests/ref_binary_range.py) against a literal double
loop, the clamped radius and the f32 radius the inverted-file form rests on, and every argument check of the new C ABI
calls and Python methods that is decided before any device work."""
import ctypes

import numpy as np
import pytest

import ref_binary as B
import ref_binary_range as BR
import ref_ivfbin as IB

F = np.float32
DENSE = ["vqhip_binary_range_search", "vqhip_binary_range_search_device"]
IVF = ["vqhip_ivfbin_range_search", "vqhip_ivfbin_range_search_device"]
NAMES = DENSE + IVF
U32_MAX = (1 << 32) - 1


def _h(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def _brute(qw, words, D, h, keep=None):
    """one (query, row) pair at a time: is the row kept (its list probed), is its Hamming distance within the radius"""
    lims, idx, dist = [0], [], []
    for j in range(qw.shape[0]):
        for i in range(words.shape[0]):
            if keep is not None and not keep(j, i):
                continue
            H = _h(qw[j], words[i])
            if H <= h[j]:
                idx.append(i)
                dist.append(D[H])
        lims.append(len(idx))
    return np.array(lims, np.uint64), np.array(idx, np.uint32), np.array(dist, F)


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("d", [1, 31, 33, 70])
def test_statement_matches_double_loop(metric, d):
    rng = np.random.default_rng(100 * d + metric)
    low, high = IB.LOW_HIGH[(d + metric) % len(IB.LOW_HIGH)]
    X = rng.standard_normal((37, d)).astype(F)
    Q = rng.standard_normal((5, d)).astype(F)
    X[7], X[20] = Q[1], Q[1]  # exact duplicates of query 1
    words, qw = B.pack(B.bits_f32(X, 0.25)), B.pack(B.bits_f32(Q, 0.25))
    D = B.reported(d, low, high, metric)
    h = [d // 3, 0, d, d + 1, U32_MAX]
    got = BR.search(qw, words, d, low, high, metric, h)
    assert BR.same(got, _brute(qw, words, D, h))
    assert BR.same(got, BR.search_rows(Q, X, 0.25, low, high, metric, np.array(h, np.uint64)))
    lims = got[0].astype(np.int64)
    assert lims[0] == 0 and lims[-1] == got[1].size == got[2].size
    assert {7, 20} <= set(got[1][lims[1]:lims[2]].tolist())  # radius 0: the bit matches
    assert all(int(lims[j + 1] - lims[j]) == 37 for j in (2, 3, 4))  # radius >= d: every row
    for j in range(5):
        assert (np.diff(got[1][lims[j]:lims[j + 1]].astype(np.int64)) > 0).all()  # ascending row id
    one = BR.search(qw, words, d, low, high, metric, d // 3)  # a scalar radius is every query's
    assert BR.same(one, BR.search(qw, words, d, low, high, metric, [d // 3] * 5))
    none = BR.search(np.empty((0, (d + 31) // 32), np.uint32), words, d, low, high, metric, [])
    assert none[0].tolist() == [0] and none[1].size == 0 and none[2].size == 0


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("coarse_metric", [1, 3])
def test_ivf_statement_matches_double_loop(metric, coarse_metric):
    rng = np.random.default_rng(7 + metric)
    d, n, nlist = 40, 33, 5
    bq = (0.0, 3, 200)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist - 1, n).astype(np.uint32)  # the last list stays empty
    X = (coarse[lists] + F(0.5) * rng.standard_normal((n, d)).astype(F)).astype(F)
    Q = rng.standard_normal((4, d)).astype(F)
    words, qw = B.pack(B.bits_f32(X, bq[0])), B.pack(B.bits_f32(Q, bq[0]))
    D = B.reported(d, bq[1], bq[2], metric)
    h = [12, 0, d, U32_MAX]
    for nprobe in (1, 2, nlist):
        P = IB.probe(coarse_metric, coarse, Q, nprobe)
        got = BR.ivf_search(metric, coarse_metric, coarse, lists, bq, words, d, Q, nprobe, h)
        want = _brute(qw, words, D, h, keep=lambda j, i: int(lists[i]) in [int(l) for l in P[j]])
        assert BR.same(got, want)
    full = BR.ivf_search(metric, coarse_metric, coarse, lists, bq, words, d, Q, nlist, h)
    assert BR.same(full, BR.search(qw, words, d, bq[1], bq[2], metric, h))  # nprobe == nlist is the dense statement
    empty = BR.ivf_search(metric, coarse_metric, coarse, np.empty(0, np.uint32), bq, np.empty((0, 2), np.uint32), d, Q, 2, h)
    assert empty[0].tolist() == [0] * 5 and empty[1].size == 0  # no rows


DIMS = list(range(1, 65)) + [1023, 1024, 1025, 8192]


@pytest.mark.parametrize("metric", B.METRICS)
def test_float_radius_is_exact_for_every_cut(metric):
    """what the inverted-file form rests on: with r = reported[min(h_q, d)], reported[h] <= r (the f32 comparison of the
    range stage) holds iff h <= h_q, for every H a row can have; and the dense kernels' clamp changes no answer"""
    for d in DIMS:
        for low, high in IB.LOW_HIGH:
            D = B.reported(d, low, high, metric)
            assert D.dtype == F and D.shape == (d + 1,) and not np.isnan(D).any()
            H = np.arange(d + 1)
            cuts = range(d + 3) if d <= 64 else [0, 1, 2, d // 2, d - 1, d, d + 1, 1 << 31, U32_MAX]
            for hq in list(cuts) + [1 << 31, U32_MAX]:
                c = BR.clamped(hq, d)
                assert c == min(hq, d) and 0 <= c <= d
                r = BR.float_radius(hq, d, low, high, metric)
                assert r.dtype == F and r.view(np.uint32) == D[c].view(np.uint32)
                assert np.array_equal(D <= r, H <= hq), (d, low, high, hq)
                assert np.array_equal(H <= c, H <= hq)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


def _call(fn, name, h, qp, nq, nprobe, radii, max_results, out):
    front = (nprobe,) if name in IVF else ()
    return fn(h, qp, nq, *front, radii, max_results, out)


@pytest.mark.parametrize("name", NAMES)
def test_cabi_argument_checks_need_no_device(lib, name):
    """out, the pointers and max_results are checked before the index handle is looked at (every u32 is a radius);
    the inverted-file form checks nprobe right after, with a handle that needs no device"""
    fn = getattr(lib.load(), name)
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    q = np.zeros((2, 4), F)
    qp = q.ctypes.data_as(f32p) if not name.endswith("_device") else ctypes.c_void_p(q.ctypes.data)
    radii = np.array([0, U32_MAX], np.uint32)
    gp = radii.ctypes.data_as(u32p)
    out = ctypes.c_void_p(1)
    assert _call(fn, name, None, qp, 2, 1, gp, 10, None) == lib.ERR_NULL_PTR
    assert _call(fn, name, None, None, 2, 1, gp, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert _call(fn, name, None, qp, 2, 1, None, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert _call(fn, name, None, qp, 2, 1, gp, 0, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert _call(fn, name, None, qp, 2, 1, gp, 10, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None
    if name in DENSE:
        return  # (a vqhip_binary exists on a device only)
    L = lib.load()
    coarse = np.arange(12, dtype=F)
    h = ctypes.c_void_p()
    assert L.vqhip_ivfbin_create(0.0, 0, 1, coarse.ctypes.data_as(f32p), 3, 4, 2, 1, ctypes.byref(h)) == lib.OK
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
        assert L.vqhip_ivfbin_destroy(h) == lib.OK


def _indexes():
    import vq_amd

    dense = vq_amd.BinaryIndex(np.zeros((3, 4), F))
    ivf = vq_amd.IVFBinaryIndex(np.arange(12, dtype=F).reshape(3, 4))
    ivf.add_packed([0, 2], np.zeros((2, 1), np.uint32))
    return dense, ivf


@pytest.mark.parametrize("which", [0, 1])
def test_python_argument_checks_need_no_device(lib, which):
    from vq_amd.errors import DimensionMismatch, InvalidParameter

    ix = _indexes()[which]
    Q = np.zeros((2, 4), F)
    probe = {"nprobe": 1} if which == 1 else {}  # (nlist = 3: the default of 8 is refused, as by search)
    for form in (lambda **kw: ix.hamming_range_search(Q, **kw), lambda **kw: ix.hamming_range_search_device(256, 2, **kw)):
        call = lambda form=form, **kw: form(**{**probe, **kw})
        for bad in (1.5, np.float32(0.25), [1, 2.5], np.nan, np.inf, [1, np.nan]):  # floats that are not integral
            with pytest.raises(InvalidParameter, match="radius"):
                call(radius=bad)
        for bad in (-1, [3, -2], np.array([-1, 0], np.int64), -1.0):  # negatives
            with pytest.raises(InvalidParameter, match="radius"):
                call(radius=bad)
        for bad in (1 << 32, [0, 1 << 32], float(1 << 32), 1 << 70):  # values >= 2^32
            with pytest.raises(InvalidParameter, match="radius"):
                call(radius=bad)
        for bad in ([1, 2, 3], [1], [], np.zeros((2, 1), np.uint32), "x", None, [1, "y"]):  # the wrong length or kind
            with pytest.raises(InvalidParameter, match="radius"):
                call(radius=bad)
        for m in (0, -1, 1 << 64, 2.5):
            with pytest.raises(InvalidParameter, match="max_results"):
                call(radius=1, max_results=m)
        if which == 1:
            for nprobe in (0, 4, 1025, 1.5):
                with pytest.raises(InvalidParameter, match="nprobe"):
                    call(radius=1, nprobe=nprobe)
    with pytest.raises(DimensionMismatch):
        ix.hamming_range_search(np.zeros((2, 5), F), 1)
    with pytest.raises(InvalidParameter, match="nq"):
        ix.hamming_range_search_device(256, -1, 1)
    with pytest.raises(InvalidParameter, match="nq"):
        ix.hamming_range_search_device(256, 1 << 32, 1)
    from vq_amd._resident_common import _hamming_radii

    for good, want in ((0, [0, 0]), (U32_MAX, [U32_MAX] * 2), (np.float64(7.0), [7, 7]), ([1, 2.0], [1, 2]),
                       (np.array([5, U32_MAX], np.uint64), [5, U32_MAX]), (np.uint8(9), [9, 9])):
        r = _hamming_radii(good, 2)
        assert r.dtype == np.uint32 and r.flags.c_contiguous and r.tolist() == want
    lims, idx, dist = ix.hamming_range_search(np.empty((0, 4), F), np.empty(0, np.uint32), **probe)  # no queries: no device either
    assert lims.tolist() == [0] and lims.dtype == np.uint64 and idx.dtype == np.uint32 and dist.dtype == F
    assert idx.size == 0 and dist.size == 0
    assert ix._ix is None  # none of this created the device handle


def test_methods_present_and_range_search_absent():
    import vq_amd
    from vq_amd import _lib

    for cls in (vq_amd.BinaryIndex, vq_amd.IVFBinaryIndex, _lib.Binary, _lib.IVFBin):
        assert callable(cls.hamming_range_search) and callable(cls.hamming_range_search_device)
        assert not hasattr(cls, "range_search") and not hasattr(cls, "range_search_device")
    assert all(n in _lib.SIGNATURES for n in NAMES)
    assert _lib.BINARY_RANGE_BLOCK == 8192
    import inspect

    from vq_amd._resident_common import DEFAULT_MAX_RESULTS

    assert inspect.signature(vq_amd.IVFBinaryIndex.hamming_range_search).parameters["nprobe"].default == 8
    for cls in (vq_amd.BinaryIndex, vq_amd.IVFBinaryIndex):
        for name in ("hamming_range_search", "hamming_range_search_device"):
            assert inspect.signature(getattr(cls, name)).parameters["max_results"].default == DEFAULT_MAX_RESULTS
