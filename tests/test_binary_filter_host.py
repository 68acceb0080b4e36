"""Filtered search of the two binary indexes without a GPU: the numpy statement (tests/ref_binary_filter.py) against a
plain loop, the eight Python methods and their signatures, the argument errors they raise before a device is touched,
the C entry points' pointer checks, and the slice rule of the masked scan."""
import ctypes
import inspect

import numpy as np
import pytest

import ref_binary as B
import ref_binary_filter as S
import ref_ivf as I

F = np.float32
METHODS = ("filtered_search", "filtered_search_device", "filtered_hamming_range_search", "filtered_hamming_range_search_device")


def _pop(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


@pytest.mark.parametrize("metric", B.METRICS)
def test_statement_matches_a_plain_loop(metric):
    rng = np.random.default_rng(metric)
    n, d, nq, topk, nlist, nprobe = 90, 45, 4, 7, 5, 2
    X = rng.standard_normal((n, d)).astype(F)
    X[40:43] = X[3:6]  # duplicates on both sides of the mask
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = X[4]
    words, qw = B.pack(B.bits_f32(X, 0.25)), B.pack(B.bits_f32(Q, 0.25))
    D = B.reported(d, 3, 200, metric)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    P = I.probe(1, coarse, Q, nprobe)
    for mask in (rng.random(n) < 0.5, rng.random(n) < 0.05, np.zeros(n, bool), np.ones(n, bool)):
        mask = mask.copy()
        if mask.any() and not mask.all():
            mask[3], mask[40], mask[4], mask[41] = True, True, False, True
        for ivf in (False, True):
            want_i = np.full((nq, topk), 0xFFFFFFFF, np.uint32)
            want_d = np.full((nq, topk), np.inf, F)
            hits = []
            for j in range(nq):
                rows = [i for i in range(n) if mask[i] and (not ivf or lists[i] in P[j])]
                pairs = sorted((_pop(qw[j], words[i]), i) for i in rows)
                for s, (h, i) in enumerate(pairs[:topk]):
                    want_i[j, s], want_d[j, s] = i, D[h]
                hits.append([(i, D[h]) for h, i in sorted(pairs, key=lambda p: p[1]) if h <= 20])
            if ivf:
                got = S.ivf_search(metric, 1, coarse, lists, (0.25, 3, 200), words, d, Q, nprobe, topk, mask)
                rng_got = S.ivf_range_search(metric, 1, coarse, lists, (0.25, 3, 200), words, d, Q, nprobe, 20, mask)
            else:
                got = S.search(qw, words, d, 3, 200, metric, topk, mask)
                rng_got = S.range_search(qw, words, d, 3, 200, metric, 20, mask)
            assert np.array_equal(got[0], want_i)
            assert np.array_equal(got[1].view(np.uint32), want_d.view(np.uint32))
            assert rng_got[0].tolist() == np.cumsum([0] + [len(h) for h in hits]).tolist()
            assert rng_got[1].tolist() == [i for h in hits for i, _ in h]
            assert np.array_equal(rng_got[2].view(np.uint32), np.array([v for h in hits for _, v in h], F).view(np.uint32))


def test_the_eight_methods_and_their_signatures():
    import vq_amd
    from vq_amd._binary_filter import BinaryFilterMixin
    from vq_amd._resident_common import DEFAULT_MAX_RESULTS

    def sig(cls, name):
        return [(p.name, p.kind, p.default) for p in inspect.signature(getattr(cls, name)).parameters.values()][1:]

    PK, KW, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    b, v = vq_amd.BinaryIndex, vq_amd.IVFBinaryIndex
    assert issubclass(b, BinaryFilterMixin) and issubclass(v, BinaryFilterMixin)  # one mixin under both
    assert sig(b, "filtered_search") == [("queries", PK, E), ("allowed", PK, E), ("topk", PK, 10), ("rerank", KW, None),
                                         ("candidates", KW, None)]
    assert sig(b, "filtered_search_device") == [(n, PK, E) for n in ("dev_queries", "nq", "topk", "dev_idx", "dev_dist", "dev_allowed")]
    assert sig(b, "filtered_hamming_range_search") == [("queries", PK, E), ("radius", PK, E), ("allowed", PK, E),
                                                       ("max_results", PK, DEFAULT_MAX_RESULTS)]
    assert sig(b, "filtered_hamming_range_search_device") == [("dev_queries", PK, E), ("nq", PK, E), ("radius", PK, E),
                                                              ("dev_allowed", PK, E), ("max_results", PK, DEFAULT_MAX_RESULTS)]
    # the inverted file: the same four with nprobe = 8 where the unfiltered method has it
    assert sig(v, "filtered_search") == [("queries", PK, E), ("allowed", PK, E), ("topk", PK, 10), ("nprobe", PK, 8),
                                         ("rerank", KW, None), ("candidates", KW, None)]
    assert sig(v, "filtered_search_device") == [(n, PK, E) for n in ("dev_queries", "nq", "topk", "dev_idx", "dev_dist",
                                                                   "dev_allowed")] + [("nprobe", PK, 8)]
    assert sig(v, "filtered_hamming_range_search") == [("queries", PK, E), ("radius", PK, E), ("allowed", PK, E), ("nprobe", PK, 8),
                                                       ("max_results", PK, DEFAULT_MAX_RESULTS)]
    assert sig(v, "filtered_hamming_range_search_device") == [("dev_queries", PK, E), ("nq", PK, E), ("radius", PK, E),
                                                              ("dev_allowed", PK, E), ("nprobe", PK, 8),
                                                              ("max_results", PK, DEFAULT_MAX_RESULTS)]
    assert not any(hasattr(vq_amd.IVFPQIndex, m) for m in METHODS)  # IVFPQIndex stays as it is


def _no_device(monkeypatch):
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "Binary", boom)
    monkeypatch.setattr(_lib, "IVFBin", boom)


@pytest.mark.parametrize("which", ["binary", "ivfbin"])
def test_python_mask_checks_need_no_device(monkeypatch, which):
    import vq_amd

    _no_device(monkeypatch)
    rng = np.random.default_rng(5)
    n, d = 70, 40
    X = rng.standard_normal((n, d)).astype(F)
    if which == "binary":
        ix, extra = vq_amd.BinaryIndex(X), {}
    else:
        ix, extra = vq_amd.IVFBinaryIndex(np.zeros((3, d), F)), {"nprobe": 2}
        ix.add_packed(np.arange(n) % 3, B.pack(B.bits_f32(X, 0.0)))
    Q = X[:2]
    ok = np.ones(n, bool)
    calls = [lambda a: ix.filtered_search(Q, a, 5, **extra), lambda a: ix.filtered_hamming_range_search(Q, 3, a, **extra)]
    for call in calls:
        with pytest.raises(vq_amd.InvalidParameter, match="allowed"):
            call(np.ones(n, np.int8))  # wrong dtype
        with pytest.raises(vq_amd.InvalidParameter, match="allowed"):
            call(np.ones(n, np.float32))
        with pytest.raises(vq_amd.DimensionMismatch):
            call(np.ones(n + 1, bool))  # wrong length, bool form
        with pytest.raises(vq_amd.DimensionMismatch):
            call(np.ones(n - 1, bool))
        with pytest.raises(vq_amd.DimensionMismatch):
            call(np.ones((n + 31) // 32 + 1, np.uint32))  # wrong length, word form
        with pytest.raises(vq_amd.DimensionMismatch):
            call(np.ones((n + 31) // 32 - 1, np.uint32))
        with pytest.raises(vq_amd.InvalidParameter, match="1D"):
            call(np.ones((n, 1), bool))  # 2-D mask
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.filtered_search(Q, ok, 0, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.filtered_search(Q, ok, n + 1, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="candidates"):
        ix.filtered_search(Q, ok, 5, candidates=8, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="rerank"):
        ix.filtered_search(Q, ok, 5, rerank=ix, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="radius"):
        ix.filtered_hamming_range_search(Q, -1, ok, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="max_results"):
        ix.filtered_hamming_range_search(Q, 1, ok, max_results=0, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.filtered_search_device(0, 2, 0, 0, 0, 4, **extra)
    with pytest.raises(vq_amd.InvalidParameter, match="radius"):
        ix.filtered_hamming_range_search_device(0, 2, 1.5, 4, **extra)
    if which == "ivfbin":
        with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
            ix.filtered_search(Q, ok, 5, nprobe=4)
        with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
            ix.filtered_hamming_range_search(Q, 1, ok, nprobe=0)
        with pytest.raises(vq_amd.InvalidParameter, match="nprobe"):
            ix.filtered_search_device(0, 2, 5, 0, 0, 4, nprobe=9)
    # no queries: the empty results, after the mask has been checked
    for a in (ok, vq_amd.pack_row_mask(ok, n)):
        i, dd = ix.filtered_search(np.zeros((0, d), F), a, 5, **extra)
        assert i.shape == (0, 5) and i.dtype == np.uint32 and dd.shape == (0, 5) and dd.dtype == F
        lims, idx, dist = ix.filtered_hamming_range_search(np.zeros((0, d), F), 1, a, **extra)
        assert lims.tolist() == [0] and idx.size == 0 and dist.size == 0
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.filtered_search(np.zeros((0, d), F), np.ones(n + 1, bool), 5, **extra)


def test_mask_length_follows_an_add(monkeypatch):
    """a mask sized for n before an add grew the index is refused, in both forms"""
    import vq_amd

    _no_device(monkeypatch)
    d = 33
    ix = vq_amd.IVFBinaryIndex(np.zeros((2, d), F))
    ix.add_packed(np.zeros(40, np.uint32), np.zeros((40, 2), np.uint32))
    old_b, old_w = np.ones(40, bool), vq_amd.pack_row_mask(np.ones(40, bool), 40)
    ix.add_packed(np.ones(30, np.uint32), np.zeros((30, 2), np.uint32))
    Q = np.zeros((1, d), F)
    for a in (old_b, old_w):
        with pytest.raises(vq_amd.DimensionMismatch):
            ix.filtered_search(Q, a, 5, 1)
        with pytest.raises(vq_amd.DimensionMismatch):
            ix.filtered_hamming_range_search(Q, 1, a, 1)
    i, _ = ix.filtered_search(np.zeros((0, d), F), np.ones(70, bool), 5, 1)  # the new length passes
    assert i.shape == (0, 5)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from vq_amd import _lib

    return _lib


@pytest.mark.parametrize("prefix,front", [("vqhip_binary", ()), ("vqhip_ivfbin", (1,))])
def test_cabi_search_masked_checks_need_no_device(lib, prefix, front):
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    idx, dist = np.zeros(2, np.uint32), np.zeros(2, F)
    qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
    host = getattr(L, prefix + "_search_masked")
    fake = ctypes.c_void_p(8)  # never dereferenced: a NULL pointer is found first
    assert host(None, qp, 2, *front, 1, wp, ip, dp) == lib.ERR_NULL_PTR  # the handle
    assert host(fake, qp, 2, *front, 1, None, ip, dp) == lib.ERR_NULL_PTR  # the mask
    assert host(fake, None, 2, *front, 1, wp, ip, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, *front, 1, wp, None, dp) == lib.ERR_NULL_PTR
    assert host(fake, qp, 2, *front, 1, wp, ip, None) == lib.ERR_NULL_PTR
    assert host(fake, qp, 0, *front, 1, None, ip, dp) == lib.ERR_NULL_PTR  # with no queries too
    dev = getattr(L, prefix + "_search_masked_device")
    v = ctypes.c_void_p
    a = (v(idx.ctypes.data), v(dist.ctypes.data))
    assert dev(None, v(q.ctypes.data), 2, *front, 1, v(w.ctypes.data), *a) == lib.ERR_NULL_PTR
    assert dev(fake, v(q.ctypes.data), 2, *front, 1, None, *a) == lib.ERR_NULL_PTR
    assert dev(fake, None, 2, *front, 1, v(w.ctypes.data), *a) == lib.ERR_NULL_PTR
    for off in (1, 2, 3):  # a device mask at an odd address, with a NULL handle behind it
        assert dev(None, v(q.ctypes.data), 2, *front, 1, v(w.ctypes.data + off), *a) == lib.ERR_INVALID_INPUT
        assert "row mask is not 4-byte aligned" in lib.last_error()


@pytest.mark.parametrize("name,front", [("vqhip_binary_range_search_masked", ()), ("vqhip_binary_range_search_masked_device", ()),
                                        ("vqhip_ivfbin_range_search_masked", (1,)),
                                        ("vqhip_ivfbin_range_search_masked_device", (1,))])
def test_cabi_range_masked_checks_need_no_device(lib, name, front):
    """out, the pointers, max_results and the mask are checked before the index handle is looked at"""
    fn = getattr(lib.load(), name)
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    device = name.endswith("_device")
    q = np.zeros((2, 4), F)
    w = np.ones(4, np.uint32)
    qp = ctypes.c_void_p(q.ctypes.data) if device else q.ctypes.data_as(f32p)
    wp = ctypes.c_void_p(w.ctypes.data) if device else w.ctypes.data_as(u32p)
    good = np.array([1, 0xFFFFFFFF], np.uint32).ctypes.data_as(u32p)
    out = ctypes.c_void_p(1)
    assert fn(None, qp, 2, *front, good, 10, wp, None) == lib.ERR_NULL_PTR
    assert fn(None, None, 2, *front, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert out.value is None  # *out is cleared first
    assert fn(None, qp, 2, *front, None, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR
    assert fn(None, qp, 2, *front, good, 0, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
    assert "max_results" in lib.last_error()
    assert fn(ctypes.c_void_p(8), qp, 2, *front, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the mask, before the handle
    assert fn(ctypes.c_void_p(8), qp, 0, *front, good, 10, None, ctypes.byref(out)) == lib.ERR_NULL_PTR  # with no queries too
    if device:
        for off in (1, 2, 3):
            assert fn(None, qp, 2, *front, good, 10, ctypes.c_void_p(w.ctypes.data + off), ctypes.byref(out)) == lib.ERR_INVALID_INPUT
            assert "row mask is not 4-byte aligned" in lib.last_error()
    assert fn(None, qp, 2, *front, good, 10, wp, ctypes.byref(out)) == lib.ERR_NULL_PTR  # the handle, last
    assert out.value is None


def test_cabi_masked_argument_ranges_need_no_device(lib):
    """nprobe and topk keep the unmasked calls' bounds on a real inverted file (create and add are host-only)"""
    L = lib.load()
    f32p, u32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    ix = lib.IVFBin(np.zeros((3, 40), F), 0.0, 0, 1, B.MAN, 1)
    try:
        ix.add_packed((np.arange(40) % 3).astype(np.uint32), np.zeros((40, 2), np.uint32))
        q = np.zeros((2, 40), F)
        w = np.ones(2, np.uint32)
        idx, dist = np.zeros(2 * 41, np.uint32), np.zeros(2 * 41, F)
        qp, wp, ip, dp = q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
        for nprobe, topk, what in ((0, 1, "nprobe"), (4, 1, "nprobe"), (1, 0, "topk"), (1, 41, "topk")):
            assert L.vqhip_ivfbin_search_masked(ix.raw, qp, 2, nprobe, topk, wp, ip, dp) == lib.ERR_INVALID_INPUT
            assert what in lib.last_error()
        out = ctypes.c_void_p(1)
        r = np.ones(2, np.uint32).ctypes.data_as(u32p)
        for nprobe in (0, 4):
            assert L.vqhip_ivfbin_range_search_masked(ix.raw, qp, 2, nprobe, r, 10, wp, ctypes.byref(out)) == lib.ERR_INVALID_INPUT
            assert "nprobe" in lib.last_error() and out.value is None
    finally:
        ix.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 65472, 65473, 65535, 65536, (1 << 20) + 1, (1 << 32) - 1])
@pytest.mark.parametrize("groups", [1, 2, 32, 128])
def test_masked_slices_are_whole_mask_word_pairs(lib, n, groups):
    """every slice of the masked scan is a multiple of 64 rows (a wave's rows are two whole mask words), at most 65472 (no
    16-bit histogram half carries), and the slices cover n within the grid's x extent"""
    slice_ = lib.binary_masked_slice(n, groups)
    assert slice_ % 64 == 0 and 64 <= slice_ <= 65472
    slices = -(-n // slice_)
    assert slices * slice_ >= n and (slices - 1) * slice_ < n and slices < 1 << 31
