"""CPU checks of the inverted-file PQ index (vq_amd.IVFPQIndex, include/vqhip.h vqhip_ivfpq_*): the numpy statement
(tests/ref_ivf.py) against its brute-force restatement -- ties, NaN, padding, one- and two-byte codes --, the argument
checks of the Python class and of the C ABI, which all come before any device work, and the VQIVFPQ1 file."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_ivf as R
import ref_knn as K

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)
NAMES = ["squared_euclidean", "euclidean", "manhattan"]


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _case(rng, n, nlist, m, k, sd, nq=6, dup=True):
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    if dup:
        codes[n // 2:n // 2 + 5] = codes[:5]  # duplicate codes: equal distances, ties by row id
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    return coarse, cb, lists, codes, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", [(300, 7, 4, 16, 3), (200, 1, 2, 300, 2), (400, 16, 8, 8, 1)])
@pytest.mark.parametrize("nprobe", [1, 3, "all"])
def test_statement_equals_brute_force(orc, metric, shape, nprobe):
    n, nlist, m, k, sd = shape
    rng = np.random.default_rng(n + nlist + 10 * metric)
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd)
    p = nlist if nprobe == "all" else min(nprobe, nlist)
    for topk in (1, 10, 64):
        want = R.brute_search(metric, coarse, cb, lists, codes, Q, p, topk)
        got = R.search(orc, metric, coarse, cb, lists, codes, Q, p, topk)
        _same(got, want)


@pytest.mark.parametrize("metric", METRICS)
def test_statement_nan_queries_ties_and_padding(orc, metric):
    rng = np.random.default_rng(5 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 120, 9, 4, 16, 2, nq=4)
    lists[lists == 3] = 4  # an empty list
    Q[1, 0] = np.nan  # NaN query: every distance NaN, rows in id order
    Q[2, -1] = np.inf
    codes[:] = codes[0]  # all rows one code: ties everywhere
    for p in (1, 2, 9):
        want = R.brute_search(metric, coarse, cb, lists, codes, Q, p, 30)
        got = R.search(orc, metric, coarse, cb, lists, codes, Q, p, 30)
        _same(got, want)
        sizes = np.bincount(lists, minlength=9)
        P = R.probe(metric, coarse, Q, p)
        for j in range(Q.shape[0]):
            s = int(sizes[P[j]].sum())
            if s < 30:  # padding after every real row, NaN rows included
                assert np.all(got[0][j, s:] == R.PAD_ID)
                assert np.all(got[1][j, s:].view(np.uint32) == R.INF_BITS)
                assert np.all(got[0][j, :s] != R.PAD_ID)


def test_statement_all_lists_is_plain_adc(orc):
    rng = np.random.default_rng(3)
    coarse, cb, lists, codes, Q = _case(rng, 500, 6, 4, 32, 2)
    for metric in METRICS:
        want = orc.adc_search(metric, cb, codes, Q, 25)
        _same(R.search(orc, metric, coarse, cb, lists, codes, Q, 6, 25), want)


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, m=2, k=16, sd=3, metric="euclidean"):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFPQIndex(rng.standard_normal((nlist, m * sd)).astype(F), rng.standard_normal((m, k, sd)).astype(F),
                             vq_amd.Distance(metric))


def test_python_construction_checks():
    import vq_amd
    from vq_amd import DimensionMismatch, InvalidParameter

    rng = np.random.default_rng(1)
    cb = rng.standard_normal((2, 16, 3)).astype(F)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex(np.zeros((0, 6), F), cb)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex(np.zeros((65537, 6), F), cb)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex(np.zeros(6, F), cb)
    with pytest.raises(DimensionMismatch):
        vq_amd.IVFPQIndex(np.zeros((4, 7), F), cb)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFPQIndex(np.zeros((4, 6), F), np.zeros((2, 0, 3), F))
    with pytest.raises(InvalidParameter):  # m * k above the ADC table limit
        vq_amd.IVFPQIndex(np.zeros((4, 2 * 200), F), np.zeros((200, 256, 2), F))
    for cos in ("cosine", "cosine_unclamped"):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb, vq_amd.Distance(cos))
    ix = vq_amd.IVFPQIndex(np.zeros((4, 6), F), cb)
    assert ix.nlist == 4 and len(ix) == 0 and ix.dim == 6 and ix.m == 2 and ix.k == 16
    assert np.array_equal(ix.list_sizes(), np.zeros(4, np.uint64))


def test_python_add_codes_and_search_checks():
    from vq_amd import DimensionMismatch, InvalidParameter

    ix = _index()
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 5], np.zeros((2, 2), np.uint8))  # list id >= nlist
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, -1], np.zeros((2, 2), np.int64))
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 1], np.array([[0, 16], [1, 1]]))  # code >= k
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 1], np.zeros((2, 3), np.uint8))
    with pytest.raises(DimensionMismatch):
        ix.add_codes([0, 1, 2], np.zeros((2, 2), np.uint8))
    assert len(ix) == 0
    ids = ix.add_codes([1, 1, 4], np.array([[0, 1], [2, 3], [15, 15]]))
    assert ids.tolist() == [0, 1, 2]
    assert ix.add_codes([0], np.array([[3, 3]])).tolist() == [3]
    assert ix.list_sizes().tolist() == [1, 2, 0, 0, 1] and len(ix) == 4
    q = np.zeros((2, 6), F)
    for bad in (0, 6, 1025):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=1, nprobe=bad)
        with pytest.raises(InvalidParameter):
            ix.probe(q, nprobe=bad)
    for bad in (0, 5):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=bad, nprobe=2)
    with pytest.raises(DimensionMismatch):
        ix.search(np.zeros((2, 5), F), topk=1, nprobe=1)
    with pytest.raises(InvalidParameter):
        ix.search(q, topk=2, nprobe=1, rerank=object())
    with pytest.raises(InvalidParameter):
        ix.search(q, topk=1.5, nprobe=1)
    i, d = ix.search(np.zeros((0, 6), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2)


def test_python_save_load_round_trip(tmp_path):
    import vq_amd

    rng = np.random.default_rng(4)
    for k in (16, 300):
        ix = _index(rng, nlist=7, m=3, k=k, sd=2, metric="manhattan")
        lists = rng.integers(0, 7, 50)
        codes = rng.integers(0, k, (50, 3))
        ix.add_codes(lists, codes)
        p = tmp_path / f"ix{k}.bin"
        ix.save(p)
        back = vq_amd.IVFPQIndex.load(p)
        assert back.distance.metric == ix.distance.metric and back.nlist == 7 and len(back) == 50
        assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
        assert np.array_equal(back.codebooks, ix.codebooks)
        assert np.array_equal(back.list_ids, lists.astype(np.uint32))
        assert np.array_equal(back.codes, codes) and back.codes.dtype == (np.uint8 if k <= 256 else np.uint16)
        raw = p.read_bytes()
        assert len(raw) == 40 + 4 * (7 * 6 + 3 * k * 2 + 50) + 50 * 3 * (1 if k <= 256 else 2)


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], np.array([[1, 2], [3, 4], [5, 6]]))
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = bytearray(p.read_bytes())
    raw = mutate(raw)
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        vq_amd.IVFPQIndex.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                   # truncated header
    lambda r: b"VQPQIDX1" + r[8:],      # another magic
    _field(8, "<I", 3),                 # cosine
    _field(12, "<I", 7),                # dim not a multiple of m
    _field(16, "<I", 0),                # nlist 0
    _field(16, "<I", 70000),            # nlist too large
    _field(20, "<I", 0),                # m 0
    _field(24, "<I", 70000),            # k too large
    _field(28, "<I", 1),                # reserved
    _field(32, "<Q", 4),                # more rows than the file holds
    _field(32, "<Q", 1 << 40),          # n beyond 2^32
    lambda r: r[:-1],                   # truncated codes
    lambda r: r + b"\0",                # trailing bytes
])
def test_python_load_rejects_corrupt_files(tmp_path, mutate):
    _corrupt(tmp_path, mutate)


def test_python_load_rejects_out_of_range_ids_and_codes(tmp_path):
    base = 40 + 4 * (4 * 6 + 2 * 16 * 3)
    _corrupt(tmp_path, _field(base + 4, "<I", 4))        # list id 4 of nlist 4
    _corrupt(tmp_path, lambda r: r[:-1] + bytes([16]))   # code 16 of k 16


# ---- the C ABI: parameters checked before any device work ----------------------------------------

@pytest.fixture(scope="module")
def lib():
    from vq_amd import _lib

    return _lib


def _create(lib, nlist=4, m=2, k=16, sd=3, metric=1):
    coarse = np.zeros((max(nlist, 1), m * sd), F)
    cb = np.zeros((m, max(k, 1), sd), F)
    h = C.c_void_p()
    rc = lib.load().vqhip_ivfpq_create(coarse.ctypes.data_as(lib._f32p), nlist, cb.ctypes.data_as(lib._f32p), m, k, sd,
                                       metric, C.byref(h))
    return rc, h


def test_cabi_create_checks(lib):
    L = lib.load()
    h = C.c_void_p()
    assert L.vqhip_ivfpq_create(None, 4, None, 2, 16, 3, 1, C.byref(h)) == lib.ERR_NULL_PTR
    assert _create(lib, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, nlist=65537)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, m=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, k=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, sd=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, k=65537)[0] == lib.ERR_UNSUPPORTED
    assert _create(lib, metric=7)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, metric=lib.COSINE)[0] == lib.ERR_UNSUPPORTED
    assert _create(lib, metric=lib.COSINE_UNCLAMPED)[0] == lib.ERR_UNSUPPORTED
    rc, _ = _create(lib, m=151, k=256, sd=1)  # m * k = 38656 > 38400
    assert rc == lib.ERR_UNSUPPORTED and "38400" in lib.last_error()


def test_cabi_add_info_sizes_and_search_bounds_are_host_only(lib):
    L = lib.load()
    rc, h = _create(lib, nlist=4, m=2, k=300, sd=3)
    assert rc == lib.OK
    try:
        lid = np.array([0, 3, 3], np.uint32)
        codes = np.array([[1, 299], [0, 0], [5, 7]], np.uint16)
        assert L.vqhip_ivfpq_add(h, lid.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._vp), 3) == lib.OK
        bad = np.array([0, 4, 1], np.uint32)
        assert L.vqhip_ivfpq_add(h, bad.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._vp), 3) == lib.ERR_INVALID_INPUT
        badc = codes.copy()
        badc[2, 1] = 300
        assert L.vqhip_ivfpq_add(h, lid.ctypes.data_as(lib._u32p), badc.ctypes.data_as(lib._vp), 3) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfpq_add(h, None, None, 0) == lib.OK
        n, nlist, dim, m, k, metric = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
        assert L.vqhip_ivfpq_info(h, C.byref(n), C.byref(nlist), C.byref(dim), C.byref(m), C.byref(k), C.byref(metric)) == lib.OK
        assert (n.value, nlist.value, dim.value, m.value, k.value, metric.value) == (3, 4, 6, 2, 300, 1)
        sizes = np.zeros(4, np.uint64)
        assert L.vqhip_ivfpq_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK
        assert sizes.tolist() == [1, 0, 0, 2]
        q = np.zeros((2, 6), F)
        idx = np.zeros((2, 8), np.uint32)
        dist = np.zeros((2, 8), F)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 4)):  # nprobe in [1, nlist], topk in [1, n]
            assert L.vqhip_ivfpq_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfpq_search_device(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfpq_probe(h, qp, 2, 0, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfpq_probe(h, qp, 2, 5, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfpq_search(h, qp, 0, 2, 2, ip, dp) == lib.OK  # nq = 0
        assert L.vqhip_ivfpq_search(h, None, 2, 2, 2, ip, dp) == lib.ERR_NULL_PTR
    finally:
        L.vqhip_ivfpq_destroy(h)
