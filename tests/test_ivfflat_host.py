"""CPU checks of the inverted-file flat index (vq_amd.IVFFlatIndex, include/vqhip.h vqhip_ivfflat_*): the numpy statement
(tests/ref_ivfflat.py) against the exact k-NN statement at nprobe == nlist and against ref_ivf's probe, the argument
checks of the Python class and of the C ABI, which all come before any device work, the host-only ABI calls, and the
VQIVFFL1 file."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_ivf as I
import ref_ivfflat as R
import ref_knn as K

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]


def _case(rng, n, nlist, dim, nq=6, dtype=np.float32):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = rng.standard_normal((n, dim)).astype(dtype)
    rows[n // 2:n // 2 + 5] = rows[:5]  # duplicate rows: equal distances, ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    return coarse, lists, rows, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_all_lists_is_exact_knn(metric, dtype):
    rng = np.random.default_rng(3 + metric)
    coarse, lists, rows, Q = _case(rng, 400, 9, 7, dtype=dtype)
    rows[10] = 0  # a zero-norm row
    Q[1, 0] = np.nan
    Q[2] = 0
    for topk in (1, 25, 400):
        _same(R.search(metric, coarse, lists, rows, Q, 9, topk), K.search(metric, Q, rows.astype(F), topk))


@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_probe_and_padding(metric):
    rng = np.random.default_rng(5 + metric)
    coarse, lists, rows, Q = _case(rng, 120, 9, 4, nq=4)
    lists[lists == 3] = 4  # an empty list
    for p in (1, 2, 9):
        P = R.probe(metric, coarse, Q, p)
        assert np.array_equal(P, I.probe(metric, coarse, Q, p))
        got = R.search(metric, coarse, lists, rows, Q, p, 30)
        sizes = np.bincount(lists, minlength=9)
        for j in range(Q.shape[0]):
            s = min(int(sizes[P[j]].sum()), 30)
            assert np.all(got[0][j, s:] == R.PAD_ID) and np.all(got[1][j, s:].view(np.uint32) == I.INF_BITS)
            assert np.all(np.isin(lists[got[0][j, :s]], P[j]))  # every hit lies in a probed list


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, dim=6, metric="euclidean", dtype=np.float32):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFFlatIndex(rng.standard_normal((nlist, dim)).astype(F), vq_amd.Distance(metric), dtype)


def test_python_construction_checks():
    import vq_amd
    from vq_amd import InvalidParameter

    for bad in (np.zeros((0, 6), F), np.zeros((65537, 6), F), np.zeros(6, F), np.zeros((4, 0), F)):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFFlatIndex(bad)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFFlatIndex(np.zeros((4, 6), F), "euclidean")
    for bad in (np.float64, np.int32, "nonsense"):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFFlatIndex(np.zeros((4, 6), F), dtype=bad)
    for name in NAMES:  # the cosines included
        ix = vq_amd.IVFFlatIndex(np.zeros((4, 6), F), vq_amd.Distance(name), np.float16)
        assert ix.nlist == 4 and len(ix) == 0 and ix.dim == 6 and ix.dtype == np.float16 and ix.distance.name() == name
        assert np.array_equal(ix.list_sizes(), np.zeros(4, np.uint64)) and ix.rows.shape == (0, 6)


def test_python_add_rows_and_search_checks():
    from vq_amd import DimensionMismatch, InvalidParameter

    ix = _index()
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 5], np.zeros((2, 6), F))  # list id >= nlist
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, -1], np.zeros((2, 6), F))
    with pytest.raises(InvalidParameter):
        ix.add_rows([0.5, 1.0], np.zeros((2, 6), F))
    with pytest.raises(InvalidParameter):
        ix.add_rows([[0, 1]], np.zeros((2, 6), F))
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 1], np.zeros(12, F))
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 1], np.zeros((2, 6), np.int32))
    with pytest.raises(DimensionMismatch):
        ix.add_rows([0, 1], np.zeros((2, 5), F))
    with pytest.raises(DimensionMismatch):
        ix.add_rows([0, 1, 2], np.zeros((2, 6), F))
    with pytest.raises(DimensionMismatch):
        ix.add(np.zeros((2, 5), F))
    assert len(ix) == 0
    assert ix.add_rows([1, 1, 4], np.ones((3, 6))).tolist() == [0, 1, 2]
    assert ix.add_rows([0], np.zeros((1, 6), np.float16)).tolist() == [3]
    assert ix.list_sizes().tolist() == [1, 2, 0, 0, 1] and len(ix) == 4 and ix.rows.dtype == np.float32
    q = np.zeros((2, 6), F)
    for bad in (0, 6, 1025):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=1, nprobe=bad)
        with pytest.raises(InvalidParameter):
            ix.probe(q, nprobe=bad)
        with pytest.raises(InvalidParameter):
            ix.search_device(0, 2, 1, 0, 0, nprobe=bad)
    for bad in (0, 5):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=bad, nprobe=2)
        with pytest.raises(InvalidParameter):
            ix.search_device(0, 2, bad, 0, 0, nprobe=2)
    with pytest.raises(InvalidParameter):
        ix.search_device(0, -1, 1, 0, 0, nprobe=2)
    with pytest.raises(DimensionMismatch):
        ix.search(np.zeros((2, 5), F), topk=1, nprobe=1)
    with pytest.raises(DimensionMismatch):
        ix.probe(np.zeros((2, 5), F), nprobe=1)
    with pytest.raises(InvalidParameter):
        ix.search(q, topk=1.5, nprobe=1)
    i, d = ix.search(np.zeros((0, 6), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2) and ix.probe(np.zeros((0, 6), F), 3).shape == (0, 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_python_save_load_round_trip(tmp_path, dtype):
    import vq_amd

    rng = np.random.default_rng(4)
    ix = _index(rng, nlist=7, dim=6, metric="cosine", dtype=dtype)
    lists = rng.integers(0, 7, 50)
    rows = rng.standard_normal((50, 6)).astype(dtype)
    ix.add_rows(lists[:20], rows[:20])
    ix.add_rows(lists[20:], rows[20:])
    p = tmp_path / "ix.bin"
    ix.save(p)
    back = vq_amd.IVFFlatIndex.load(p)
    assert back.distance.metric == ix.distance.metric and back.nlist == 7 and len(back) == 50 and back.dtype == dtype
    assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
    assert np.array_equal(back.list_ids, lists.astype(np.uint32))
    assert back.rows.dtype == dtype and np.array_equal(back.rows.view(np.uint8), rows.view(np.uint8))
    assert len(p.read_bytes()) == 32 + 4 * (7 * 6 + 50) + 50 * 6 * np.dtype(dtype).itemsize


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_rows([0, 3, 2], np.arange(18, dtype=F).reshape(3, 6))
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = mutate(bytearray(p.read_bytes()))
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        vq_amd.IVFFlatIndex.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


BASE = 32 + 4 * 4 * 6  # the header and the centroids of _corrupt's file


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                    # truncated header
    lambda r: b"VQIVFPQ1" + r[8:],       # another magic
    _field(8, "<I", 5),                  # metric out of range
    _field(12, "<I", 0),                 # dim 0
    _field(16, "<I", 0),                 # nlist 0
    _field(16, "<I", 70000),             # nlist too large
    _field(20, "<I", 2),                 # dtype out of range
    _field(24, "<Q", 4),                 # more rows than the file holds
    _field(24, "<Q", 1 << 40),           # n beyond 2^32
    lambda r: r[:BASE - 4],              # truncated centroids
    lambda r: r[:BASE + 8],              # truncated list ids
    lambda r: r[:-1],                    # truncated rows
    lambda r: r + b"\0",                 # trailing bytes
    _field(BASE + 4, "<I", 4),           # list id 4 of nlist 4
])
def test_python_load_rejects_corrupt_files(tmp_path, mutate):
    _corrupt(tmp_path, mutate)


# ---- the C ABI: parameters checked before any device work ----------------------------------------

@pytest.fixture(scope="module")
def lib():
    from vq_amd import _lib

    return _lib


def _create(lib, nlist=4, dim=6, dtype=0, metric=1):
    coarse = np.zeros((max(nlist, 1), max(dim, 1)), F)
    h = C.c_void_p()
    rc = lib.load().vqhip_ivfflat_create(coarse.ctypes.data_as(lib._f32p), nlist, dim, dtype, metric, C.byref(h))
    return rc, h


def test_cabi_create_checks(lib):
    L = lib.load()
    h = C.c_void_p()
    assert L.vqhip_ivfflat_create(None, 4, 6, 0, 1, C.byref(h)) == lib.ERR_NULL_PTR
    assert L.vqhip_ivfflat_create(np.zeros((4, 6), F).ctypes.data_as(lib._f32p), 4, 6, 0, 1, None) == lib.ERR_NULL_PTR
    assert _create(lib, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, nlist=65537)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dim=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dtype=2)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, metric=7)[0] == lib.ERR_INVALID_INPUT
    for metric in K.METRICS:  # the cosines included
        rc, h = _create(lib, metric=metric, dtype=1)
        assert rc == lib.OK
        L.vqhip_ivfflat_destroy(h)


def test_cabi_add_info_sizes_and_search_bounds_are_host_only(lib):
    L = lib.load()
    rc, h = _create(lib, nlist=4, dim=6, dtype=1, metric=lib.COSINE)
    assert rc == lib.OK
    try:
        lid = np.array([0, 3, 3], np.uint32)
        rows = np.ones((3, 6), np.float16)
        assert L.vqhip_ivfflat_add(h, lid.ctypes.data_as(lib._u32p), rows.ctypes.data_as(lib._vp), 3) == lib.OK
        bad = np.array([0, 4, 1], np.uint32)
        assert L.vqhip_ivfflat_add(h, bad.ctypes.data_as(lib._u32p), rows.ctypes.data_as(lib._vp), 3) == lib.ERR_INVALID_INPUT
        assert "list id 4" in lib.last_error()
        assert L.vqhip_ivfflat_add(h, None, None, 0) == lib.OK
        assert L.vqhip_ivfflat_add(h, None, rows.ctypes.data_as(lib._vp), 3) == lib.ERR_NULL_PTR
        n, nlist, dim, dtype, metric = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
        assert L.vqhip_ivfflat_info(h, C.byref(n), C.byref(nlist), C.byref(dim), C.byref(dtype), C.byref(metric)) == lib.OK
        assert (n.value, nlist.value, dim.value, dtype.value, metric.value) == (3, 4, 6, 1, lib.COSINE)  # the refused add stored nothing
        assert L.vqhip_ivfflat_info(h, None, None, None, None, None) == lib.OK
        sizes = np.zeros(4, np.uint64)
        assert L.vqhip_ivfflat_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK
        assert sizes.tolist() == [1, 0, 0, 2]
        q = np.zeros((2, 6), F)
        idx = np.zeros((2, 8), np.uint32)
        dist = np.zeros((2, 8), F)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 4)):  # nprobe in [1, nlist], topk in [1, n]
            assert L.vqhip_ivfflat_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfflat_search_device(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfflat_probe(h, qp, 2, 0, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfflat_probe(h, qp, 2, 5, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfflat_search(h, qp, 0, 2, 2, ip, dp) == lib.OK  # nq = 0
        assert L.vqhip_ivfflat_search(h, None, 2, 2, 2, ip, dp) == lib.ERR_NULL_PTR
    finally:
        L.vqhip_ivfflat_destroy(h)


def test_several_adds_equal_one_add(lib):
    rng = np.random.default_rng(21)
    coarse, lists, rows, _ = _case(rng, 200, 6, 5, dtype=np.float16)
    one = lib.IVFFlat(coarse, lib.EUCLIDEAN, np.float16)
    many = lib.IVFFlat(coarse, lib.EUCLIDEAN, np.float16)
    a, b = _index(nlist=6, dim=5, dtype=np.float16), _index(nlist=6, dim=5, dtype=np.float16)
    try:
        one.add(lists, rows)
        a.add_rows(lists, rows)
        for part in np.array_split(np.arange(200), 7):
            many.add(lists[part], rows[part])
            b.add_rows(lists[part], rows[part])
        assert one.info() == many.info() == (200, 6, 5, 1, lib.EUCLIDEAN)
        assert np.array_equal(one.list_sizes(), many.list_sizes())
        assert np.array_equal(one.list_sizes(), np.bincount(lists, minlength=6))
        assert np.array_equal(a.list_ids, b.list_ids) and np.array_equal(a.list_ids, lists)
        assert np.array_equal(a.rows.view(np.uint16), b.rows.view(np.uint16)) and np.array_equal(a.rows, rows)
        assert np.array_equal(a.list_sizes(), one.list_sizes())
    finally:
        one.close()
        many.close()
