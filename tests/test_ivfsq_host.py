"""CPU checks of the inverted-file scalar index (vq_amd.IVFScalarIndex, include/vqhip.h vqhip_ivfsq_*): the numpy statement
(tests/ref_ivfsq.py) against a double loop on a tiny case and against the scalar index's statement at nprobe == nlist, the
argument checks of the Python class and of the C ABI that come before any device work, the host-only ABI calls
(add_codes, codes, info, list_sizes), and the VQIVFSQ1 file."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_ivf as I
import ref_ivfsq as R
import ref_knn as K
import ref_sqindex as S

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
SQ = (-3.0, 5.0, 17)


def _case(rng, n, nlist, dim, nq=6):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)  # the full byte range: codes >= levels occur
    codes[n // 2:n // 2 + 5] = codes[:5]  # duplicate rows: equal distances, ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    return coarse, lists, codes, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_statement_against_a_double_loop():
    """squared Euclidean and Manhattan spelled out pair by pair and element by element in f32, on 30 rows in 4 lists"""
    rng = np.random.default_rng(2)
    coarse, lists, codes, Q = _case(rng, 30, 4, 3, nq=3)
    mn, mx, levels = SQ
    step = F((F(mx) - F(mn)) / F(levels - 1))
    assert np.array_equal(S.table(SQ), np.array([F(mn) + F(c) * step for c in range(256)], F))
    for metric in (K.SQUARED_EUCLIDEAN, K.MANHATTAN):
        for nprobe in (1, 2, 4):
            want_i, want_d = R.search(metric, coarse, lists, SQ, codes, Q, nprobe, 8)
            P = R.probe(metric, coarse, Q, nprobe)
            for j in range(Q.shape[0]):
                pairs = []
                for i in range(30):
                    if lists[i] not in P[j]:
                        continue
                    acc = F(-0.0)
                    for t in range(3):
                        v = F(F(mn) + F(F(codes[i, t]) * step))
                        diff = F(Q[j, t] - v)
                        acc = F(acc + (F(diff * diff) if metric == K.SQUARED_EUCLIDEAN else F(abs(diff))))
                    pairs.append((float(acc), i))
                pairs.sort()
                top = pairs[:8]
                assert [i for _, i in top] == want_i[j, :len(top)].tolist()
                assert np.array_equal(np.array([d for d, _ in top], F).view(np.uint32), want_d[j, :len(top)].view(np.uint32))
                assert np.all(want_i[j, len(top):] == R.PAD_ID) and np.all(want_d[j, len(top):].view(np.uint32) == I.INF_BITS)


@pytest.mark.parametrize("sq", S.QUANTIZERS)
@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_all_lists_is_the_scalar_index(metric, sq):
    rng = np.random.default_rng(3 + metric)
    coarse, lists, codes, Q = _case(rng, 300, 9, 7)
    Q[1, 0] = np.nan
    Q[2] = 0
    with np.errstate(all="ignore"):
        for topk in (1, 25, 300):
            _same(R.search(metric, coarse, lists, sq, codes, Q, 9, topk), S.search(metric, Q, sq, codes, topk))


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, dim=6, metric="euclidean", sq=SQ):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFScalarIndex(rng.standard_normal((nlist, dim)).astype(F), vq_amd.ScalarQuantizer(*sq), vq_amd.Distance(metric))


def test_python_construction_checks():
    import vq_amd
    from vq_amd import InvalidParameter

    sq = vq_amd.ScalarQuantizer(*SQ)
    for bad in (np.zeros((0, 6), F), np.zeros((65537, 6), F), np.zeros(6, F), np.zeros((4, 0), F)):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFScalarIndex(bad, sq)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalarIndex(np.zeros((4, 6), F), sq, "euclidean")
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalarIndex(np.zeros((4, 6), F), SQ)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalarIndex.train(np.zeros((40, 6), F), 4, SQ)
    for name in NAMES:  # the cosines included
        ix = vq_amd.IVFScalarIndex(np.zeros((4, 6), F), sq, vq_amd.Distance(name))
        assert ix.nlist == 4 and len(ix) == 0 and ix.dim == 6 and ix.quantizer is sq and ix.distance.name() == name
        assert np.array_equal(ix.list_sizes(), np.zeros(4, np.uint64)) and ix.codes.shape == (0, 6) and ix.codes.dtype == np.uint8
        assert ix.coarse_centroids.shape == (4, 6) and ix.list_ids.shape == (0,)


def test_python_add_and_search_checks():
    from vq_amd import DimensionMismatch, InvalidParameter

    ix = _index()
    z = np.zeros((2, 6), np.uint8)
    for add, good in ((ix.add_codes, z), (ix.add_rows, np.zeros((2, 6), F))):
        with pytest.raises(InvalidParameter):
            add([0, 5], good)  # list id >= nlist
        with pytest.raises(InvalidParameter):
            add([0, -1], good)
        with pytest.raises(InvalidParameter):
            add([0.5, 1.0], good)
        with pytest.raises(InvalidParameter):
            add([[0, 1]], good)
        with pytest.raises(InvalidParameter):
            add([0, 1], good.reshape(12))
        with pytest.raises(DimensionMismatch):
            add([0, 1], good[:, :5])
        with pytest.raises(DimensionMismatch):
            add([0, 1, 2], good)
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 1], np.zeros((2, 6), np.int32))  # codes are bytes
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 1], np.zeros((2, 6), np.int32))  # rows are floating point
    with pytest.raises(DimensionMismatch):
        ix.add(np.zeros((2, 5), F))
    assert len(ix) == 0
    assert ix.add_codes([1, 1, 4], np.full((3, 6), 200, np.uint8)).tolist() == [0, 1, 2]
    assert ix.add_codes([0], np.zeros((1, 6), np.uint8)).tolist() == [3]
    assert ix.add_codes([], np.zeros((0, 6), np.uint8)).tolist() == []
    assert ix.list_sizes().tolist() == [1, 2, 0, 0, 1] and len(ix) == 4 and ix.list_ids.tolist() == [1, 1, 4, 0]
    assert ix.codes.tolist() == [[200] * 6] * 3 + [[0] * 6]
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
    with pytest.raises(InvalidParameter):
        ix.search(q, topk=1, nprobe=1, rerank=object())
    i, d = ix.search(np.zeros((0, 6), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2) and ix.probe(np.zeros((0, 6), F), 3).shape == (0, 3)


def test_python_save_load_round_trip(tmp_path):
    import vq_amd

    rng = np.random.default_rng(4)
    ix = _index(rng, nlist=7, dim=6, metric="cosine")
    lists = rng.integers(0, 7, 50)
    codes = rng.integers(0, 256, (50, 6)).astype(np.uint8)
    ix.add_codes(lists[:20], codes[:20])
    ix.add_codes(lists[20:], codes[20:])
    p = tmp_path / "ix.bin"
    ix.save(p)
    back = vq_amd.IVFScalarIndex.load(p)
    assert back.distance.metric == ix.distance.metric and back.nlist == 7 and len(back) == 50 and back.dim == 6
    assert (back.quantizer.min, back.quantizer.max, back.quantizer.levels) == SQ
    assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
    assert np.array_equal(back.list_ids, lists.astype(np.uint32))
    assert back.codes.dtype == np.uint8 and np.array_equal(back.codes, codes)
    assert len(p.read_bytes()) == 40 + 4 * (7 * 6 + 50) + 50 * 6
    assert back.add_codes([6], codes[:1]).tolist() == [50]  # a loaded index takes more rows


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], np.arange(18, dtype=np.uint8).reshape(3, 6))
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = mutate(bytearray(p.read_bytes()))
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        vq_amd.IVFScalarIndex.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


BASE = 40 + 4 * 4 * 6  # the header and the centroids of _corrupt's file


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                    # truncated header
    lambda r: b"VQIVFFL1" + r[8:],       # another magic
    _field(8, "<I", 5),                  # metric out of range
    _field(12, "<I", 0),                 # dim 0
    _field(16, "<I", 0),                 # nlist 0
    _field(16, "<I", 70000),             # nlist too large
    _field(20, "<f", float("nan")),      # min not finite
    _field(24, "<f", -4.0),              # max below min
    _field(28, "<I", 1),                 # levels below 2
    _field(28, "<I", 257),               # levels above 256
    _field(32, "<Q", 4),                 # more rows than the file holds
    _field(32, "<Q", 1 << 40),           # n beyond 2^32
    lambda r: r[:BASE - 4],              # truncated centroids
    lambda r: r[:BASE + 8],              # truncated list ids
    lambda r: r[:-1],                    # truncated codes
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


def _create(lib, nlist=4, dim=6, metric=1, sq=SQ):
    coarse = np.zeros((max(nlist, 1), max(dim, 1)), F)
    h = C.c_void_p()
    rc = lib.load().vqhip_ivfsq_create(sq[0], sq[1], sq[2], coarse.ctypes.data_as(lib._f32p), nlist, dim, metric, C.byref(h))
    return rc, h


def test_cabi_create_checks(lib):
    L = lib.load()
    h = C.c_void_p()
    coarse = np.zeros((4, 6), F).ctypes.data_as(lib._f32p)
    assert L.vqhip_ivfsq_create(-3.0, 5.0, 17, None, 4, 6, 1, C.byref(h)) == lib.ERR_NULL_PTR
    assert L.vqhip_ivfsq_create(-3.0, 5.0, 17, coarse, 4, 6, 1, None) == lib.ERR_NULL_PTR
    assert _create(lib, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, nlist=65537)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dim=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, metric=7)[0] == lib.ERR_INVALID_INPUT
    step = C.c_float()
    for bad in ((float("nan"), 1.0, 4), (0.0, float("inf"), 4), (1.0, 1.0, 4), (0.0, 1.0, 1), (0.0, 1.0, 257)):
        rc = L.vqhip_sq_check(bad[0], bad[1], bad[2], C.byref(step))
        text = lib.last_error()
        assert rc != lib.OK and _create(lib, sq=bad)[0] == rc and lib.last_error() == text  # vqhip_sq_check's, unchanged
    for metric in K.METRICS:  # the cosines included
        for sq in S.QUANTIZERS:  # the degenerate quantizer included
            rc, h = _create(lib, metric=metric, sq=sq)
            assert rc == lib.OK
            L.vqhip_ivfsq_destroy(h)


def test_cabi_add_info_sizes_codes_and_search_bounds_are_host_only(lib):
    L = lib.load()
    rc, h = _create(lib, nlist=4, dim=6, metric=lib.COSINE)
    assert rc == lib.OK
    try:
        lid = np.array([0, 3, 3], np.uint32)
        codes = np.arange(18, dtype=np.uint8).reshape(3, 6) + 240  # codes >= levels are legal
        lp, cp = lid.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._u8p)
        assert L.vqhip_ivfsq_add_codes(h, lp, cp, 3) == lib.OK
        bad = np.array([0, 4, 1], np.uint32)
        assert L.vqhip_ivfsq_add_codes(h, bad.ctypes.data_as(lib._u32p), cp, 3) == lib.ERR_INVALID_INPUT
        assert "list id 4" in lib.last_error()
        rows = np.zeros((3, 6), F).ctypes.data_as(lib._f32p)
        assert L.vqhip_ivfsq_add_rows(h, bad.ctypes.data_as(lib._u32p), rows, 3) == lib.ERR_INVALID_INPUT  # before the device
        assert "list id 4" in lib.last_error()
        assert L.vqhip_ivfsq_add_codes(h, None, None, 0) == lib.OK and L.vqhip_ivfsq_add_rows(h, None, None, 0) == lib.OK
        assert L.vqhip_ivfsq_add_codes(h, None, cp, 3) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfsq_add_codes(h, lp, None, 3) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfsq_add_rows(h, lp, None, 3) == lib.ERR_NULL_PTR
        n, nlist, dim, metric = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int()
        mn, mx, levels = C.c_float(), C.c_float(), C.c_uint32()
        assert L.vqhip_ivfsq_info(h, C.byref(n), C.byref(nlist), C.byref(dim), C.byref(metric), C.byref(mn), C.byref(mx),
                                  C.byref(levels)) == lib.OK
        assert (n.value, nlist.value, dim.value, metric.value, mn.value, mx.value, levels.value) == (3, 4, 6, lib.COSINE, -3.0, 5.0, 17)
        assert L.vqhip_ivfsq_info(h, None, None, None, None, None, None, None) == lib.OK
        sizes = np.zeros(4, np.uint64)
        assert L.vqhip_ivfsq_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK
        assert sizes.tolist() == [1, 0, 0, 2]
        out = np.zeros((3, 6), np.uint8)
        assert L.vqhip_ivfsq_codes(h, out.ctypes.data_as(lib._u8p)) == lib.OK and np.array_equal(out, codes)
        assert L.vqhip_ivfsq_codes(h, None) == lib.ERR_NULL_PTR
        q = np.zeros((2, 6), F)
        idx = np.zeros((2, 8), np.uint32)
        dist = np.zeros((2, 8), F)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 4)):  # nprobe in [1, nlist], topk in [1, n]
            assert L.vqhip_ivfsq_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfsq_search_device(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq_probe(h, qp, 2, 0, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq_probe(h, qp, 2, 5, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq_search(h, qp, 0, 2, 2, ip, dp) == lib.OK  # nq = 0
        assert L.vqhip_ivfsq_search(h, None, 2, 2, 2, ip, dp) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfsq_probe(h, qp, 2, 2, None) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfsq_list_sizes(h, None) == lib.ERR_NULL_PTR and L.vqhip_ivfsq_info(None, *[None] * 7) == lib.ERR_NULL_PTR
    finally:
        L.vqhip_ivfsq_destroy(h)


def test_several_adds_equal_one_add(lib):
    rng = np.random.default_rng(21)
    coarse, lists, codes, _ = _case(rng, 200, 6, 5)
    one = lib.IVFSQ(coarse, *SQ, lib.EUCLIDEAN)
    many = lib.IVFSQ(coarse, *SQ, lib.EUCLIDEAN)
    a, b = _index(nlist=6, dim=5), _index(nlist=6, dim=5)
    try:
        one.add_codes(lists, codes)
        a.add_codes(lists, codes)
        for part in np.array_split(np.arange(200), 7):
            many.add_codes(lists[part], codes[part])
            b.add_codes(lists[part], codes[part])
        assert one.info() == many.info() == (200, 6, 5, lib.EUCLIDEAN, -3.0, 5.0, 17)
        assert np.array_equal(one.list_sizes(), many.list_sizes())
        assert np.array_equal(one.list_sizes(), np.bincount(lists, minlength=6))
        assert np.array_equal(one.codes(), codes) and np.array_equal(many.codes(), codes)
        assert np.array_equal(a.list_ids, b.list_ids) and np.array_equal(a.list_ids, lists)
        assert np.array_equal(a.codes, b.codes) and np.array_equal(a.codes, codes)
        assert np.array_equal(a.list_sizes(), one.list_sizes())
    finally:
        one.close()
        many.close()
