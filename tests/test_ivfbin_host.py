"""CPU checks of the inverted-file binary index (vq_amd.IVFBinaryIndex, include/vqhip.h vqhip_ivfbin_*): the numpy statement
(tests/ref_ivfbin.py) against a double loop on a tiny case and against the binary index's statement at nprobe == nlist, the
argument checks of the Python class and of the C ABI that come before any device work, the host-only ABI calls
(add_packed, add_codes, packed, info, list_sizes), and the VQIVFBN1 file."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_binary as B
import ref_ivf as I
import ref_ivfbin as R
import ref_knn as K

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
BQ = (0.25, 3, 200)


def _case(rng, n, nlist, dim, nq=6):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    codes[n // 2:n // 2 + 5] = codes[:5]  # duplicate rows: equal distances, ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    return coarse, lists, codes, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_statement_against_a_double_loop():
    """H counted bit by bit and D summed term by term in f32, on 30 rows of 37 dimensions in 4 lists; the probe under
    another metric than the reported distance"""
    rng = np.random.default_rng(2)
    coarse, lists, codes, Q = _case(rng, 30, 4, 37, nq=3)
    Q[1, 5], Q[2, 7] = np.nan, -0.0
    thr, low, high = BQ
    rbits = codes >= high
    words = B.pack(rbits)
    for metric in B.METRICS:
        for nprobe in (1, 2, 4):
            want_i, want_d = R.search(metric, K.MANHATTAN, coarse, lists, BQ, words, 37, Q, nprobe, 8)
            P = K.search(K.MANHATTAN, Q, coarse, nprobe)[0]
            for j in range(Q.shape[0]):
                pairs = []
                for i in range(30):
                    if lists[i] not in P[j]:
                        continue
                    h = sum(int(bool(Q[j, t] >= F(thr)) != bool(rbits[i, t])) for t in range(37))
                    a = F(high) - F(low)
                    s = F(0.0)
                    for _ in range(h):
                        s = F(s + (a if metric == B.MAN else F(a * a)))
                    pairs.append((h, i, np.sqrt(s) if metric == B.EUC else s))
                pairs.sort(key=lambda p: (p[0], p[1]))
                top = pairs[:8]
                assert [i for _, i, _ in top] == want_i[j, :len(top)].tolist()
                assert np.array_equal(np.array([d for _, _, d in top], F).view(np.uint32), want_d[j, :len(top)].view(np.uint32))
                assert np.all(want_i[j, len(top):] == R.PAD_ID) and np.all(want_d[j, len(top):].view(np.uint32) == I.INF_BITS)


@pytest.mark.parametrize("low,high", R.LOW_HIGH)
@pytest.mark.parametrize("metric", B.METRICS)
def test_statement_all_lists_is_the_binary_index(metric, low, high):
    rng = np.random.default_rng(3 + metric)
    coarse, lists, codes, Q = _case(rng, 300, 9, 40)
    Q[1, 0] = np.nan
    Q[2] = -0.0
    words = B.pack(B.bits_u8(codes, high))
    for topk in (1, 25, 300):
        _same(R.search(metric, K.COSINE, coarse, lists, (0.0, low, high), words, 40, Q, 9, topk),
              B.search(B.pack(B.bits_f32(Q, 0.0)), words, 40, low, high, metric, topk))


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, dim=37, metric="manhattan", bq=BQ, coarse_metric="euclidean"):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFBinaryIndex(rng.standard_normal((nlist, dim)).astype(F), vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(metric),
                                 vq_amd.Distance(coarse_metric))


def test_python_construction_checks():
    import vq_amd
    from vq_amd import InvalidParameter

    bq = vq_amd.BinaryQuantizer(*BQ)
    for bad in (np.zeros((0, 6), F), np.zeros((65537, 6), F), np.zeros(6, F), np.zeros((4, 0), F), np.zeros((4, 8193), F)):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFBinaryIndex(bad, bq)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFBinaryIndex(np.zeros((4, 6), F), bq, "euclidean")
    with pytest.raises(InvalidParameter):
        vq_amd.IVFBinaryIndex(np.zeros((4, 6), F), bq, None, "euclidean")
    with pytest.raises(InvalidParameter):
        vq_amd.IVFBinaryIndex(np.zeros((4, 6), F), BQ)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFBinaryIndex.train(np.zeros((40, 6), F), 4, BQ)
    for name in NAMES[3:]:  # cosine is refused for the reported distance, as BinaryIndex refuses it ...
        with pytest.raises(InvalidParameter) as e:
            vq_amd.IVFBinaryIndex(np.zeros((4, 6), F), bq, vq_amd.Distance(name))
        with pytest.raises(InvalidParameter) as e2:
            vq_amd.BinaryIndex(np.zeros((4, 6), F), bq, vq_amd.Distance(name))
        assert str(e.value) == str(e2.value)
    for name in NAMES[:3]:
        for cname in NAMES:  # ... and accepted for the probe
            ix = vq_amd.IVFBinaryIndex(np.zeros((4, 8192), F), bq, vq_amd.Distance(name), vq_amd.Distance(cname))
            assert ix.nlist == 4 and len(ix) == 0 and ix.dim == 8192 and ix.quantizer is bq
            assert ix.distance.name() == name and ix.coarse_distance.name() == cname
            assert np.array_equal(ix.list_sizes(), np.zeros(4, np.uint64))
            assert ix.packed().shape == (0, 256) and ix.packed().dtype == np.uint32
            assert ix.coarse_centroids.shape == (4, 8192) and ix.list_ids.shape == (0,)
    ix = vq_amd.IVFBinaryIndex(np.zeros((4, 6), F))  # the defaults are BinaryIndex's, and a Euclidean probe
    assert ix.distance.name() == "manhattan" and ix.coarse_distance.name() == "euclidean"
    assert (ix.quantizer.threshold, ix.quantizer.low, ix.quantizer.high) == (0.0, 0, 1)


def test_python_add_and_search_checks():
    from vq_amd import DimensionMismatch, InvalidParameter

    ix = _index()
    for add, good in ((ix.add_codes, np.zeros((2, 37), np.uint8)), (ix.add_rows, np.zeros((2, 37), F)),
                      (ix.add_packed, np.zeros((2, 2), np.uint32))):
        w = good.shape[1]
        with pytest.raises(InvalidParameter):
            add([0, 5], good)  # list id >= nlist
        with pytest.raises(InvalidParameter):
            add([0, -1], good)
        with pytest.raises(InvalidParameter):
            add([0.5, 1.0], good)
        with pytest.raises(InvalidParameter):
            add([[0, 1]], good)
        with pytest.raises(InvalidParameter):
            add([0, 1], good.reshape(2 * w))
        with pytest.raises(DimensionMismatch):
            add([0, 1], good[:, :w - 1])
        with pytest.raises(DimensionMismatch):
            add([0, 1, 2], good)
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 1], np.zeros((2, 37), np.int32))  # codes are bytes
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 1], np.zeros((2, 37), np.int32))  # rows are floating point
    with pytest.raises(InvalidParameter):
        ix.add_packed([0, 1], np.zeros((2, 2), np.int32))  # words are uint32
    with pytest.raises(InvalidParameter):
        ix.add_packed([0, 1], np.array([[0, 0], [0, 1 << 5]], np.uint32))  # dimension 37 of 37: a pad bit
    with pytest.raises(DimensionMismatch):
        ix.add(np.zeros((2, 5), F))
    assert len(ix) == 0
    assert ix.add_codes([1, 1, 4], np.full((3, 37), 200, np.uint8)).tolist() == [0, 1, 2]
    assert ix.add_packed([0], np.array([[5, 1 << 4]], np.uint32)).tolist() == [3]  # dimension 36: the last real bit
    assert ix.add_codes([2], np.full((1, 37), 199, np.uint8)).tolist() == [4]
    assert ix.add_codes([], np.zeros((0, 37), np.uint8)).tolist() == []
    assert ix.list_sizes().tolist() == [1, 2, 1, 0, 1] and len(ix) == 5 and ix.list_ids.tolist() == [1, 1, 4, 0, 2]
    assert ix.packed().tolist() == [[0xFFFFFFFF, 31]] * 3 + [[5, 16], [0, 0]]
    q = np.zeros((2, 37), F)
    for bad in (0, 6, 1025):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=1, nprobe=bad)
        with pytest.raises(InvalidParameter):
            ix.probe(q, nprobe=bad)
        with pytest.raises(InvalidParameter):
            ix.search_device(0, 2, 1, 0, 0, nprobe=bad)
    for bad in (0, 6):
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
    assert not hasattr(ix, "range_search")
    i, d = ix.search(np.zeros((0, 37), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2) and ix.probe(np.zeros((0, 37), F), 3).shape == (0, 3)


def test_python_save_load_round_trip(tmp_path):
    import vq_amd

    rng = np.random.default_rng(4)
    ix = _index(rng, nlist=7, dim=37, metric="euclidean", coarse_metric="cosine")
    lists = rng.integers(0, 7, 50)
    codes = rng.integers(0, 256, (50, 37)).astype(np.uint8)
    words = B.pack(B.bits_u8(codes, 200))
    ix.add_codes(lists[:20], codes[:20])
    ix.add_packed(lists[20:], words[20:])
    p = tmp_path / "ix.bin"
    ix.save(p)
    back = vq_amd.IVFBinaryIndex.load(p)
    assert back.distance.name() == "euclidean" and back.coarse_distance.name() == "cosine"
    assert back.nlist == 7 and len(back) == 50 and back.dim == 37
    assert (back.quantizer.threshold, back.quantizer.low, back.quantizer.high) == BQ
    assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
    assert np.array_equal(back.list_ids, lists.astype(np.uint32))
    assert back.packed().dtype == np.uint32 and np.array_equal(back.packed(), words)
    assert len(p.read_bytes()) == 44 + 4 * (7 * 37 + 50) + 50 * 2 * 4
    assert back.add_codes([6], codes[:1]).tolist() == [50]  # a loaded index takes more rows


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], np.arange(111, dtype=np.uint8).reshape(3, 37) + 140)
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = mutate(bytearray(p.read_bytes()))
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        vq_amd.IVFBinaryIndex.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


BASE = 44 + 4 * 4 * 37  # the header and the centroids of _corrupt's file


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                    # truncated header
    lambda r: r[:43],                    # ... by one byte
    lambda r: b"VQIVFSQ1" + r[8:],       # another magic
    _field(8, "<I", 3),                  # metric: cosine
    _field(8, "<I", 5),                  # metric out of range
    _field(12, "<I", 5),                 # coarse metric out of range
    _field(16, "<I", 0),                 # dim 0
    _field(16, "<I", 8193),              # dim too large
    _field(20, "<I", 0),                 # nlist 0
    _field(20, "<I", 70000),             # nlist too large
    _field(24, "<f", float("nan")),      # threshold not finite
    _field(28, "<I", 256),               # low beyond u8
    _field(32, "<I", 300),               # high beyond u8
    _field(36, "<Q", 4),                 # more rows than the file holds
    _field(36, "<Q", 1 << 40),           # n beyond 2^32
    lambda r: r[:BASE - 4],              # truncated centroids
    lambda r: r[:BASE + 8],              # truncated list ids
    lambda r: r[:BASE + 12 + 4],         # truncated words: one of six
    lambda r: r[:-1],                    # truncated words: the last byte
    lambda r: r + b"\0",                 # trailing bytes
    _field(BASE + 4, "<I", 4),           # list id 4 of nlist 4
    _field(BASE + 12 + 4, "<I", 1 << 5),  # row 0, dimension 37: a pad bit
    _field(BASE + 12 + 20, "<I", 1 << 31),  # row 2, dimension 63: a pad bit
])
def test_python_load_rejects_corrupt_files(tmp_path, mutate):
    _corrupt(tmp_path, mutate)


def test_python_load_accepts_the_uncorrupted_file(tmp_path):
    """_corrupt's file as it is, and with its last real bit flipped: the mutations above are what load refuses"""
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], np.arange(111, dtype=np.uint8).reshape(3, 37) + 140)
    p = tmp_path / "c.bin"
    ix.save(p)
    assert np.array_equal(vq_amd.IVFBinaryIndex.load(p).packed(), ix.packed())
    raw = bytearray(p.read_bytes())
    struct.pack_into("<I", raw, BASE + 12 + 4, 1 << 4)
    p.write_bytes(bytes(raw))
    assert vq_amd.IVFBinaryIndex.load(p).packed()[0, 1] == 16


# ---- the C ABI: parameters checked before any device work ----------------------------------------

@pytest.fixture(scope="module")
def lib():
    from vq_amd import _lib

    return _lib


def _create(lib, nlist=4, dim=37, metric=2, cmetric=1, bq=BQ):
    coarse = np.zeros((max(nlist, 1), max(dim, 1)), F)
    h = C.c_void_p()
    rc = lib.load().vqhip_ivfbin_create(bq[0], bq[1], bq[2], coarse.ctypes.data_as(lib._f32p), nlist, dim, metric, cmetric, C.byref(h))
    return rc, h


def test_cabi_create_checks(lib):
    L = lib.load()
    h = C.c_void_p()
    coarse = np.zeros((4, 37), F).ctypes.data_as(lib._f32p)
    assert L.vqhip_ivfbin_create(0.0, 0, 1, None, 4, 37, 2, 1, C.byref(h)) == lib.ERR_NULL_PTR
    assert L.vqhip_ivfbin_create(0.0, 0, 1, coarse, 4, 37, 2, 1, None) == lib.ERR_NULL_PTR
    assert _create(lib, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, nlist=65537)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dim=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dim=8193)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, metric=7)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, cmetric=7)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, cmetric=-1)[0] == lib.ERR_INVALID_INPUT
    # cosine for the reported distance: vqhip_binary_create's status and text (it refuses before any device work too)
    words = np.zeros((1, 2), np.uint32)
    for cos in (lib.COSINE, lib.COSINE_UNCLAMPED):
        rc = L.vqhip_binary_create(words.ctypes.data_as(C.c_void_p), lib.BINARY_PACKED, 1, 37, 0.0, 0, 1, cos, C.byref(h))
        text = lib.last_error()
        assert rc == lib.ERR_UNSUPPORTED and _create(lib, metric=cos)[0] == rc and lib.last_error() == text
    for bad in ((float("nan"), 0, 1), (float("inf"), 0, 1), (0.0, 256, 1), (0.0, 0, 256)):
        rc = L.vqhip_bq_check(bad[0], bad[1], bad[2])
        text = lib.last_error()
        assert rc != lib.OK and _create(lib, bq=bad)[0] == rc and lib.last_error() == text  # vqhip_bq_check's, unchanged
    for metric in B.METRICS:
        for cmetric in K.METRICS:  # the cosines included
            for low, high in R.LOW_HIGH:
                for dim in (1, 8192):
                    rc, h = _create(lib, dim=dim, metric=metric, cmetric=cmetric, bq=(0.5, low, high))
                    assert rc == lib.OK
                    L.vqhip_ivfbin_destroy(h)


def test_cabi_adds_info_sizes_packed_and_search_bounds_are_host_only(lib):
    L = lib.load()
    rc, h = _create(lib, nlist=4, dim=37, metric=lib.EUCLIDEAN, cmetric=lib.COSINE)
    assert rc == lib.OK
    try:
        lid = np.array([0, 3, 3], np.uint32)
        codes = np.arange(111, dtype=np.uint8).reshape(3, 37) + 140  # on both sides of high = 200
        words = B.pack(B.bits_u8(codes, 200))
        lp, cp, wp = lid.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._u8p), words.ctypes.data_as(lib._u32p)
        assert L.vqhip_ivfbin_add_codes(h, lp, cp, 3) == lib.OK
        assert L.vqhip_ivfbin_add_packed(h, lp, wp, 3) == lib.OK
        bad = np.array([0, 4, 1], np.uint32)
        bp = bad.ctypes.data_as(lib._u32p)
        rows = np.zeros((3, 37), F).ctypes.data_as(lib._f32p)
        for rc in (L.vqhip_ivfbin_add_codes(h, bp, cp, 3), L.vqhip_ivfbin_add_packed(h, bp, wp, 3),
                   L.vqhip_ivfbin_add_rows(h, bp, rows, 3)):  # (add_rows: before the device)
            assert rc == lib.ERR_INVALID_INPUT and "list id 4" in lib.last_error()
        # a set pad bit: vqhip_binary_create's status and text
        padded = words.copy()
        padded[1, 1] |= np.uint32(1 << 5)
        hb = C.c_void_p()
        rc = L.vqhip_binary_create(padded.ctypes.data_as(C.c_void_p), lib.BINARY_PACKED, 3, 37, 0.25, 3, 200, lib.EUCLIDEAN, C.byref(hb))
        text = lib.last_error()
        assert rc == lib.ERR_INVALID_INPUT and "row 1 has a pad bit set" in text
        assert L.vqhip_ivfbin_add_packed(h, lp, padded.ctypes.data_as(lib._u32p), 3) == rc and lib.last_error() == text
        assert L.vqhip_ivfbin_add_codes(h, None, None, 0) == lib.OK and L.vqhip_ivfbin_add_rows(h, None, None, 0) == lib.OK
        assert L.vqhip_ivfbin_add_packed(h, None, None, 0) == lib.OK
        assert L.vqhip_ivfbin_add_codes(h, None, cp, 3) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfbin_add_codes(h, lp, None, 3) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfbin_add_packed(h, lp, None, 3) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfbin_add_rows(h, lp, None, 3) == lib.ERR_NULL_PTR
        n, nlist, dim, metric, cmetric = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int()
        thr, low, high = C.c_float(), C.c_uint32(), C.c_uint32()
        assert L.vqhip_ivfbin_info(h, C.byref(n), C.byref(nlist), C.byref(dim), C.byref(metric), C.byref(cmetric), C.byref(thr),
                                   C.byref(low), C.byref(high)) == lib.OK
        assert (n.value, nlist.value, dim.value, metric.value, cmetric.value, thr.value, low.value, high.value) == \
            (6, 4, 37, lib.EUCLIDEAN, lib.COSINE, 0.25, 3, 200)  # (nothing of the refused adds was stored)
        assert L.vqhip_ivfbin_info(h, *[None] * 8) == lib.OK
        sizes = np.zeros(4, np.uint64)
        assert L.vqhip_ivfbin_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK
        assert sizes.tolist() == [2, 0, 0, 4]
        out = np.zeros((6, 2), np.uint32)
        assert L.vqhip_ivfbin_packed(h, out.ctypes.data_as(lib._u32p)) == lib.OK
        assert np.array_equal(out, np.concatenate([words, words]))  # add_codes packs as the statement does
        assert L.vqhip_ivfbin_packed(h, None) == lib.ERR_NULL_PTR
        q = np.zeros((2, 37), F)
        idx = np.zeros((2, 8), np.uint32)
        dist = np.zeros((2, 8), F)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 7)):  # nprobe in [1, nlist], topk in [1, n]
            assert L.vqhip_ivfbin_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfbin_search_device(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfbin_probe(h, qp, 2, 0, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfbin_probe(h, qp, 2, 5, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfbin_search(h, qp, 0, 2, 2, ip, dp) == lib.OK  # nq = 0
        assert L.vqhip_ivfbin_search(h, None, 2, 2, 2, ip, dp) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfbin_probe(h, qp, 2, 2, None) == lib.ERR_NULL_PTR
        assert L.vqhip_ivfbin_list_sizes(h, None) == lib.ERR_NULL_PTR and L.vqhip_ivfbin_info(None, *[None] * 8) == lib.ERR_NULL_PTR
    finally:
        L.vqhip_ivfbin_destroy(h)


@pytest.mark.parametrize("dim", [1, 31, 32, 33, 100])
def test_several_adds_equal_one_add(lib, dim):
    rng = np.random.default_rng(21)
    coarse, lists, codes, _ = _case(rng, 200, 6, dim)
    words = B.pack(B.bits_u8(codes, 200))
    one = lib.IVFBin(coarse, *BQ, lib.MANHATTAN, lib.EUCLIDEAN)
    many = lib.IVFBin(coarse, *BQ, lib.MANHATTAN, lib.EUCLIDEAN)
    a, b = _index(nlist=6, dim=dim), _index(nlist=6, dim=dim)
    try:
        one.add_codes(lists, codes)
        a.add_codes(lists, codes)
        for k, part in enumerate(np.array_split(np.arange(200), 7)):
            if k % 2:
                many.add_codes(lists[part], codes[part])
                b.add_codes(lists[part], codes[part])
            else:
                many.add_packed(lists[part], words[part])
                b.add_packed(lists[part], words[part])
        assert one.info() == many.info() == (200, 6, dim, lib.MANHATTAN, lib.EUCLIDEAN, 0.25, 3, 200)
        assert np.array_equal(one.list_sizes(), many.list_sizes())
        assert np.array_equal(one.list_sizes(), np.bincount(lists, minlength=6))
        assert np.array_equal(one.packed(), words) and np.array_equal(many.packed(), words)
        assert np.array_equal(a.list_ids, b.list_ids) and np.array_equal(a.list_ids, lists)
        assert np.array_equal(a.packed(), b.packed()) and np.array_equal(a.packed(), words)
        assert np.array_equal(a.list_sizes(), one.list_sizes())
    finally:
        one.close()
        many.close()
