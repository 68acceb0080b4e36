"""CPU checks of the inverted-file 4-bit scalar index (vq_amd.IVFScalar4Index, include/vqhip.h vqhip_ivfsq4_*): the numpy
statement (tests/ref_ivfsq4.py) against a double loop on a tiny case and against the 4-bit scalar index's statement at
nprobe == nlist, the argument checks of the Python class and of the C ABI that come before any device work, the host-only
calls (add_codes, add_packed, codes, packed, info, list_sizes, remove), and the VQIVFS41 file."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_ivf as I
import ref_ivfsq4 as R
import ref_knn as K
import ref_sq4 as S4

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
SQ = (-3.5, 200.0, 5)  # few levels: codes 5 .. 15 are above them, and legal


def _case(rng, n, nlist, dim, nq=6):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 16, (n, dim)).astype(np.uint8)  # every nibble value: codes >= levels occur
    codes[n // 2:n // 2 + 5] = codes[:5]  # duplicate rows: equal distances, ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    return coarse, lists, codes, Q


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_statement_against_a_double_loop():
    """squared Euclidean and Manhattan spelled out pair by pair and nibble by nibble in f32, on 30 rows in 4 lists of 11
    dimensions (two words a row, the second with five pad nibbles)"""
    rng = np.random.default_rng(2)
    coarse, lists, codes, Q = _case(rng, 30, 4, 11, nq=3)
    words = S4.pack4(codes)
    mn, mx, levels = SQ
    step = F((F(mx) - F(mn)) / F(levels - 1))
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
                    for t in range(11):
                        c = (int(words[i, t // 8]) >> (4 * (t % 8))) & 15
                        v = F(F(mn) + F(F(c) * step))
                        diff = F(Q[j, t] - v)
                        acc = F(acc + (F(diff * diff) if metric == K.SQUARED_EUCLIDEAN else F(abs(diff))))
                    pairs.append((float(acc), i))
                pairs.sort()
                top = pairs[:8]
                assert [i for _, i in top] == want_i[j, :len(top)].tolist()
                assert np.array_equal(np.array([d for d, _ in top], F).view(np.uint32), want_d[j, :len(top)].view(np.uint32))
                assert np.all(want_i[j, len(top):] == R.PAD_ID) and np.all(want_d[j, len(top):].view(np.uint32) == I.INF_BITS)


@pytest.mark.parametrize("sq", R.QUANTIZERS)
@pytest.mark.parametrize("metric", K.METRICS)
def test_statement_all_lists_is_the_4bit_scalar_index(metric, sq):
    rng = np.random.default_rng(3 + metric)
    coarse, lists, codes, Q = _case(rng, 300, 9, 7)
    Q[1, 0] = np.nan
    Q[2] = 0
    with np.errstate(all="ignore"):
        for topk in (1, 25, 300):
            _same(R.search(metric, coarse, lists, sq, codes, Q, 9, topk), S4.search(metric, Q, S4.pack4(codes), 7, *sq, topk))


def test_name_is_exported():
    import vq_amd

    assert "IVFScalar4Index" in vq_amd.__all__ and vq_amd.IVFScalar4Index is vq_amd.ivf_scalar4.IVFScalar4Index


# ---- the Python class: checks before any device ------------------------------------------------

def _index(rng=None, nlist=5, dim=6, metric="euclidean", sq=SQ):
    import vq_amd

    rng = rng or np.random.default_rng(0)
    return vq_amd.IVFScalar4Index(rng.standard_normal((nlist, dim)).astype(F), vq_amd.ScalarQuantizer(*sq), vq_amd.Distance(metric))


def test_python_construction_checks():
    import vq_amd
    from vq_amd import InvalidParameter

    sq = vq_amd.ScalarQuantizer(*SQ)
    for bad in (np.zeros((0, 6), F), np.zeros((65537, 6), F), np.zeros(6, F), np.zeros((4, 0), F)):
        with pytest.raises(InvalidParameter):
            vq_amd.IVFScalar4Index(bad, sq)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalar4Index(np.zeros((4, 6), F), sq, "euclidean")
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalar4Index(np.zeros((4, 6), F), SQ)
    with pytest.raises(InvalidParameter):
        vq_amd.IVFScalar4Index.train(np.zeros((40, 6), F), 4, SQ)
    for levels in (17, 256):  # more than a nibble holds
        with pytest.raises(InvalidParameter, match="at most 16"):
            vq_amd.IVFScalar4Index(np.zeros((4, 6), F), vq_amd.ScalarQuantizer(0.0, 1.0, levels))
        with pytest.raises(InvalidParameter, match="at most 16"):
            vq_amd.IVFScalar4Index.train(np.zeros((40, 6), F), 4, vq_amd.ScalarQuantizer(0.0, 1.0, levels))
    for levels in (2, 16):
        assert vq_amd.IVFScalar4Index(np.zeros((4, 6), F), vq_amd.ScalarQuantizer(0.0, 1.0, levels)).quantizer.levels == levels
    for name in NAMES:  # the cosines included
        ix = vq_amd.IVFScalar4Index(np.zeros((4, 11), F), sq, vq_amd.Distance(name))
        assert ix.nlist == 4 and len(ix) == 0 and ix.dim == 11 and ix.words == 2 and ix.quantizer is sq and ix.distance.name() == name
        assert np.array_equal(ix.list_sizes(), np.zeros(4, np.uint64))
        assert ix.codes().shape == (0, 11) and ix.codes().dtype == np.uint8
        assert ix.packed().shape == (0, 2) and ix.packed().dtype == np.uint32
        assert ix.coarse_centroids.shape == (4, 11) and ix.list_ids.shape == (0,)


def test_python_add_and_search_checks():
    from vq_amd import DimensionMismatch, InvalidParameter

    ix = _index()
    z = np.zeros((2, 6), np.uint8)
    for add, good in ((ix.add_codes, z), (ix.add_rows, np.zeros((2, 6), F)), (ix.add_packed, np.zeros((2, 1), np.uint32))):
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
            add([0, 1], np.zeros((2, w + 1), good.dtype))
        with pytest.raises(DimensionMismatch):
            add([0, 1, 2], good)
    with pytest.raises(InvalidParameter):
        ix.add_codes([0, 1], np.zeros((2, 6), np.int32))  # codes are bytes
    with pytest.raises(InvalidParameter):
        ix.add_packed([0, 1], np.zeros((2, 1), np.int32))  # words are uint32
    with pytest.raises(InvalidParameter):
        ix.add_rows([0, 1], np.zeros((2, 6), np.int32))  # rows are floating point
    with pytest.raises(DimensionMismatch):
        ix.add(np.zeros((2, 5), F))
    assert len(ix) == 0
    assert ix.add_codes([1, 1, 4], np.full((3, 6), 15, np.uint8)).tolist() == [0, 1, 2]
    bad = np.zeros((2, 6), np.uint8)
    bad[1, 5] = 16
    with pytest.raises(InvalidParameter, match="at most 15"):
        ix.add_codes([0, 0], bad)  # a code a nibble cannot hold
    with pytest.raises(InvalidParameter, match="pad nibble"):
        ix.add_packed([0, 0], np.array([[0], [1 << 24]], np.uint32))  # dimension 6 of a row of 6
    assert len(ix) == 3 and ix.list_sizes().tolist() == [0, 2, 0, 0, 1]  # the refused adds left the index as it was
    assert ix.add_packed([0], np.array([[0x00ABCDEF]], np.uint32)).tolist() == [3]
    assert ix.add_codes([], np.zeros((0, 6), np.uint8)).tolist() == []
    assert ix.add_packed([], np.zeros((0, 1), np.uint32)).tolist() == []
    assert ix.list_sizes().tolist() == [1, 2, 0, 0, 1] and len(ix) == 4 and ix.list_ids.tolist() == [1, 1, 4, 0]
    assert ix.codes().tolist() == [[15] * 6] * 3 + [[0xF, 0xE, 0xD, 0xC, 0xB, 0xA]]
    assert ix.packed().tolist() == [[0x00FFFFFF]] * 3 + [[0x00ABCDEF]]
    q = np.zeros((2, 6), F)
    for bad_p in (0, 6, 1025):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=1, nprobe=bad_p)
        with pytest.raises(InvalidParameter):
            ix.probe(q, nprobe=bad_p)
        with pytest.raises(InvalidParameter):
            ix.search_device(0, 2, 1, 0, 0, nprobe=bad_p)
        with pytest.raises(InvalidParameter):
            ix.range_search(q, 1.0, nprobe=bad_p)
    for bad_k in (0, 5):
        with pytest.raises(InvalidParameter):
            ix.search(q, topk=bad_k, nprobe=2)
        with pytest.raises(InvalidParameter):
            ix.search_device(0, 2, bad_k, 0, 0, nprobe=2)
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
    with pytest.raises(DimensionMismatch):
        ix.search(q, topk=1, nprobe=1, allowed=np.ones(3, bool))  # a mask of another length
    with pytest.raises(DimensionMismatch):
        ix.range_search(q, 1.0, nprobe=1, allowed=np.ones(5, bool))
    i, d = ix.search(np.zeros((0, 6), F), topk=2, nprobe=2)
    assert i.shape == (0, 2) and d.shape == (0, 2) and ix.probe(np.zeros((0, 6), F), 3).shape == (0, 3)
    lims, ri, rd = ix.range_search(np.zeros((0, 6), F), 1.0, nprobe=2, allowed=np.ones(4, bool))
    assert lims.tolist() == [0] and ri.shape == (0,) and rd.shape == (0,)


@pytest.mark.parametrize("dim", [1, 7, 8, 9, 33])
def test_python_bookkeeping_and_host_side_remove(dim):
    """adds of both forms, a handle in between, and removals without a device state: the rows, the words (pack4_codes'),
    the lists and their sizes follow, and equal those of one add of the remaining rows"""
    import vq_amd

    rng = np.random.default_rng(30 + dim)
    lists = rng.integers(0, 5, 90).astype(np.uint32)
    codes = rng.integers(0, 16, (90, dim)).astype(np.uint8)
    words = vq_amd.ScalarQuantizer.pack4_codes(codes)
    assert np.array_equal(words, S4.pack4(codes))
    ix = _index(nlist=5, dim=dim)
    assert ix.add_codes(lists[:20], codes[:20]).tolist() == list(range(20))
    assert ix.add_packed(lists[20:50], words[20:50]).tolist() == list(range(20, 50))
    h = ix._handle()  # host-only: the rows move into the handle
    assert ix._host is None and h.info() == (50, 5, dim, 1, *[float(F(v)) for v in SQ[:2]], SQ[2])
    ix.add_codes(lists[50:70], codes[50:70])
    ix.add_packed(lists[70:], words[70:])
    assert np.array_equal(ix.codes(), codes) and np.array_equal(ix.packed(), words) and ix.packed().dtype == np.uint32
    assert np.array_equal(h.list_sizes(), np.bincount(lists, minlength=5)) and np.array_equal(ix.list_sizes(), h.list_sizes())
    assert h.uploads() == 0
    gone = np.zeros(90, bool)
    gone[[0, 3, 31, 32, 33, 89]] = True
    kept = ix.remove_rows(gone)
    assert np.array_equal(kept, np.flatnonzero(~gone)) and len(ix) == 84 and h.info()[0] == 84 and h.uploads() == 0
    assert np.array_equal(ix.codes(), codes[kept]) and np.array_equal(ix.packed(), words[kept]) and np.array_equal(ix.list_ids, lists[kept])
    assert np.array_equal(h.list_sizes(), np.bincount(lists[kept], minlength=5))
    ix.close()  # the words come back to the host
    assert np.array_equal(ix.packed(), words[kept])
    kept2 = ix.remove_rows([5, 5, 0])  # by ids, before a handle exists
    assert np.array_equal(ix.codes(), codes[kept][kept2]) and np.array_equal(ix.list_ids, lists[kept][kept2])
    assert ix.remove_rows(np.ones(len(ix), bool)).shape == (0,) and len(ix) == 0 and ix.packed().shape == (0, (dim + 7) // 8)
    assert ix.add_codes(lists[:3], codes[:3]).tolist() == [0, 1, 2]  # an emptied index takes rows


def test_python_save_load_round_trip(tmp_path):
    import vq_amd

    rng = np.random.default_rng(4)
    ix = _index(rng, nlist=7, dim=11, metric="cosine")
    lists = rng.integers(0, 7, 50)
    codes = rng.integers(0, 16, (50, 11)).astype(np.uint8)
    ix.add_codes(lists[:20], codes[:20])
    ix.add_packed(lists[20:], S4.pack4(codes[20:]))
    p = tmp_path / "ix.bin"
    ix.save(p)
    back = vq_amd.IVFScalar4Index.load(p)
    assert back.distance.metric == ix.distance.metric and back.nlist == 7 and len(back) == 50 and back.dim == 11
    assert (back.quantizer.min, back.quantizer.max, back.quantizer.levels) == SQ
    assert np.array_equal(back.coarse_centroids, ix.coarse_centroids)
    assert np.array_equal(back.list_ids, lists.astype(np.uint32))
    assert back.codes().dtype == np.uint8 and np.array_equal(back.codes(), codes) and np.array_equal(back.packed(), S4.pack4(codes))
    raw = p.read_bytes()
    assert raw[:8] == b"VQIVFS41" and len(raw) == 40 + 4 * (7 * 11 + 50) + 50 * 2 * 4
    assert back.add_codes([6], codes[:1]).tolist() == [50]  # a loaded index takes more rows
    ix._handle()
    ix.save(tmp_path / "h.bin")  # from the handle's rows
    assert (tmp_path / "h.bin").read_bytes() == raw


def _corrupt(tmp_path, mutate):
    import vq_amd

    ix = _index(np.random.default_rng(9), nlist=4)
    ix.add_codes([0, 3, 2], (np.arange(18, dtype=np.uint8) % 16).reshape(3, 6))
    p = tmp_path / "c.bin"
    ix.save(p)
    raw = mutate(bytearray(p.read_bytes()))
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError):
        vq_amd.IVFScalar4Index.load(p)


def _field(off, fmt, value):
    def f(raw):
        struct.pack_into(fmt, raw, off, value)
        return raw
    return f


BASE = 40 + 4 * 4 * 6  # the header and the centroids of _corrupt's file


@pytest.mark.parametrize("mutate", [
    lambda r: r[:20],                    # truncated header
    lambda r: b"VQIVFSQ1" + r[8:],       # another magic: the 8-bit index's
    lambda r: b"VQSQ4IX1" + r[8:],       # another magic: the resident 4-bit index's
    _field(8, "<I", 5),                  # metric out of range
    _field(12, "<I", 0),                 # dim 0
    _field(16, "<I", 0),                 # nlist 0
    _field(16, "<I", 70000),             # nlist too large
    _field(20, "<f", float("nan")),      # min not finite
    _field(24, "<f", -4.0),              # max below min
    _field(28, "<I", 1),                 # levels below 2
    _field(28, "<I", 17),                # levels above 16
    _field(28, "<I", 256),               # a scalar quantizer's, not a nibble's
    _field(32, "<Q", 4),                 # more rows than the file holds
    _field(32, "<Q", 1 << 40),           # n beyond 2^32
    lambda r: r[:BASE - 4],              # truncated centroids
    lambda r: r[:BASE + 8],              # truncated list ids
    lambda r: r[:-1],                    # truncated words
    lambda r: r + b"\0",                 # trailing bytes
    _field(BASE + 4, "<I", 4),           # list id 4 of nlist 4
    _field(BASE + 12 + 4, "<I", 1 << 24),  # row 1: dimension 6 of 6, a pad nibble
    _field(BASE + 12 + 8, "<I", 1 << 31),  # row 2: the last pad nibble
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
    rc = lib.load().vqhip_ivfsq4_create(sq[0], sq[1], sq[2], coarse.ctypes.data_as(lib._f32p), nlist, dim, metric, C.byref(h))
    return rc, h


def test_cabi_create_checks(lib):
    L = lib.load()
    h = C.c_void_p()
    coarse = np.zeros((4, 6), F).ctypes.data_as(lib._f32p)
    assert L.vqhip_ivfsq4_create(-3.0, 5.0, 16, None, 4, 6, 1, C.byref(h)) == lib.ERR_NULL_PTR
    assert L.vqhip_ivfsq4_create(-3.0, 5.0, 16, coarse, 4, 6, 1, None) == lib.ERR_NULL_PTR
    assert _create(lib, nlist=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, nlist=65537)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, dim=0)[0] == lib.ERR_INVALID_INPUT
    assert _create(lib, metric=7)[0] == lib.ERR_INVALID_INPUT
    step = C.c_float()
    for bad in ((float("nan"), 1.0, 4), (0.0, float("inf"), 4), (1.0, 1.0, 4), (0.0, 1.0, 1), (0.0, 1.0, 257)):
        rc = L.vqhip_sq_check(bad[0], bad[1], bad[2], C.byref(step))
        text = lib.last_error()
        assert rc != lib.OK and _create(lib, sq=bad)[0] == rc and lib.last_error() == text  # vqhip_sq_check's, unchanged
    for levels in (17, 256):  # a legal quantizer that a nibble cannot hold: behind the quantizer's own check, before the rest
        assert _create(lib, sq=(0.0, 1.0, levels), nlist=0)[0] == lib.ERR_INVALID_INPUT
        assert lib.last_error() == f"levels {levels}: a 4-bit index holds at most 16"
    assert _create(lib, sq=(float("nan"), 1.0, 17))[0] != lib.OK and "at most 16" not in lib.last_error()
    for metric in K.METRICS:  # the cosines included
        for sq in R.QUANTIZERS + [(-3e38, 3e38, 2)]:  # levels 2 and 16, and the degenerate quantizer
            rc, h = _create(lib, metric=metric, sq=sq)
            assert rc == lib.OK
            L.vqhip_ivfsq4_destroy(h)


def test_cabi_adds_info_sizes_codes_packed_and_search_bounds_are_host_only(lib):
    L = lib.load()
    rc, h = _create(lib, nlist=4, dim=6, metric=lib.COSINE)
    assert rc == lib.OK
    try:
        lid = np.array([0, 3, 3], np.uint32)
        codes = (np.arange(18, dtype=np.uint8).reshape(3, 6) + 3) % 16  # codes >= levels are legal
        words = S4.pack4(codes)
        lp, cp, wp = lid.ctypes.data_as(lib._u32p), codes.ctypes.data_as(lib._u8p), words.ctypes.data_as(lib._u32p)
        assert L.vqhip_ivfsq4_add_codes(h, lp, cp, 3) == lib.OK
        bad = np.array([0, 4, 1], np.uint32)
        bp = bad.ctypes.data_as(lib._u32p)
        rows = np.zeros((3, 6), F).ctypes.data_as(lib._f32p)
        for rc in (L.vqhip_ivfsq4_add_codes(h, bp, cp, 3), L.vqhip_ivfsq4_add_packed(h, bp, wp, 3),
                   L.vqhip_ivfsq4_add_rows(h, bp, rows, 3)):  # (add_rows: before the device)
            assert rc == lib.ERR_INVALID_INPUT and "list id 4" in lib.last_error()
        c16 = codes.copy()
        c16[2, 5] = 16
        assert L.vqhip_ivfsq4_add_codes(h, lp, c16.ctypes.data_as(lib._u8p), 3) == lib.ERR_INVALID_INPUT
        assert "row 2 holds code 16" in lib.last_error()
        c16[0, 0] = 99
        assert L.vqhip_ivfsq4_add_codes(h, bp, c16.ctypes.data_as(lib._u8p), 3) == lib.ERR_INVALID_INPUT
        assert "list id 4" in lib.last_error()  # the list ids come first
        wpad = words.copy()
        wpad[1, 0] |= 1 << 28
        assert L.vqhip_ivfsq4_add_packed(h, lp, wpad.ctypes.data_as(lib._u32p), 3) == lib.ERR_INVALID_INPUT
        assert "row 1 has a pad nibble set" in lib.last_error()
        n = C.c_uint64()
        assert L.vqhip_ivfsq4_info(h, C.byref(n), None, None, None, None, None, None) == lib.OK and n.value == 3  # n unchanged
        assert L.vqhip_ivfsq4_add_packed(h, lp, wp, 3) == lib.OK
        for add, p in ((L.vqhip_ivfsq4_add_codes, cp), (L.vqhip_ivfsq4_add_packed, wp), (L.vqhip_ivfsq4_add_rows, rows)):
            assert add(h, None, None, 0) == lib.OK
            assert add(h, None, p, 3) == lib.ERR_NULL_PTR and add(h, lp, None, 3) == lib.ERR_NULL_PTR
            assert add(None, lp, p, 3) == lib.ERR_NULL_PTR
        nlist, dim, metric = C.c_uint32(), C.c_uint32(), C.c_int()
        mn, mx, levels = C.c_float(), C.c_float(), C.c_uint32()
        assert L.vqhip_ivfsq4_info(h, C.byref(n), C.byref(nlist), C.byref(dim), C.byref(metric), C.byref(mn), C.byref(mx),
                                   C.byref(levels)) == lib.OK
        assert (n.value, nlist.value, dim.value, metric.value, mn.value, mx.value, levels.value) == (6, 4, 6, lib.COSINE, -3.5, 200.0, 5)
        sizes = np.zeros(4, np.uint64)
        assert L.vqhip_ivfsq4_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK
        assert sizes.tolist() == [2, 0, 0, 4]
        out = np.zeros((6, 6), np.uint8)
        assert L.vqhip_ivfsq4_codes(h, out.ctypes.data_as(lib._u8p)) == lib.OK and np.array_equal(out, np.concatenate([codes, codes]))
        wout = np.zeros((6, 1), np.uint32)
        assert L.vqhip_ivfsq4_packed(h, wout.ctypes.data_as(lib._u32p)) == lib.OK and np.array_equal(wout, np.concatenate([words, words]))
        q = np.zeros((2, 6), F)
        idx = np.zeros((2, 8), np.uint32)
        dist = np.zeros((2, 8), F)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        mask = np.full(1, 0xFFFFFFFF, np.uint32).ctypes.data_as(lib._u32p)
        for nprobe, topk in ((0, 1), (5, 1), (1, 0), (1, 7)):  # nprobe in [1, nlist], topk in [1, n]
            assert L.vqhip_ivfsq4_search(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfsq4_search_device(h, qp, 2, nprobe, topk, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfsq4_search_masked(h, qp, 2, nprobe, topk, mask, ip, dp) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfsq4_search_masked_device(h, qp, 2, nprobe, topk, mask, ip, dp) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq4_probe(h, qp, 2, 0, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq4_probe(h, qp, 2, 5, ip) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq4_search(h, qp, 0, 2, 2, ip, dp) == lib.OK  # nq = 0
        radii = np.ones(2, F).ctypes.data_as(lib._f32p)
        r = C.c_void_p()
        for nprobe in (0, 5):
            assert L.vqhip_ivfsq4_range_search(h, qp, 2, nprobe, radii, 10, C.byref(r)) == lib.ERR_INVALID_INPUT
            assert L.vqhip_ivfsq4_range_search_masked(h, qp, 2, nprobe, radii, 10, mask, C.byref(r)) == lib.ERR_INVALID_INPUT
        assert L.vqhip_ivfsq4_range_search(h, qp, 2, 1, radii, 0, C.byref(r)) == lib.ERR_INVALID_INPUT  # max_results
        odd = C.c_void_p(mask_addr := np.zeros(3, np.uint32).ctypes.data + 1)
        assert mask_addr % 4 == 1
        assert L.vqhip_ivfsq4_search_masked_device(h, qp, 2, 1, 1, C.cast(odd, lib._u32p), ip, dp) == lib.ERR_INVALID_INPUT
        # a removal without a device state is the host's
        rm = np.array([0b100001], np.uint32)
        gone = C.c_uint64()
        assert L.vqhip_ivfsq4_remove(h, rm.ctypes.data_as(lib._u32p), C.byref(gone)) == lib.OK and gone.value == 2
        wout = np.zeros((4, 1), np.uint32)
        assert L.vqhip_ivfsq4_packed(h, wout.ctypes.data_as(lib._u32p)) == lib.OK
        assert np.array_equal(wout, np.concatenate([words, words])[1:5])
        assert L.vqhip_ivfsq4_list_sizes(h, sizes.ctypes.data_as(lib._u64p)) == lib.OK and sizes.tolist() == [1, 0, 0, 3]
        up = C.c_uint64(7)
        assert L.vqhip_ivfsq4_uploads(h, C.byref(up)) == lib.OK and up.value == 0
    finally:
        L.vqhip_ivfsq4_destroy(h)


def test_cabi_null_pointers_from_each_entry_point(lib):
    L = lib.load()
    rc, h = _create(lib)
    assert rc == lib.OK
    try:
        lid = np.zeros(1, np.uint32)
        assert L.vqhip_ivfsq4_add_codes(h, lid.ctypes.data_as(lib._u32p), np.zeros((1, 6), np.uint8).ctypes.data_as(lib._u8p), 1) == lib.OK
        q = np.zeros((1, 6), F)
        idx, dist, radii = np.zeros(1, np.uint32), np.zeros(1, F), np.ones(1, F)
        mask = np.ones(1, np.uint32)
        qp, ip, dp = q.ctypes.data_as(lib._f32p), idx.ctypes.data_as(lib._u32p), dist.ctypes.data_as(lib._f32p)
        rp, mp = radii.ctypes.data_as(lib._f32p), mask.ctypes.data_as(lib._u32p)
        qv, iv, dv, mv = (C.c_void_p(a.ctypes.data) for a in (q, idx, dist, mask))
        r = C.c_void_p()
        out = C.byref(r)
        n = C.c_uint64()
        calls = {
            "info": [(None, None, None, None, None, None, None, None)],
            "list_sizes": [(None, np.zeros(4, np.uint64).ctypes.data_as(lib._u64p)), (h, None)],
            "codes": [(None, np.zeros(6, np.uint8).ctypes.data_as(lib._u8p)), (h, None)],
            "packed": [(None, ip), (h, None)],
            "probe": [(None, qp, 1, 1, ip), (h, None, 1, 1, ip), (h, qp, 1, 1, None)],
            "search": [(None, qp, 1, 1, 1, ip, dp), (h, None, 1, 1, 1, ip, dp), (h, qp, 1, 1, 1, None, dp), (h, qp, 1, 1, 1, ip, None)],
            "search_device": [(None, qv, 1, 1, 1, iv, dv), (h, None, 1, 1, 1, iv, dv), (h, qv, 1, 1, 1, None, dv),
                              (h, qv, 1, 1, 1, iv, None)],
            "search_masked": [(None, qp, 1, 1, 1, mp, ip, dp), (h, None, 1, 1, 1, mp, ip, dp), (h, qp, 1, 1, 1, None, ip, dp),
                              (h, qp, 1, 1, 1, mp, None, dp), (h, qp, 1, 1, 1, mp, ip, None)],
            "search_masked_device": [(None, qv, 1, 1, 1, mv, iv, dv), (h, None, 1, 1, 1, mv, iv, dv), (h, qv, 1, 1, 1, None, iv, dv),
                                     (h, qv, 1, 1, 1, mv, None, dv), (h, qv, 1, 1, 1, mv, iv, None)],
            "range_search": [(None, qp, 1, 1, rp, 10, out), (h, None, 1, 1, rp, 10, out), (h, qp, 1, 1, None, 10, out),
                             (h, qp, 1, 1, rp, 10, None)],
            "range_search_device": [(None, qv, 1, 1, rp, 10, out), (h, None, 1, 1, rp, 10, out), (h, qv, 1, 1, None, 10, out),
                                    (h, qv, 1, 1, rp, 10, None)],
            "range_search_masked": [(None, qp, 1, 1, rp, 10, mp, out), (h, None, 1, 1, rp, 10, mp, out), (h, qp, 1, 1, None, 10, mp, out),
                                    (h, qp, 1, 1, rp, 10, None, out), (h, qp, 1, 1, rp, 10, mp, None)],
            "range_search_masked_device": [(None, qv, 1, 1, rp, 10, mv, out), (h, None, 1, 1, rp, 10, mv, out),
                                           (h, qv, 1, 1, None, 10, mv, out), (h, qv, 1, 1, rp, 10, None, out),
                                           (h, qv, 1, 1, rp, 10, mv, None)],
            "remove": [(None, mp, C.byref(n)), (h, None, C.byref(n)), (h, mp, None)],
            "uploads": [(None, C.byref(n)), (h, None)],
        }
        for name, arg_sets in calls.items():
            fn = getattr(L, f"vqhip_ivfsq4_{name}")
            for args in arg_sets:
                assert fn(*args) == lib.ERR_NULL_PTR, (name, args)
        assert L.vqhip_ivfsq4_destroy(None) == lib.OK
        assert L.vqhip_ivfsq4_info(h, C.byref(n), None, None, None, None, None, None) == lib.OK and n.value == 1  # nothing changed
    finally:
        L.vqhip_ivfsq4_destroy(h)


def test_several_adds_equal_one_add(lib):
    rng = np.random.default_rng(21)
    coarse, lists, codes, _ = _case(rng, 200, 6, 13)
    words = S4.pack4(codes)
    one = lib.IVFSQ4(coarse, *SQ, lib.EUCLIDEAN)
    many = lib.IVFSQ4(coarse, *SQ, lib.EUCLIDEAN)
    a, b = _index(nlist=6, dim=13), _index(nlist=6, dim=13)
    try:
        one.add_codes(lists, codes)
        a.add_codes(lists, codes)
        for j, part in enumerate(np.array_split(np.arange(200), 7)):
            if j % 2:
                many.add_packed(lists[part], words[part])
                b.add_packed(lists[part], words[part])
            else:
                many.add_codes(lists[part], codes[part])
                b.add_codes(lists[part], codes[part])
        assert one.info() == many.info() == (200, 6, 13, lib.EUCLIDEAN, -3.5, 200.0, 5)
        assert np.array_equal(one.list_sizes(), many.list_sizes())
        assert np.array_equal(one.list_sizes(), np.bincount(lists, minlength=6))
        assert np.array_equal(one.codes(), codes) and np.array_equal(many.codes(), codes)
        assert np.array_equal(one.packed(), words) and np.array_equal(many.packed(), words)
        assert np.array_equal(a.list_ids, b.list_ids) and np.array_equal(a.list_ids, lists)
        assert np.array_equal(a.packed(), b.packed()) and np.array_equal(a.codes(), codes)
        assert np.array_equal(a.list_sizes(), one.list_sizes())
    finally:
        one.close()
        many.close()
