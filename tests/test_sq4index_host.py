"""CPU checks of the 4-bit scalar index (vq_amd.Scalar4Index, include/vqhip.h vqhip_sq4index_*): every argument error,
raised before any device is touched and with the index unchanged; the limit of 16 levels; a code above 15 and a set pad
nibble refused in the package and at the C ABI's host forms; the 4-bit layout of ScalarQuantizer.pack4_codes /
unpack4_batch on hand-written words; the file format and every malformed file; VQHIP_ERR_NULL_PTR from the new entry
points and the C ABI's checks in order; the exports; and the checks of a search reranked through an index of another
shape."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_knn as K
import ref_sq4 as R
import vq_amd
from vq_amd import BinaryIndex, Distance, Scalar4Index, ScalarQuantizer, _lib
from vq_amd._resident_common import ExactResidentIndex
from vq_amd.errors import DimensionMismatch, EmptyInput, InvalidData, InvalidParameter

F = np.float32
HEAD = "<8sQIIffI"  # magic, n, d, metric, min, max, levels
SQZ = ScalarQuantizer(-1.0, 1.0, 16)
ENTRY_POINTS = ("create", "create_device", "destroy", "info", "packed", "search", "search_device", "search_masked",
                "search_masked_device", "rerank", "range_search", "range_search_device", "range_search_masked",
                "range_search_masked_device", "add", "add_device", "remove", "remove_device")


def _X(n=20, d=40):
    return np.random.default_rng(0).standard_normal((n, d)).astype(F)


def _C(n=20, d=40):
    return np.random.default_rng(1).integers(0, 16, (n, d), dtype=np.uint8)


def test_exports():
    assert "Scalar4Index" in vq_amd.__all__ and vq_amd.Scalar4Index is Scalar4Index
    assert issubclass(Scalar4Index, ExactResidentIndex)
    for name in ENTRY_POINTS:
        assert f"vqhip_sq4index_{name}" in _lib.SIGNATURES
        assert hasattr(_lib.load(), f"vqhip_sq4index_{name}")
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("vqhip_sq4index_")) == sorted(f"vqhip_sq4index_{n}" for n in ENTRY_POINTS)
    assert (_lib.SQ4_F32, _lib.SQ4_U8, _lib.SQ4_PACKED) == (0, 1, 2) and issubclass(_lib.SQ4Index, _lib._ResidentExactHandle)
    for name in ("search", "search_device", "range_search", "range_search_device", "rerank", "add", "add_device", "add_codes",
                 "add_packed", "add_codes_device", "add_packed_device", "remove_rows", "remove_rows_device", "packed", "codes",
                 "save", "load", "from_codes", "from_packed", "quantizer"):
        assert hasattr(Scalar4Index, name)
    assert hasattr(ScalarQuantizer, "pack4_codes") and hasattr(ScalarQuantizer, "unpack4_batch")


def test_defaults_accessors_and_repr():
    ix = Scalar4Index(_X(), SQZ)
    assert len(ix) == 20 and ix.dim == 40
    assert ix.distance == Distance.euclidean() and ix.quantizer is SQZ
    assert repr(ix) == ("Scalar4Index(n=20, dim=40, quantizer=ScalarQuantizer(min=-1, max=1, levels=16), "
                        "distance=Distance('euclidean'))")
    assert ix._ix is None


def test_levels_above_16_are_refused_2_and_16_accepted():
    X, codes = _X(), _C()
    for levels in (17, 256):
        q = ScalarQuantizer(0.0, 1.0, levels)
        for make in (lambda: Scalar4Index(X, q), lambda: Scalar4Index.from_codes(codes, q),
                     lambda: Scalar4Index.from_packed(R.pack4(codes), 40, q)):
            with pytest.raises(InvalidParameter, match=f"levels {levels}: a 4-bit index holds at most 16"):
                make()
    for levels in (2, 16):
        q = ScalarQuantizer(0.0, 1.0, levels)
        ix = Scalar4Index.from_codes(codes, q)  # codes >= levels are legal: every nibble value is
        assert ix.quantizer.levels == levels and ix._ix is None
        assert np.array_equal(ix.codes(), codes)


def test_every_metric_is_accepted():
    for name in ("squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"):
        ix = Scalar4Index(_X(), SQZ, Distance(name))
        assert ix.distance == Distance(name) and ix._ix is None


def test_constructor_checks_raise_first():
    X = _X()
    with pytest.raises(InvalidParameter, match="dimension"):
        Scalar4Index(np.zeros((2, 0), F), SQZ)
    with pytest.raises(EmptyInput):
        Scalar4Index(np.zeros((0, 4), F), SQZ)
    with pytest.raises(ValueError):
        Scalar4Index(np.zeros(4, F), SQZ)
    with pytest.raises(InvalidParameter, match="rows"):
        Scalar4Index(X.astype(np.float64), SQZ)
    with pytest.raises(InvalidParameter, match="quantizer"):
        Scalar4Index(X, "sq")
    with pytest.raises(InvalidParameter, match="quantizer"):
        Scalar4Index(X, vq_amd.BinaryQuantizer(0.0))
    with pytest.raises(InvalidParameter, match="distance"):
        Scalar4Index(X, SQZ, distance="cosine")
    with pytest.raises(InvalidParameter, match="codes"):
        Scalar4Index.from_codes(X, SQZ)
    with pytest.raises(InvalidParameter, match="words"):
        Scalar4Index.from_packed(np.zeros((2, 5), np.int32), 40, SQZ)
    with pytest.raises(InvalidParameter, match="dim"):
        Scalar4Index.from_packed(np.zeros((2, 5), np.uint32), 40.5, SQZ)
    with pytest.raises(InvalidParameter, match="dim"):
        Scalar4Index.from_packed(np.zeros((2, 0), np.uint32), 0, SQZ)
    with pytest.raises(ValueError):
        Scalar4Index.from_packed(np.zeros(5, np.uint32), 40, SQZ)


def test_a_code_of_16_and_a_pad_nibble_are_refused_in_the_package():
    codes = _C()
    bad = codes.copy()
    bad[7, 39] = 16
    with pytest.raises(InvalidParameter, match="at most 15, got 16"):
        Scalar4Index.from_codes(bad, SQZ)
    with pytest.raises(InvalidParameter, match="at most 15"):
        ScalarQuantizer.pack4_codes(bad)
    with pytest.raises(DimensionMismatch):
        Scalar4Index.from_packed(np.zeros((2, 6), np.uint32), 40, SQZ)
    with pytest.raises(DimensionMismatch):
        Scalar4Index.from_packed(np.zeros((2, 4), np.uint32), 33, SQZ)
    w = np.zeros((2, 5), np.uint32)
    w[1, 4] = 1 << 4  # dimension 33 of 33: the first pad nibble
    with pytest.raises(InvalidParameter, match="pad nibble"):
        Scalar4Index.from_packed(w, 33, SQZ)
    w[1, 4] = 15  # dimension 32: the last legal nibble
    ix = Scalar4Index.from_packed(w, 33, SQZ)
    assert np.array_equal(ix.packed(), w) and ix.codes()[1, 32] == 15 and ix._ix is None
    Scalar4Index.from_packed(np.full((2, 5), 0xFFFFFFFF, np.uint32), 40, SQZ)  # no pad nibbles at a whole word
    ix = Scalar4Index.from_codes(codes, SQZ)
    with pytest.raises(InvalidParameter, match="at most 15"):
        ix.add_codes(bad)
    with pytest.raises(InvalidParameter, match="pad nibble"):
        Scalar4Index.from_packed(np.zeros((2, 5), np.uint32), 33, SQZ).add_packed(np.full((1, 5), 1 << 31, np.uint32))
    assert ix._ix is None and len(ix) == 20


def test_pack4_unpack4_layout_and_round_trip():
    """the layout on hand-written words: dimension t in bits 4 (t % 8) .. + 3 of word t // 8, low nibble first"""
    codes = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
                      [15, 0, 0, 0, 0, 0, 0, 15, 0, 0, 12]], np.uint8)
    words = np.array([[0x87654321, 0x00000BA9], [0xF000000F, 0x00000C00]], np.uint32)
    assert np.array_equal(ScalarQuantizer.pack4_codes(codes), words)
    assert np.array_equal(SQZ.pack4_codes(codes), words)
    assert np.array_equal(ScalarQuantizer.unpack4_batch(words, 11), codes)
    assert np.array_equal(R.pack4(codes), words) and np.array_equal(R.unpack4(words, 11), codes)
    dirty = words | np.array([[0, 0xFFFFF000]], np.uint32)  # the pad nibbles are not read
    assert np.array_equal(ScalarQuantizer.unpack4_batch(dirty, 11), codes)
    rng = np.random.default_rng(4)
    for d in (1, 7, 8, 9, 31, 32, 33, 40, 100):
        c = rng.integers(0, 16, (13, d), dtype=np.uint8)
        w = ScalarQuantizer.pack4_codes(c)
        assert w.dtype == np.uint32 and w.shape == (13, (d + 7) // 8) and np.array_equal(w, R.pack4(c))
        assert np.array_equal(ScalarQuantizer.unpack4_batch(w, d), c)
        if d % 8:
            assert not (w[:, -1] >> np.uint32(4 * (d % 8))).any()
    assert ScalarQuantizer.pack4_codes(np.zeros((0, 9), np.uint8)).shape == (0, 2)
    with pytest.raises(InvalidParameter, match="codes"):
        ScalarQuantizer.pack4_codes(codes.astype(np.int32))
    with pytest.raises(ValueError):
        ScalarQuantizer.pack4_codes(codes[0])
    with pytest.raises(InvalidParameter, match="words"):
        ScalarQuantizer.unpack4_batch(words.astype(np.int64), 11)
    with pytest.raises(DimensionMismatch):
        ScalarQuantizer.unpack4_batch(words, 17)
    with pytest.raises(InvalidParameter, match="dim"):
        ScalarQuantizer.unpack4_batch(np.zeros((2, 0), np.uint32), 0)


def test_the_statement_is_ref_knn_over_the_decoded_rows():
    """tests/ref_sq4.py computes every query at once; per query it is tests/ref_knn.py's distances, bit for bit"""
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 16, (37, 19), dtype=np.uint8)
    Q = rng.standard_normal((4, 19)).astype(F)
    Q[1, 3] = np.nan
    for quant in R.QUANTIZERS:
        V = R.decode(R.pack4(codes), 19, *quant)
        step = R.step_of(*quant)
        assert V[0, 0] == F(quant[0]) + F(codes[0, 0]) * step
        for metric in K.METRICS:
            D = R.matrix_over(metric, Q, V)
            for j in range(4):
                assert np.array_equal(D[j].view(np.uint32), K.distances(metric, Q[j], V).astype(F).view(np.uint32))


def test_call_checks_leave_the_index_unchanged():
    X = _X()
    ix = Scalar4Index(X, SQZ, Distance.cosine())
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 0)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 21)
    with pytest.raises(InvalidParameter, match="topk"):
        Scalar4Index(np.zeros((2000, 4), F), SQZ).search(np.zeros((1, 4), F), 1025)
    with pytest.raises(DimensionMismatch):
        ix.search(X[:2, :39], 5)
    with pytest.raises(InvalidParameter, match="allowed"):
        ix.search(X[:2], 5, allowed=np.zeros(20, np.int32))
    with pytest.raises(DimensionMismatch):
        ix.search(X[:2], 5, allowed=np.zeros(19, bool))
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search_device(0, 1, 0, 0, 0)
    with pytest.raises(InvalidParameter, match="nq"):
        ix.search_device(0, -1, 1, 0, 0)
    with pytest.raises(InvalidParameter, match="radius"):
        ix.range_search(X[:2], float("nan"))
    with pytest.raises(DimensionMismatch):
        ix.range_search(X[:2], [1.0, 2.0, 3.0])
    with pytest.raises(InvalidParameter, match="max_results"):
        ix.range_search(X[:2], 1.0, max_results=0)
    with pytest.raises(InvalidParameter, match="radius"):
        ix.range_search_device(0, 2, "far")
    with pytest.raises(InvalidParameter, match="candidates"):
        ix.rerank(X[:2], np.zeros((2, 4097), np.int64), 1)
    with pytest.raises(InvalidParameter, match="outside"):
        ix.rerank(X[:2], np.array([[0, 20], [1, 2]]), 1)
    with pytest.raises(InvalidParameter, match="distinct"):
        ix.rerank(X[:2], np.array([[0, 0], [1, 2]]), 1)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.rerank(X[:2], np.array([[0, 3], [1, 2]]), 3)
    with pytest.raises(InvalidParameter, match="rows"):
        ix.add(X.astype(np.float64))
    with pytest.raises(DimensionMismatch):
        ix.add(X[:, :39])
    with pytest.raises(InvalidParameter, match="codes"):
        ix.add_codes(X)
    with pytest.raises(DimensionMismatch):
        ix.add_codes(_C(3, 39))
    with pytest.raises(InvalidParameter, match="words"):
        ix.add_packed(np.zeros((2, 5), np.int32))
    with pytest.raises(DimensionMismatch):
        ix.add_packed(np.zeros((2, 6), np.uint32))
    with pytest.raises(InvalidParameter, match="n"):
        ix.add_packed_device(0, -1)
    with pytest.raises(InvalidParameter, match="n"):
        ix.add_codes_device(0, 1.5)
    with pytest.raises(InvalidParameter, match="no row"):
        ix.remove_rows(np.ones(20, bool))
    with pytest.raises(DimensionMismatch):
        ix.remove_rows(np.ones(19, bool))
    with pytest.raises(InvalidParameter, match="row id"):
        ix.remove_rows(np.array([20]))
    # calls that do nothing need no device either
    assert ix.add(np.zeros((0, 40), F)).size == 0 and ix.add_packed(np.zeros((0, 5), np.uint32)).size == 0
    assert ix.add_codes(np.zeros((0, 40), np.uint8)).size == 0 and ix.add_codes_device(0, 0).size == 0
    assert np.array_equal(ix.remove_rows(np.zeros(20, bool)), np.arange(20, dtype=np.uint32))
    idx, dist = ix.search(np.zeros((0, 40), F), 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3)
    assert ix.range_search(np.zeros((0, 40), F), 1.0)[0].tolist() == [0]
    assert ix._ix is None and len(ix) == 20 and ix.dim == 40  # nothing reached the device, nothing changed


def test_a_reranker_of_another_n_or_dim_is_refused():
    X = _X()
    b = BinaryIndex(X)
    with pytest.raises(DimensionMismatch):
        b.search(X[:2], 5, rerank=Scalar4Index(X[:10], SQZ))
    with pytest.raises(DimensionMismatch):
        b.search(X[:2], 5, rerank=Scalar4Index(X[:, :39], SQZ))
    with pytest.raises(InvalidParameter, match="candidates"):
        b.search(X[:2], 5, rerank=Scalar4Index(X, SQZ), candidates=4)
    assert b._ix is None


def test_save_load_round_trip_without_device(tmp_path):
    codes = _C(33, 70)
    words = R.pack4(codes)
    q = ScalarQuantizer(-3.5, 200.0, 5)
    for ix in (Scalar4Index.from_codes(codes, q, Distance.cosine()), Scalar4Index.from_packed(words, 70, q, Distance.cosine())):
        p = tmp_path / "a.bin"
        ix.save(p)
        raw = p.read_bytes()
        assert raw[:36] == struct.pack(HEAD, b"VQSQ4IX1", 33, 70, 3, -3.5, 200.0, 5)
        assert raw[36:] == words.astype("<u4").tobytes()
        back = Scalar4Index.load(p)
        assert len(back) == 33 and back.dim == 70 and back.distance == Distance.cosine()
        assert repr(back.quantizer) == repr(q)
        assert np.array_equal(back.packed(), words) and np.array_equal(back.codes(), codes)
        assert back._ix is None and ix._ix is None


def test_load_rejects_bad_files(tmp_path):
    words = R.pack4(_C(3, 41))
    body = words.astype("<u4").tobytes()
    good = struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 3, -1.0, 1.0, 16) + body
    p = tmp_path / "a.bin"

    def load(raw):
        p.write_bytes(raw)
        return Scalar4Index.load(p)

    load(good)
    with pytest.raises(InvalidData):
        load(b"VQSQIDX1" + good[8:])  # the 8-bit index's file is not this one
    with pytest.raises(InvalidData):
        load(good[:20])
    with pytest.raises(InvalidData):
        load(b"")
    with pytest.raises(InvalidData):
        load(good[:-1])
    with pytest.raises(InvalidData):
        load(good + b"\0")
    bad_pad = words.copy()
    bad_pad[1, 5] |= 1 << 4
    with pytest.raises(InvalidData, match="pad nibble"):
        load(good[:36] + bad_pad.astype("<u4").tobytes())
    with pytest.raises(InvalidParameter, match="distance"):
        load(struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 5, -1.0, 1.0, 16) + body)
    with pytest.raises(InvalidParameter, match="dim"):
        load(struct.pack(HEAD, b"VQSQ4IX1", 3, 0, 3, -1.0, 1.0, 16) + body)
    with pytest.raises(InvalidData):
        load(struct.pack(HEAD, b"VQSQ4IX1", 0, 41, 3, -1.0, 1.0, 16))
    with pytest.raises(InvalidData):
        load(struct.pack(HEAD, b"VQSQ4IX1", 1 << 32, 41, 3, -1.0, 1.0, 16) + body)
    for levels in (17, 256):
        with pytest.raises(InvalidParameter, match="at most 16"):
            load(struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 3, -1.0, 1.0, levels) + body)
    for levels in (0, 1, 257):
        with pytest.raises(InvalidParameter, match="levels"):
            load(struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 3, -1.0, 1.0, levels) + body)
    with pytest.raises(InvalidParameter, match="max"):
        load(struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 3, 1.0, 1.0, 16) + body)
    with pytest.raises(InvalidParameter, match="min"):
        load(struct.pack(HEAD, b"VQSQ4IX1", 3, 41, 3, float("nan"), 1.0, 16) + body)


def test_null_pointers_are_refused_by_every_entry_point():
    """VQHIP_ERR_NULL_PTR from each new entry point (vqhip_sq4index_destroy takes NULL like free); no device needed"""
    lib = _lib.load()
    h = C.c_void_p()
    buf = np.zeros(64, np.uint32)
    f32 = np.zeros(64, F)
    src, u32p, f32p = buf.ctypes.data_as(C.c_void_p), _lib.ptr(buf, C.POINTER(C.c_uint32)), _lib.ptr(f32, C.POINTER(C.c_float))
    removed, n = C.c_uint64(), C.c_uint64()
    NULL = _lib.ERR_NULL_PTR
    for create in (lib.vqhip_sq4index_create, lib.vqhip_sq4index_create_device):
        assert create(-1.0, 1.0, 16, src, _lib.SQ4_PACKED, 2, 32, _lib.COSINE, None) == NULL
        assert create(-1.0, 1.0, 16, None, _lib.SQ4_PACKED, 2, 32, _lib.COSINE, C.byref(h)) == NULL and not h.value
    assert lib.vqhip_sq4index_destroy(None) == _lib.OK
    assert lib.vqhip_sq4index_info(None, C.byref(n), None, None, None, None, None) == NULL
    assert lib.vqhip_sq4index_packed(None, u32p) == NULL
    assert lib.vqhip_sq4index_search(None, f32p, 1, 1, u32p, f32p) == NULL
    assert lib.vqhip_sq4index_search_device(None, src, 1, 1, src, src) == NULL
    assert lib.vqhip_sq4index_search_masked(None, f32p, 1, 1, u32p, u32p, f32p) == NULL
    assert lib.vqhip_sq4index_search_masked_device(None, src, 1, 1, src, src, src) == NULL
    assert lib.vqhip_sq4index_search_masked_device(None, src, 1, 1, None, src, src) == NULL
    assert lib.vqhip_sq4index_rerank(None, f32p, 1, u32p, 1, 1, u32p, f32p) == NULL
    for fn, q in ((lib.vqhip_sq4index_range_search, f32p), (lib.vqhip_sq4index_range_search_device, src)):
        assert fn(None, q, 1, f32p, 1, C.byref(h)) == NULL and not h.value
        assert fn(None, q, 1, f32p, 1, None) == NULL
        assert fn(None, q, 1, None, 1, C.byref(h)) == NULL
    for fn, q, m in ((lib.vqhip_sq4index_range_search_masked, f32p, u32p), (lib.vqhip_sq4index_range_search_masked_device, src, src)):
        assert fn(None, q, 1, f32p, 1, m, C.byref(h)) == NULL and not h.value
        assert fn(None, q, 1, f32p, 1, None, C.byref(h)) == NULL
    assert lib.vqhip_sq4index_add(None, src, _lib.SQ4_PACKED, 1) == NULL
    assert lib.vqhip_sq4index_add_device(None, src, _lib.SQ4_PACKED, 1) == NULL
    assert lib.vqhip_sq4index_remove(None, u32p, C.byref(removed)) == NULL
    assert lib.vqhip_sq4index_remove_device(None, src, C.byref(removed)) == NULL


def test_create_checks_come_before_the_device_and_in_order():
    """the C ABI's own checks, in the order of vqhip_sqindex_create (out, the quantizer, levels <= 16, the source
    pointer, d, n, the metric, then the kind and the source) and with its texts"""
    lib = _lib.load()
    h = C.c_void_p()
    words = np.zeros((2, 5), np.uint32)
    codes = np.zeros((2, 33), np.uint8)
    src = words.ctypes.data_as(C.c_void_p)

    def create(mn=-1.0, mx=1.0, levels=16, kind=_lib.SQ4_PACKED, n=2, d=33, metric=_lib.COSINE, fn=lib.vqhip_sq4index_create, s=src):
        rc = fn(mn, mx, levels, s, kind, n, d, metric, C.byref(h))
        return rc, _lib.last_error()

    INVALID = _lib.ERR_INVALID_INPUT
    rc, msg = create(mx=-1.0, levels=17, d=0)
    assert rc == INVALID and "'max'" in msg  # the quantizer first
    rc, msg = create(levels=1, d=0)
    assert rc == INVALID and "'levels'" in msg
    for levels in (17, 256):
        rc, msg = create(levels=levels, d=0, s=None)
        assert rc == INVALID and f"levels {levels}: a 4-bit index holds at most 16" in msg  # before the source pointer and d
    rc, _ = create(s=None, d=0)
    assert rc == _lib.ERR_NULL_PTR
    rc, msg = create(d=0, n=0)
    assert rc == INVALID and "d must be at least 1" in msg
    for n in (0, 1 << 32):
        rc, msg = create(n=n, metric=9)
        assert rc == INVALID and "n must be" in msg
    for metric in (-1, 5):
        rc, msg = create(metric=metric, kind=3)
        assert rc == INVALID and "metric" in msg
    rc, msg = create(kind=3)
    assert rc == INVALID and "source kind" in msg
    words[1, 4] = 1 << 4
    rc, msg = create()
    assert rc == INVALID and "row 1 has a pad nibble set" in msg
    words[1, 4] = 0
    codes[1, 32] = 16
    rc, msg = create(kind=_lib.SQ4_U8, s=codes.ctypes.data_as(C.c_void_p))
    assert rc == INVALID and "row 1 holds code 16" in msg
    codes[1, 32] = 15
    odd = C.c_void_p(words.ctypes.data + 2)
    rc, msg = create(fn=lib.vqhip_sq4index_create_device, s=odd)
    assert rc == INVALID and "words are not 4-byte aligned" in msg
    rc, msg = create(kind=_lib.SQ4_F32, fn=lib.vqhip_sq4index_create_device, s=odd)
    assert rc == INVALID and "rows are not 4-byte aligned" in msg
    assert not h.value
    # every argument check passed: a machine without a GPU ends at the device, one with a GPU creates the index
    for levels, kind, s in ((2, _lib.SQ4_PACKED, src), (16, _lib.SQ4_U8, codes.ctypes.data_as(C.c_void_p))):
        rc, _ = create(levels=levels, kind=kind, s=s)
        assert rc in (_lib.OK, _lib.ERR_NO_DEVICE)
        if rc == _lib.OK:
            assert lib.vqhip_sq4index_destroy(h) == _lib.OK
            h.value = None
