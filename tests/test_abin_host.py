"""CPU checks of the asymmetric binary index (vq_amd.AsymmetricBinaryIndex, include/vqhip.h vqhip_abin_*): every argument
error, raised before any device is touched and with the index unchanged; cosine accepted where BinaryIndex refuses it; the
pad-bit and width checks of packed rows; the file format and every malformed file; VQHIP_ERR_NULL_PTR from the new entry
points; the exports; and the checks of a Hamming search reranked through an index of another shape."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_abin as R
import vq_amd
from vq_amd import AsymmetricBinaryIndex, BinaryIndex, BinaryQuantizer, Distance, FlatIndex, _lib
from vq_amd._resident_common import ExactResidentIndex
from vq_amd.errors import DimensionMismatch, EmptyInput, InvalidData, InvalidParameter

F = np.float32
HEAD = "<8sQIIfII"  # magic, n, d, metric, threshold, low, high


def _X(n=20, d=40):
    return np.random.default_rng(0).standard_normal((n, d)).astype(F)


def test_exports():
    assert "AsymmetricBinaryIndex" in vq_amd.__all__ and vq_amd.AsymmetricBinaryIndex is AsymmetricBinaryIndex
    assert issubclass(AsymmetricBinaryIndex, ExactResidentIndex)
    for name in ("create", "create_device", "destroy", "info", "packed", "search", "search_device", "search_masked",
                 "search_masked_device", "rerank", "range_search", "range_search_device", "range_search_masked",
                 "range_search_masked_device", "add", "add_device", "remove", "remove_device"):
        assert f"vqhip_abin_{name}" in _lib.SIGNATURES
        assert hasattr(_lib.load(), f"vqhip_abin_{name}")
    for name in ("search", "search_device", "range_search", "range_search_device", "rerank", "add", "add_device", "add_codes",
                 "add_packed", "add_packed_device", "remove_rows", "remove_rows_device", "packed", "save", "load", "from_codes",
                 "from_packed", "quantizer"):
        assert hasattr(AsymmetricBinaryIndex, name)


def test_defaults_accessors_and_repr():
    ix = AsymmetricBinaryIndex(_X())
    assert len(ix) == 20 and ix.dim == 40
    assert ix.distance == Distance.euclidean()
    assert repr(ix.quantizer) == "BinaryQuantizer(threshold=0, low=0, high=1)"
    assert repr(ix) == ("AsymmetricBinaryIndex(n=20, dim=40, quantizer=BinaryQuantizer(threshold=0, low=0, high=1), "
                        "distance=Distance('euclidean'))")
    assert ix._ix is None


def test_every_metric_is_accepted_cosine_included():
    X = _X()
    for name in ("squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"):
        ix = AsymmetricBinaryIndex(X, BinaryQuantizer(0.0, 3, 200), Distance(name))
        assert ix.distance == Distance(name) and ix._ix is None
    with pytest.raises(InvalidParameter, match="distance"):  # the sibling still refuses it
        BinaryIndex(X, distance=Distance.cosine())


def test_constructor_checks_raise_first():
    X = _X()
    with pytest.raises(InvalidParameter, match="dim"):
        AsymmetricBinaryIndex(np.zeros((2, 8193), F))
    with pytest.raises(InvalidParameter, match="dim"):
        AsymmetricBinaryIndex(np.zeros((2, 0), F))
    with pytest.raises(EmptyInput):
        AsymmetricBinaryIndex(np.zeros((0, 4), F))
    with pytest.raises(ValueError):
        AsymmetricBinaryIndex(np.zeros(4, F))
    with pytest.raises(InvalidParameter, match="rows"):
        AsymmetricBinaryIndex(X.astype(np.float64))
    with pytest.raises(InvalidParameter, match="quantizer"):
        AsymmetricBinaryIndex(X, quantizer="bq")
    with pytest.raises(InvalidParameter, match="quantizer"):
        AsymmetricBinaryIndex(X, quantizer=vq_amd.ScalarQuantizer(0.0, 1.0, 2))
    with pytest.raises(InvalidParameter, match="distance"):
        AsymmetricBinaryIndex(X, distance="cosine")
    with pytest.raises(InvalidParameter, match="codes"):
        AsymmetricBinaryIndex.from_codes(X)
    with pytest.raises(InvalidParameter, match="words"):
        AsymmetricBinaryIndex.from_packed(np.zeros((2, 2), np.int32), 40)
    with pytest.raises(InvalidParameter, match="dim"):
        AsymmetricBinaryIndex.from_packed(np.zeros((2, 2), np.uint32), 40.5)
    with pytest.raises(InvalidParameter, match="dim"):
        AsymmetricBinaryIndex.from_packed(np.zeros((2, 257), np.uint32), 8193)
    with pytest.raises(ValueError):
        AsymmetricBinaryIndex.from_packed(np.zeros(2, np.uint32), 40)


def test_from_packed_checks_the_width_and_the_pad_bits():
    with pytest.raises(DimensionMismatch):
        AsymmetricBinaryIndex.from_packed(np.zeros((2, 3), np.uint32), 40)
    with pytest.raises(DimensionMismatch):
        AsymmetricBinaryIndex.from_packed(np.zeros((2, 1), np.uint32), 33)
    with pytest.raises(InvalidParameter, match="pad bit"):
        AsymmetricBinaryIndex.from_packed(np.full((2, 2), 1 << 9, np.uint32), 40)
    ok = np.full((2, 2), (1 << 8) - 1, np.uint32)  # dimensions 32 .. 39 set: the last legal bit is bit 7
    ix = AsymmetricBinaryIndex.from_packed(ok, 40)
    assert np.array_equal(ix.packed(), ok) and ix._ix is None
    AsymmetricBinaryIndex.from_packed(np.full((2, 1), 0xFFFFFFFF, np.uint32), 32)  # no pad bits at a whole word


def test_call_checks_leave_the_index_unchanged():
    X = _X()
    ix = AsymmetricBinaryIndex(X, BinaryQuantizer(0.0, 3, 200), Distance.cosine())
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 0)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 21)
    with pytest.raises(InvalidParameter, match="topk"):
        AsymmetricBinaryIndex(np.zeros((2000, 4), F)).search(np.zeros((1, 4), F), 1025)
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
    with pytest.raises(InvalidParameter, match="words"):
        ix.add_packed(np.zeros((2, 2), np.int32))
    with pytest.raises(DimensionMismatch):
        ix.add_packed(np.zeros((2, 3), np.uint32))
    with pytest.raises(InvalidParameter, match="pad bit"):
        ix.add_packed(np.full((2, 2), 1 << 9, np.uint32))
    with pytest.raises(InvalidParameter, match="n"):
        ix.add_packed_device(0, -1)
    with pytest.raises(InvalidParameter, match="no row"):
        ix.remove_rows(np.ones(20, bool))
    with pytest.raises(DimensionMismatch):
        ix.remove_rows(np.ones(19, bool))
    with pytest.raises(InvalidParameter, match="row id"):
        ix.remove_rows(np.array([20]))
    # calls that do nothing need no device either
    assert ix.add(np.zeros((0, 40), F)).size == 0 and ix.add_packed(np.zeros((0, 2), np.uint32)).size == 0
    assert np.array_equal(ix.remove_rows(np.zeros(20, bool)), np.arange(20, dtype=np.uint32))
    idx, dist = ix.search(np.zeros((0, 40), F), 3)
    assert idx.shape == (0, 3) and dist.shape == (0, 3)
    assert ix.range_search(np.zeros((0, 40), F), 1.0)[0].tolist() == [0]
    assert ix._ix is None and len(ix) == 20 and ix.dim == 40  # nothing reached the device, nothing changed


def test_hamming_search_reranked_through_an_index_of_another_shape_is_refused():
    X = _X()
    b = BinaryIndex(X)
    with pytest.raises(DimensionMismatch):
        b.search(X[:2], 5, rerank=AsymmetricBinaryIndex(X[:10]))
    with pytest.raises(DimensionMismatch):
        b.search(X[:2], 5, rerank=AsymmetricBinaryIndex(X[:, :39]))
    with pytest.raises(InvalidParameter, match="candidates"):
        b.search(X[:2], 5, rerank=AsymmetricBinaryIndex(X), candidates=4)
    with pytest.raises(InvalidParameter, match="rerank"):  # the Hamming index itself is still no reranker
        b.search(X[:2], 5, rerank=BinaryIndex(X))
    assert b._ix is None


def test_save_load_round_trip_without_device(tmp_path):
    X = _X(33, 70)
    bq = BinaryQuantizer(0.25, 2, 9)
    codes = np.where(X >= F(0.25), 9, 2).astype(np.uint8)
    words = R.pack(X >= F(0.25))
    for ix in (AsymmetricBinaryIndex(X, bq, Distance.cosine()), AsymmetricBinaryIndex.from_codes(codes, bq, Distance.cosine()),
               AsymmetricBinaryIndex.from_packed(words, 70, bq, Distance.cosine())):
        p = tmp_path / "a.bin"
        ix.save(p)
        raw = p.read_bytes()
        assert raw[:36] == struct.pack(HEAD, b"VQABINX1", 33, 70, 3, 0.25, 2, 9)
        assert raw[36:] == words.astype("<u4").tobytes()
        back = AsymmetricBinaryIndex.load(p)
        assert len(back) == 33 and back.dim == 70 and back.distance == Distance.cosine()
        assert (back.quantizer.threshold, back.quantizer.low, back.quantizer.high) == (np.float32(0.25), 2, 9)
        assert np.array_equal(back.packed(), words)
        assert back._ix is None and ix._ix is None


def test_load_rejects_bad_files(tmp_path):
    words = R.pack(_X(3, 40) >= 0)
    body = words.astype("<u4").tobytes()
    good = struct.pack(HEAD, b"VQABINX1", 3, 40, 3, 0.0, 0, 1) + body
    p = tmp_path / "a.bin"

    def load(raw):
        p.write_bytes(raw)
        return AsymmetricBinaryIndex.load(p)

    load(good)
    with pytest.raises(InvalidData):
        load(b"VQBINIX1" + good[8:])  # the Hamming index's file is not this one
    with pytest.raises(InvalidData):
        load(good[:20])
    with pytest.raises(InvalidData):
        load(b"")
    with pytest.raises(InvalidData):
        load(good[:-1])
    with pytest.raises(InvalidData):
        load(good + b"\0")
    bad_pad = words.copy()
    bad_pad[1, 1] |= 1 << 20
    with pytest.raises(InvalidData, match="pad bit"):
        load(good[:36] + bad_pad.astype("<u4").tobytes())
    with pytest.raises(InvalidParameter, match="distance"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 40, 5, 0.0, 0, 1) + body)
    with pytest.raises(InvalidParameter, match="dim"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 8193, 3, 0.0, 0, 1) + body)
    with pytest.raises(InvalidParameter, match="dim"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 0, 3, 0.0, 0, 1) + body)
    with pytest.raises(InvalidData):
        load(struct.pack(HEAD, b"VQABINX1", 0, 40, 3, 0.0, 0, 1))
    with pytest.raises(InvalidData):
        load(struct.pack(HEAD, b"VQABINX1", 1 << 32, 40, 3, 0.0, 0, 1) + body)
    with pytest.raises(InvalidParameter, match="low"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 40, 3, 0.0, 1, 1) + body)
    with pytest.raises(InvalidParameter, match="low/high"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 40, 3, 0.0, 0, 256) + body)
    with pytest.raises(InvalidParameter, match="threshold"):
        load(struct.pack(HEAD, b"VQABINX1", 3, 40, 3, float("nan"), 0, 1) + body)


def test_null_pointers_are_refused_by_every_entry_point():
    """VQHIP_ERR_NULL_PTR from each new entry point (vqhip_abin_destroy takes NULL like free); no device needed"""
    lib = _lib.load()
    h = C.c_void_p()
    buf = np.zeros(64, np.uint32)
    f32 = np.zeros(64, F)
    src, u32p, f32p = buf.ctypes.data_as(C.c_void_p), _lib.ptr(buf, C.POINTER(C.c_uint32)), _lib.ptr(f32, C.POINTER(C.c_float))
    removed, n = C.c_uint64(), C.c_uint64()
    NULL = _lib.ERR_NULL_PTR
    for create in (lib.vqhip_abin_create, lib.vqhip_abin_create_device):
        assert create(src, _lib.BINARY_PACKED, 2, 32, 0.0, 0, 1, _lib.COSINE, None) == NULL
        assert create(None, _lib.BINARY_PACKED, 2, 32, 0.0, 0, 1, _lib.COSINE, C.byref(h)) == NULL and not h.value
    assert lib.vqhip_abin_destroy(None) == _lib.OK
    assert lib.vqhip_abin_info(None, C.byref(n), None, None, None, None, None) == NULL
    assert lib.vqhip_abin_packed(None, u32p) == NULL
    assert lib.vqhip_abin_search(None, f32p, 1, 1, u32p, f32p) == NULL
    assert lib.vqhip_abin_search_device(None, src, 1, 1, src, src) == NULL
    assert lib.vqhip_abin_search_masked(None, f32p, 1, 1, u32p, u32p, f32p) == NULL
    assert lib.vqhip_abin_search_masked_device(None, src, 1, 1, src, src, src) == NULL
    assert lib.vqhip_abin_search_masked_device(None, src, 1, 1, None, src, src) == NULL
    assert lib.vqhip_abin_rerank(None, f32p, 1, u32p, 1, 1, u32p, f32p) == NULL
    for fn, q in ((lib.vqhip_abin_range_search, f32p), (lib.vqhip_abin_range_search_device, src)):
        assert fn(None, q, 1, f32p, 1, C.byref(h)) == NULL and not h.value
        assert fn(None, q, 1, f32p, 1, None) == NULL
        assert fn(None, q, 1, None, 1, C.byref(h)) == NULL
    for fn, q, m in ((lib.vqhip_abin_range_search_masked, f32p, u32p), (lib.vqhip_abin_range_search_masked_device, src, src)):
        assert fn(None, q, 1, f32p, 1, m, C.byref(h)) == NULL and not h.value
        assert fn(None, q, 1, f32p, 1, None, C.byref(h)) == NULL
    assert lib.vqhip_abin_add(None, src, _lib.BINARY_PACKED, 1) == NULL
    assert lib.vqhip_abin_add_device(None, src, _lib.BINARY_PACKED, 1) == NULL
    assert lib.vqhip_abin_remove(None, u32p, C.byref(removed)) == NULL
    assert lib.vqhip_abin_remove_device(None, src, C.byref(removed)) == NULL


def test_create_checks_come_before_the_device():
    """the C ABI's own checks, in the binary index's order and with its texts; cosine passes the metric check"""
    lib = _lib.load()
    h = C.c_void_p()
    words = np.zeros((2, 2), np.uint32)
    src = words.ctypes.data_as(C.c_void_p)

    def create(kind=_lib.BINARY_PACKED, n=2, d=40, thr=0.0, low=0, high=1, metric=_lib.COSINE, fn=lib.vqhip_abin_create, s=src):
        rc = fn(s, kind, n, d, thr, low, high, metric, C.byref(h))
        return rc, _lib.last_error()

    INVALID = _lib.ERR_INVALID_INPUT
    rc, msg = create(kind=3)
    assert rc == INVALID and "source kind" in msg
    for d in (0, 8193):
        rc, msg = create(d=d)
        assert rc == INVALID and "[1, 8192]" in msg
    for n in (0, 1 << 32):
        rc, msg = create(n=n)
        assert rc == INVALID and "n must be" in msg
    rc, msg = create(low=1, high=1)
    assert rc == INVALID and "low" in msg
    for metric in (-1, 5):
        rc, msg = create(metric=metric)
        assert rc == INVALID and "metric" in msg
    words[1, 1] = 1 << 8
    rc, msg = create()
    assert rc == INVALID and "row 1 has a pad bit set" in msg
    words[1, 1] = 0
    odd = C.c_void_p(words.ctypes.data + 2)
    rc, msg = create(fn=lib.vqhip_abin_create_device, s=odd)
    assert rc == INVALID and "words are not 4-byte aligned" in msg
    rc, msg = create(kind=_lib.BINARY_F32, fn=lib.vqhip_abin_create_device, s=odd)
    assert rc == INVALID and "rows are not 4-byte aligned" in msg
    assert not h.value
    # every argument check passed: a machine without a GPU ends at the device, one with a GPU creates the index
    rc, _ = create()
    assert rc in (_lib.OK, _lib.ERR_NO_DEVICE)
    if rc == _lib.OK:
        assert lib.vqhip_abin_destroy(h) == _lib.OK
