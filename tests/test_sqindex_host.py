"""CPU checks of the scalar index (vq_amd.ScalarIndex, include/vqhip.h vqhip_sqindex_*): the numpy statement
(tests/ref_sqindex.py) against the oracle's Distance::compute on decoded vectors and against ScalarQuantizer's decode
formula for every byte, the argument checks -- which all raise before any device is touched -- and the file format."""
import ctypes as C
import struct

import numpy as np
import pytest

import ref_knn as K
import ref_sqindex as R

F = np.float32


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


# ---- the statement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq", R.QUANTIZERS + [(1e-40, 3e-40, 256), (0.0, 1e-45, 3)])
def test_decode_table_is_the_quantizers_formula(sq):
    """v(c) = min + f32(c) * step, two roundings, for all 256 bytes: levels < 256 and the inf step included"""
    mn, mx, levels = sq
    with np.errstate(all="ignore"):
        step = F(F(F(mx) - F(mn)) / F(levels - 1))
        want = np.array([F(F(mn) + F(F(c) * step)) for c in range(256)], F)
    got = R.table(sq)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if sq == (-3e38, 3e38, 2):
        assert np.isinf(step) and np.isnan(got[0]) and np.all(got[1:] == np.inf)
    if sq == (0.0, 1.0, 2):
        assert got[1] == 1.0 and got[255] == 255.0  # codes >= levels decode by the same formula


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", [1, 3, 8, 33])
def test_statement_equals_oracle_distance_on_decoded_vectors(orc, metric, d):
    rng = np.random.default_rng(300 + d)
    for sq in R.QUANTIZERS:
        codes = rng.integers(0, 256, (40, d), dtype=np.uint8)
        codes[5] = 0
        codes[6] = codes[7]
        V = R.decode(sq, codes)
        Q = np.concatenate([rng.standard_normal((3, d)).astype(F), V[:1], np.zeros((1, d), F)])
        for q in Q:
            got = R.distances(metric, q, sq, codes)
            want = np.array([orc.distance(metric, q, v) for v in V], F)
            nan_g, nan_w = np.isnan(got), np.isnan(want)
            assert np.array_equal(nan_g, nan_w)
            assert np.array_equal(got[~nan_g].view(np.uint32), want[~nan_w].view(np.uint32))


# ---- argument checks: no device needed ----------------------------------------------------------------------------
def _no_device(monkeypatch):
    """any attempt to reach the library's index fails the test"""
    from vq_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "SQIndex", boom)
    monkeypatch.setattr(_lib, "Flat", boom)


def _sq():
    import vq_amd

    return vq_amd.ScalarQuantizer(-1.0, 1.0, 256)


def test_constructs_without_a_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = vq_amd.ScalarIndex(np.zeros((5, 3), F), _sq())
    assert len(ix) == 5 and ix.dim == 3 and ix.distance == vq_amd.Distance.euclidean() and ix.quantizer.levels == 256
    ic = vq_amd.ScalarIndex.from_codes(np.zeros((2, 7), np.uint8), _sq(), vq_amd.Distance.cosine())
    assert "ScalarIndex(n=2, dim=7" in repr(ic) and "cosine" in repr(ic)
    assert ic.codes().shape == (2, 7)


@pytest.mark.parametrize("rows, exc", [
    (np.zeros((0, 4), F), "EmptyInput"),
    (np.zeros((4, 0), F), "InvalidParameter"),
    (np.zeros((4, 3), np.float64), "InvalidParameter"),
    (np.zeros((4, 3), np.uint8), "InvalidParameter"),
    (np.zeros(4, F), ValueError),
])
def test_rejects_bad_rows(rows, exc):
    import vq_amd

    e = getattr(vq_amd, exc) if isinstance(exc, str) else exc
    with pytest.raises(e):
        vq_amd.ScalarIndex(rows, _sq())


@pytest.mark.parametrize("codes, exc", [
    (np.zeros((0, 4), np.uint8), "EmptyInput"),
    (np.zeros((4, 0), np.uint8), "InvalidParameter"),
    (np.zeros((4, 3), F), "InvalidParameter"),
    (np.zeros((4, 3), np.int8), "InvalidParameter"),
    (np.zeros((2, 2, 2), np.uint8), ValueError),
])
def test_rejects_bad_codes(codes, exc):
    import vq_amd

    e = getattr(vq_amd, exc) if isinstance(exc, str) else exc
    with pytest.raises(e):
        vq_amd.ScalarIndex.from_codes(codes, _sq())


def test_rejects_bad_quantizer_and_distance():
    import vq_amd

    with pytest.raises(vq_amd.InvalidParameter, match="quantizer"):
        vq_amd.ScalarIndex(np.zeros((4, 3), F), (-1.0, 1.0, 256))
    with pytest.raises(vq_amd.InvalidParameter, match="quantizer"):
        vq_amd.ScalarIndex.from_codes(np.zeros((4, 3), np.uint8), vq_amd.BinaryQuantizer(0.0))
    with pytest.raises(vq_amd.InvalidParameter, match="distance"):
        vq_amd.ScalarIndex(np.zeros((4, 3), F), _sq(), "euclidean")


CRATE_TEXTS = [
    ((np.nan, 1.0, 256), "Invalid parameter 'min': must be finite (not NaN or infinite)"),
    ((0.0, np.inf, 256), "Invalid parameter 'max': must be finite (not NaN or infinite)"),
    ((1.0, 1.0, 256), "Invalid parameter 'max': must be greater than min"),
    ((0.0, 1.0, 1), "Invalid parameter 'levels': must be at least 2"),
    ((0.0, 1.0, 257), "Invalid parameter 'levels': must be no more than 256 to fit in u8"),
]


@pytest.mark.parametrize("params, text", CRATE_TEXTS)
def test_cabi_reports_the_crates_quantizer_errors_unchanged(params, text):
    """every create form runs vqhip_sq_check first -- before NULL, shape and device checks -- and keeps its text"""
    from vq_amd import _lib

    lib = _lib.load()
    codes = np.zeros((4, 3), np.uint8)
    h = C.c_void_p()
    for name in ("vqhip_sqindex_create", "vqhip_sqindex_create_device", "vqhip_sqindex_create_rows",
                 "vqhip_sqindex_create_rows_device"):
        rc = getattr(lib, name)(*params, codes.ctypes.data_as(C.c_void_p), 4, 3, 1, C.byref(h))
        assert rc == _lib.ERR_INVALID_INPUT and _lib.last_error() == text, (name, _lib.last_error())
        assert not h.value


def test_cabi_checks_without_device():
    from vq_amd import _lib

    lib = _lib.load()
    codes = np.zeros((4, 4), np.uint8)
    p = codes.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    for name in ("vqhip_sqindex_create", "vqhip_sqindex_create_rows"):
        fn = getattr(lib, name)
        for args in [(p, 0, 3, 1), (p, 4, 0, 1), (p, 4, 3, 7), (p, 4, 3, -1), (p, 1 << 32, 3, 1)]:
            assert fn(-1.0, 1.0, 256, *args, C.byref(h)) == _lib.ERR_INVALID_INPUT, (name, args)
            assert not h.value
        assert fn(-1.0, 1.0, 256, None, 4, 3, 1, C.byref(h)) == _lib.ERR_NULL_PTR
        assert fn(-1.0, 1.0, 256, p, 4, 3, 1, None) == _lib.ERR_NULL_PTR
    assert lib.vqhip_sqindex_create_rows_device(-1.0, 1.0, 256, C.c_void_p(p.value + 1), 1, 3, 1, C.byref(h)) == _lib.ERR_INVALID_INPUT
    assert "aligned" in _lib.last_error()
    assert lib.vqhip_sqindex_search(None, None, 1, 1, None, None) == _lib.ERR_NULL_PTR
    assert lib.vqhip_sqindex_rerank(None, None, 1, None, 1, 1, None, None) == _lib.ERR_NULL_PTR
    assert lib.vqhip_sqindex_info(None, None, None, None, None, None, None) == _lib.ERR_NULL_PTR
    assert lib.vqhip_sqindex_codes(None, None) == _lib.ERR_NULL_PTR
    assert lib.vqhip_sqindex_destroy(None) == _lib.OK


def test_search_checks_before_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = vq_amd.ScalarIndex.from_codes(np.zeros((20, 4), np.uint8), _sq())
    with pytest.raises(vq_amd.DimensionMismatch, match="expected 4, found 5"):
        ix.search(np.zeros((2, 5), F), 3)
    for k in (0, 21, -1):
        with pytest.raises(vq_amd.InvalidParameter, match="topk"):
            ix.search(np.zeros((2, 4), F), k)
    big = vq_amd.ScalarIndex(np.zeros((2000, 4), F), _sq())
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        big.search(np.zeros((1, 4), F), 1025)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search(np.zeros((1, 4), F), 2.5)
    with pytest.raises(ValueError):
        ix.search(np.zeros((1, 2, 4), F), 1)
    i, d = ix.search(np.zeros((0, 4), F), 3)
    assert i.shape == (0, 3) and d.shape == (0, 3)
    with pytest.raises(vq_amd.InvalidParameter, match="topk"):
        ix.search_device(0, 1, 21, 0, 0)
    with pytest.raises(vq_amd.InvalidParameter, match="nq"):
        ix.search_device(0, 1 << 32, 3, 0, 0)


def test_rerank_checks_before_device(monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    ix = vq_amd.ScalarIndex.from_codes(np.zeros((20, 4), np.uint8), _sq())
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
        vq_amd.ScalarIndex.from_codes(np.zeros((5000, 4), np.uint8), _sq()).rerank(q, np.tile(np.arange(4097), (2, 1)), 1)
    with pytest.raises(vq_amd.InvalidParameter, match="integers"):
        ix.rerank(q, np.zeros((2, 3), F), 1)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.rerank(q, np.array([[0, 1, 2]]), 1)
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.rerank(np.zeros((2, 3), F), np.array([[0, 1, 2], [2, 3, 4]]), 1)


def test_rerank_keyword_takes_a_scalar_index_and_refuses_other_types(monkeypatch):
    """flat.rerank_candidates: a ScalarIndex passes the checks a FlatIndex passes; any other type is refused as before"""
    import vq_amd
    from vq_amd.flat import adc_then_rerank, rerank_candidates

    _no_device(monkeypatch)

    def adc(q, c):
        raise AssertionError("the search ran before the arguments were checked")

    q = np.zeros((1, 4), F)
    six = vq_amd.ScalarIndex.from_codes(np.zeros((20, 4), np.uint8), _sq())
    assert rerank_candidates(20, 4, 2, six, None) == 8
    assert rerank_candidates(20, 4, 2, six, 5) == 5
    for bad in (object(), np.zeros((20, 4), F), _sq(), None):
        with pytest.raises(vq_amd.InvalidParameter, match="rerank"):
            adc_then_rerank(adc, 20, 4, q, 2, bad, None)
    with pytest.raises(vq_amd.DimensionMismatch):
        adc_then_rerank(adc, 21, 4, q, 2, six, None)
    with pytest.raises(vq_amd.DimensionMismatch):
        adc_then_rerank(adc, 20, 8, q, 2, six, None)
    with pytest.raises(vq_amd.InvalidParameter, match="candidates"):
        adc_then_rerank(adc, 20, 4, q, 5, six, 3)
    bix = vq_amd.BinaryIndex(np.zeros((20, 4), F))
    with pytest.raises(vq_amd.InvalidParameter, match="rerank"):
        bix.search(q, 2, rerank=object())
    with pytest.raises(vq_amd.DimensionMismatch):
        bix.search(q, 2, rerank=vq_amd.ScalarIndex.from_codes(np.zeros((19, 4), np.uint8), _sq()))


# ---- file ---------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_from_codes(tmp_path, monkeypatch):
    import vq_amd

    _no_device(monkeypatch)
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 256, (37, 13), dtype=np.uint8)
    sq = vq_amd.ScalarQuantizer(-3.0, 5.0, 17)
    ix = vq_amd.ScalarIndex.from_codes(codes, sq, vq_amd.Distance.manhattan())
    path = tmp_path / "a.vqsq"
    ix.save(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"VQSQIDX1" and len(raw) == 36 + 37 * 13
    assert struct.unpack("<QIIffI", raw[8:36]) == (37, 13, 2, -3.0, 5.0, 17)
    assert raw[36:] == codes.tobytes()
    back = vq_amd.ScalarIndex.load(path)
    assert len(back) == 37 and back.dim == 13 and back.distance == vq_amd.Distance.manhattan()
    assert (back.quantizer.min, back.quantizer.max, back.quantizer.levels) == (-3.0, 5.0, 17)
    assert np.array_equal(back.codes(), codes)


def test_load_refuses_bad_files(tmp_path):
    import vq_amd

    codes = np.arange(12, dtype=np.uint8).reshape(3, 4)
    good = tmp_path / "good"
    vq_amd.ScalarIndex.from_codes(codes, _sq()).save(good)
    raw = open(good, "rb").read()

    def load(data):
        p = tmp_path / "x"
        p.write_bytes(data)
        return vq_amd.ScalarIndex.load(p)

    with pytest.raises(vq_amd.InvalidData, match="VQSQIDX1"):
        load(b"VQBINIX1" + raw[8:])
    with pytest.raises(vq_amd.InvalidData, match="header"):
        load(raw[:20])
    with pytest.raises(vq_amd.InvalidData, match="truncated codes"):
        load(raw[:-1])
    with pytest.raises(vq_amd.InvalidData, match="trailing"):
        load(raw + b"\0")
    with pytest.raises(vq_amd.InvalidData, match="row count"):
        load(raw[:8] + struct.pack("<Q", 0) + raw[16:])
    with pytest.raises(vq_amd.InvalidParameter, match="dim"):
        load(raw[:16] + struct.pack("<I", 0) + raw[20:])
    with pytest.raises(vq_amd.InvalidParameter, match="metric"):
        load(raw[:20] + struct.pack("<I", 9) + raw[24:])
    with pytest.raises(vq_amd.InvalidParameter, match="must be greater than min"):
        load(raw[:24] + struct.pack("<ff", 1.0, 1.0) + raw[32:])
    with pytest.raises(vq_amd.InvalidParameter, match="no more than 256"):
        load(raw[:32] + struct.pack("<I", 300) + raw[36:])
