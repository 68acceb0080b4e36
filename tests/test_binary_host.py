"""CPU checks of the binary index (vq_amd.BinaryIndex, include/vqhip.h vqhip_binary_*): the numpy statement
(tests/ref_binary.py) against the oracle's Distance::compute on dequantized BQ vectors, the strict monotonicity of every
S table, the bit rule on special values, the argument checks (all before any device is touched) and the file format."""
import struct

import numpy as np
import pytest

import ref_binary as R
from vq_amd import BinaryIndex, BinaryQuantizer, Distance, FlatIndex
from vq_amd.errors import DimensionMismatch, EmptyInput, InvalidData, InvalidParameter

F = np.float32
DIST = {R.SQ: Distance.squared_euclidean(), R.EUC: Distance.euclidean(), R.MAN: Distance.manhattan()}


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _lowhigh_vectors(d, H, low, high):
    """two dequantized BQ vectors of dimension d that differ in H places, the differing ones spread over the vector"""
    a = np.full(d, F(low))
    b = a.copy()
    where = np.linspace(0, d - 1, H).astype(int) if H else np.array([], int)
    b[np.unique(where)] = F(high)
    a[::3] = F(high)  # agreeing high dimensions too
    b[::3] = np.where(np.isin(np.arange(d)[::3], where), F(low), F(high))
    return a, b, int((a != b).sum())


@pytest.mark.parametrize("low,high", [(0, 1), (0, 255), (254, 255), (3, 200)])
@pytest.mark.parametrize("d", [1, 7, 31, 32, 33, 100, 1024])
def test_statement_equals_oracle_distance(orc, d, low, high):
    for metric in R.METRICS:
        D = R.reported(d, low, high, metric)
        seen = set()
        for H in range(d + 1):
            a, b, h = _lowhigh_vectors(d, H, low, high)
            if h in seen and d > 100:
                continue
            seen.add(h)
            want = orc.distance(metric, a, b)
            assert D[h].view(np.uint32) == np.float32(want).view(np.uint32), (metric, d, h)
        assert len(seen) == d + 1 or d > 100  # every H in 0..d for the small d


def test_statement_every_h_at_1024(orc):
    d, low, high = 1024, 3, 200
    for metric in R.METRICS:
        D = R.reported(d, low, high, metric)
        for h in range(d + 1):
            a = np.full(d, F(low))
            b = a.copy()
            b[np.arange(h) * 7 % d if h <= d // 7 else np.arange(h)] = F(high)
            assert int((a != b).sum()) == h
            assert D[h].view(np.uint32) == np.float32(orc.distance(metric, a, b)).view(np.uint32)


def test_statement_equals_quantize_then_distance(orc):
    rng = np.random.default_rng(3)
    bq = (0.1, 2, 9)
    X = rng.standard_normal((40, 45)).astype(F)
    Q = rng.standard_normal((3, 45)).astype(F)
    deq = lambda v: np.where(v >= F(bq[0]), F(bq[2]), F(bq[1])).astype(F)  # noqa: E731
    for metric in R.METRICS:
        idx, dist = R.search_rows(Q, X, *bq, metric, 40)
        for qi, q in enumerate(Q):
            want = np.array([orc.distance(metric, deq(q), deq(x)) for x in X], F)
            order = sorted(range(40), key=lambda i: (want[i], i))
            assert list(idx[qi]) == order
            assert np.array_equal(dist[qi].view(np.uint32), want[order].view(np.uint32))


def test_tables_strictly_increasing():
    """for every a in 1..255, d <= 8192 and all three metrics: S strictly increasing (and sqrtf(S) for Euclidean), so
    the (H, row) order is the (D, row) order"""
    d = 8192
    for a in range(1, 256):
        for metric in R.METRICS:
            D = R.reported(d, 0, a, metric)
            assert D[0] == 0 and not np.signbit(D[0])
            assert bool((D[1:] > D[:-1]).all()), (a, metric)


def test_table_depends_on_high_minus_low_only():
    for metric in R.METRICS:
        assert np.array_equal(R.table(300, 3, 200, metric), R.table(300, 0, 197, metric))


def test_pack_rule_special_values():
    tiny = np.float32(1e-45)  # the smallest subnormal
    x = np.array([[np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, np.nextafter(F(0.5), F(0)), tiny, -tiny]], F)
    assert R.bits_f32(x, 0.5).tolist() == [[False, True, False, False, False, True, False, False, False]]
    assert R.bits_f32(x, 0.0).tolist() == [[False, True, False, True, True, True, True, True, False]]
    assert R.bits_f32(x, -0.0).tolist() == R.bits_f32(x, 0.0).tolist()
    assert R.bits_f32(x, tiny).tolist() == [[False, True, False, False, False, True, True, True, False]]


def test_pack_layout():
    bits = np.zeros((2, 33), bool)
    bits[0, 0] = bits[0, 31] = bits[0, 32] = True
    bits[1, 5] = True
    w = R.pack(bits)
    assert w.dtype == np.uint32 and w.shape == (2, 2)
    assert w.tolist() == [[0x80000001, 1], [1 << 5, 0]]
    bq = BinaryQuantizer(0.0, 3, 7)
    assert np.array_equal(bq.unpack_batch(w, 33), np.where(bits, 7, 3).astype(np.uint8))


def _X(n=20, d=40):
    return np.random.default_rng(0).standard_normal((n, d)).astype(F)


def test_argument_checks_raise_first():
    X = _X()
    with pytest.raises(InvalidParameter, match="distance"):
        BinaryIndex(X, distance=Distance.cosine())
    with pytest.raises(InvalidParameter, match="distance"):
        BinaryIndex(X, distance=Distance.cosine_unclamped())
    with pytest.raises(InvalidParameter, match="dim"):
        BinaryIndex(np.zeros((2, 8193), F))
    with pytest.raises(InvalidParameter, match="dim"):
        BinaryIndex(np.zeros((2, 0), F))
    with pytest.raises(EmptyInput):
        BinaryIndex(np.zeros((0, 4), F))
    with pytest.raises(InvalidParameter, match="rows"):
        BinaryIndex(X.astype(np.float64))
    with pytest.raises(InvalidParameter, match="quantizer"):
        BinaryIndex(X, quantizer="bq")
    with pytest.raises(InvalidParameter, match="codes"):
        BinaryIndex.from_codes(X)
    with pytest.raises(InvalidParameter, match="words"):
        BinaryIndex.from_packed(np.zeros((2, 2), np.int32), 40)
    with pytest.raises(DimensionMismatch):
        BinaryIndex.from_packed(np.zeros((2, 3), np.uint32), 40)
    with pytest.raises(InvalidParameter, match="pad bit"):
        BinaryIndex.from_packed(np.full((2, 2), 1 << 9, np.uint32), 40)
    ix = BinaryIndex(X)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 0)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search(X[:2], 21)
    with pytest.raises(InvalidParameter, match="topk"):
        BinaryIndex(np.zeros((2000, 4), F)).search(np.zeros((1, 4), F), 1025)
    with pytest.raises(DimensionMismatch):
        ix.search(X[:2, :39], 5)
    with pytest.raises(InvalidParameter, match="topk"):
        ix.search_device(0, 1, 0, 0, 0)
    with pytest.raises(InvalidParameter, match="nq"):
        ix.search_device(0, -1, 1, 0, 0)
    with pytest.raises(InvalidParameter, match="candidates"):
        ix.search(X[:2], 5, candidates=10)
    with pytest.raises(InvalidParameter, match="rerank"):
        ix.search(X[:2], 5, rerank="flat")
    with pytest.raises(DimensionMismatch):
        ix.search(X[:2], 5, rerank=FlatIndex(X[:10]))
    with pytest.raises(InvalidParameter, match="candidates"):
        ix.search(X[:2], 5, rerank=FlatIndex(X), candidates=4)
    assert ix._ix is None  # nothing reached the device


def test_accessors_and_repr():
    ix = BinaryIndex(_X())
    assert len(ix) == 20 and ix.dim == 40
    assert ix.distance == Distance.manhattan()
    assert repr(ix.quantizer) == "BinaryQuantizer(threshold=0, low=0, high=1)"
    assert repr(ix) == ("BinaryIndex(n=20, dim=40, quantizer=BinaryQuantizer(threshold=0, low=0, high=1), "
                        "distance=Distance('manhattan'))")


def test_save_load_round_trip_without_device(tmp_path):
    X = _X(33, 70)
    bq = BinaryQuantizer(0.25, 2, 9)
    codes = np.where(X >= F(0.25), 9, 2).astype(np.uint8)
    words = R.pack(R.bits_f32(X, 0.25))
    for ix in (BinaryIndex.from_codes(codes, bq, Distance.euclidean()),
               BinaryIndex.from_packed(words, 70, bq, Distance.euclidean())):
        p = tmp_path / "b.bin"
        ix.save(p)
        raw = p.read_bytes()
        head = struct.pack("<8sIIfIIQ", b"VQBINIX1", 1, 70, 0.25, 2, 9, 33)
        assert raw[:36] == head
        assert raw[36:] == words.astype("<u4").tobytes()
        back = BinaryIndex.load(p)
        assert len(back) == 33 and back.dim == 70 and back.distance == Distance.euclidean()
        assert (back.quantizer.threshold, back.quantizer.low, back.quantizer.high) == (np.float32(0.25), 2, 9)
        assert np.array_equal(back._host_words(), words)
        assert back._ix is None


def test_load_rejects_bad_files(tmp_path):
    words = R.pack(R.bits_f32(_X(3, 40), 0.0))
    good = struct.pack("<8sIIfIIQ", b"VQBINIX1", 2, 40, 0.0, 0, 1, 3) + words.astype("<u4").tobytes()
    p = tmp_path / "b.bin"

    def load(raw):
        p.write_bytes(raw)
        return BinaryIndex.load(p)

    load(good)
    with pytest.raises(InvalidData):
        load(b"VQBINIX2" + good[8:])
    with pytest.raises(InvalidData):
        load(good[:20])
    with pytest.raises(InvalidData):
        load(good[:-1])
    with pytest.raises(InvalidData):
        load(good + b"\0")
    bad_pad = words.copy()
    bad_pad[1, 1] |= 1 << 20
    with pytest.raises(InvalidData, match="pad bit"):
        load(good[:36] + bad_pad.astype("<u4").tobytes())
    with pytest.raises(InvalidParameter, match="distance"):
        load(struct.pack("<8sIIfIIQ", b"VQBINIX1", 3, 40, 0.0, 0, 1, 3) + good[36:])
    with pytest.raises(InvalidParameter, match="dim"):
        load(struct.pack("<8sIIfIIQ", b"VQBINIX1", 2, 8193, 0.0, 0, 1, 3) + good[36:])
    with pytest.raises(InvalidData):
        load(struct.pack("<8sIIfIIQ", b"VQBINIX1", 2, 40, 0.0, 0, 1, 0))
    with pytest.raises(InvalidParameter, match="low"):
        load(struct.pack("<8sIIfIIQ", b"VQBINIX1", 2, 40, 0.0, 1, 1, 3) + good[36:])
    with pytest.raises(InvalidParameter, match="threshold"):
        load(struct.pack("<8sIIfIIQ", b"VQBINIX1", 2, 40, float("nan"), 0, 1, 3) + good[36:])
