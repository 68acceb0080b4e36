"""The binary index on the MI355X (vq_amd.BinaryIndex, vqhip_binary_*, k_binary.hip) against its numpy statement
(tests/ref_binary.py): packed words bit for bit, search indices equal and distances equal as uint32 bits."""
import numpy as np
import pytest

import ref_binary as R
from vq_amd import BinaryIndex, BinaryQuantizer, Distance, FlatIndex

pytestmark = pytest.mark.gpu

F = np.float32
DIST = {R.SQ: Distance.squared_euclidean(), R.EUC: Distance.euclidean(), R.MAN: Distance.manhattan()}


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F)


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("d", [1, 7, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 1024, 8191, 8192])
def test_pack_batch_and_index_words(d):
    rng = np.random.default_rng(d)
    n = 37
    X = rng.standard_normal((n, d)).astype(F)
    X[0, : min(d, 4)] = [np.nan, -0.0, 0.0, np.inf][: min(d, 4)]
    bq = BinaryQuantizer(0.0)
    want = R.pack(R.bits_f32(X, 0.0))
    got = bq.pack_batch(X)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(bq.unpack_batch(got, d), bq.quantize_batch(X))
    assert np.array_equal(BinaryIndex(X).packed(), want)
    bq2 = BinaryQuantizer(0.25, 3, 200)
    codes = bq2.quantize_batch(X)
    assert np.array_equal(BinaryIndex.from_codes(codes, bq2).packed(), R.pack(R.bits_u8(codes, 200)))
    assert np.array_equal(BinaryIndex.from_packed(want, d).packed(), want)


def test_pack_batch_unaligned_rows():
    X = _rows(65, 37, 3)
    buf = np.empty(X.size + 1, F)
    Xu = buf[1:].reshape(X.shape)
    Xu[:] = X
    assert np.array_equal(BinaryQuantizer(0.1).pack_batch(Xu), R.pack(R.bits_f32(X, 0.1)))


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("low,high", [(0, 1), (0, 255), (254, 255), (3, 200)])
@pytest.mark.parametrize("n,d", [(1037, 100), (4099, 256), (600, 33)])
def test_search_matches_statement(metric, low, high, n, d):
    X = _rows(n, d, n + d)
    Q = _rows(23, d, 5)
    Q[0] = X[17]  # a query equal to a row
    X[40] = X[41]  # duplicate rows
    bq = BinaryQuantizer(0.0, low, high)
    ix = BinaryIndex(X, bq, DIST[metric])
    for topk in (1, 10, min(n, 1024)):
        _same(ix.search(Q, topk), R.search_rows(Q, X, 0.0, low, high, metric, topk))


def test_search_n_equals_topk():
    X = _rows(300, 64, 1)
    Q = _rows(5, 64, 2)
    _same(BinaryIndex(X).search(Q, 300), R.search_rows(Q, X, 0.0, 0, 1, R.MAN, 300))


def test_search_several_batches():
    X = _rows(2000, 96, 11)
    Q = _rows(2500, 96, 12)
    _same(BinaryIndex(X, distance=Distance.euclidean()).search(Q, 10), R.search_rows(Q, X, 0.0, 0, 1, R.EUC, 10))


@pytest.mark.parametrize("d", [1, 3])
def test_heavy_ties_take_lowest_ids(d):
    n = 100_003
    X = _rows(n, d, 40 + d)
    Q = _rows(7, d, 41)
    _same(BinaryIndex(X).search(Q, 1024), R.search_rows(Q, X, 0.0, 0, 1, R.MAN, 1024))


def test_search_from_codes_and_packed_equal_rows():
    X = _rows(3000, 200, 21)
    Q = _rows(9, 200, 22)
    bq = BinaryQuantizer(0.0, 2, 9)
    want = BinaryIndex(X, bq, Distance.squared_euclidean()).search(Q, 50)
    _same(BinaryIndex.from_codes(bq.quantize_batch(X), bq, Distance.squared_euclidean()).search(Q, 50), want)
    _same(BinaryIndex.from_packed(bq.pack_batch(X), 200, bq, Distance.squared_euclidean()).search(Q, 50), want)


def test_search_device_equals_host():
    torch = pytest.importorskip("torch")
    X = _rows(5000, 128, 31)
    Q = _rows(40, 128, 32)
    ix = BinaryIndex(X, distance=Distance.euclidean())
    want = ix.search(Q, 17)
    qd = torch.from_numpy(Q).cuda()
    idx = torch.empty((40, 17), dtype=torch.int32, device="cuda")
    dist = torch.empty((40, 17), dtype=torch.float32, device="cuda")
    ix.search_device(qd.data_ptr(), 40, 17, idx.data_ptr(), dist.data_ptr())
    torch.cuda.synchronize()
    _same((idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want)


def test_rerank_equals_flat_rerank_of_candidates():
    X = _rows(4000, 64, 51)
    Q = _rows(12, 64, 52)
    ix = BinaryIndex(X)
    flat = FlatIndex(X, Distance.cosine())
    got = ix.search(Q, 10, rerank=flat, candidates=80)
    cand, _ = ix.search(Q, 80)
    _same(got, flat.rerank(Q, cand, 10))


def test_loaded_index_searches_identically(tmp_path):
    X = _rows(3001, 77, 61)
    Q = _rows(8, 77, 62)
    ix = BinaryIndex(X, BinaryQuantizer(0.1, 1, 4), Distance.squared_euclidean())
    want = ix.search(Q, 25)
    ix.save(tmp_path / "b.bin")
    back = BinaryIndex.load(tmp_path / "b.bin")
    _same(back.search(Q, 25), want)
    assert np.array_equal(back.packed(), ix.packed())


def test_sampled_1m_x_1024():
    n, d = 1 << 20, 1024
    rng = np.random.default_rng(71)
    X = rng.standard_normal((n, d), dtype=F)
    bq = BinaryQuantizer(0.0)
    words = bq.pack_batch(X)
    sample = np.sort(rng.choice(n, 2048, replace=False))
    assert np.array_equal(words[sample], R.pack(R.bits_f32(X[sample], 0.0)))
    Q = rng.standard_normal((8, d), dtype=F)
    ix = BinaryIndex.from_packed(words, d)
    got = ix.search(Q, 100)
    _same(got, R.search(R.pack(R.bits_f32(Q, 0.0)), words, d, 0, 1, R.MAN, 100))
