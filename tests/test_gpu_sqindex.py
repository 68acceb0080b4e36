"""The scalar index on the MI355X (vq_amd.ScalarIndex, vqhip_sqindex_*, vq_amd/csrc/k_sqindex.hip) against the numpy
statement (tests/ref_sqindex.py): indices equal, distances equal as uint32 bits.  All five metrics, d around the
32-dimension chunks and on each of the loader's three widths (d % 16 == 0, d % 4 == 0, neither), n off every tile,
topk 1 / 10 / min(n, 1024), four quantizers (one with an infinite step), planted ties / zeros / NaN / inf, codes >=
levels, unaligned buffers, the encode at create, large shapes against FlatIndex over the decoded rows, rerank, the
rerank keyword of the other indexes, the device form and the file."""
import numpy as np
import pytest

import ref_knn as K
import ref_sqindex as R

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
DIMS = [1, 3, 7, 31, 32, 33, 48, 64, 100, 128, 129, 768]
NS = [1, 37, 63, 64, 65, 1037, 4099]


def _assert_same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _quantizer(sq):
    import vq_amd

    return vq_amd.ScalarQuantizer(*sq)


def _index(codes, sq, metric):
    import vq_amd

    return vq_amd.ScalarIndex.from_codes(codes, _quantizer(sq), vq_amd.Distance(NAMES[metric]))


def _codes(n, d, sq, rng):
    """codes inside the quantizer's levels, with exact duplicate rows (ties by row id)"""
    c = rng.integers(0, sq[2], (n, d), dtype=np.uint8)
    if n >= 30:
        c[n - 3:] = c[20:23]
    return c


def _queries(nq, d, sq, codes, rng):
    mn, mx = max(sq[0], -4.0), min(sq[1], 4.0)
    Q = (mn + (mx - mn) * rng.random((nq, d))).astype(F)
    Q[0] = R.decode(sq, codes[min(21, len(codes) - 1)])  # a query equal to a decoded (and duplicated) row
    if nq > 2:
        Q[2] = 0.0  # the zero query (cosine: the EPSILON rule)
    return Q


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_search_matches_statement(metric, d):
    rng = np.random.default_rng(1000 * metric + d)
    for sq in R.QUANTIZERS:
        codes = _codes(1037, d, sq, rng)
        Q = _queries(5, d, sq, codes, rng)
        got = _index(codes, sq, metric).search(Q, 10)
        _assert_same(got, R.search(metric, Q, sq, codes, 10))


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("n", NS)
def test_rows_and_topk_edges(metric, n):
    rng = np.random.default_rng(77 * metric + n)
    for j, d in enumerate((33, 64, 100)):  # the byte, 16-byte and dword loaders
        sq = R.QUANTIZERS[(n + j + metric) % len(R.QUANTIZERS)]
        codes = _codes(n, d, sq, rng)
        Q = _queries(4, d, sq, codes, rng)
        ix = _index(codes, sq, metric)
        for topk in sorted({1, min(10, n), min(n, 1024)}):
            _assert_same(ix.search(Q, topk), R.search(metric, Q, sq, codes, topk))


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("sq", R.QUANTIZERS[:3])
def test_planted_rows_and_queries(metric, sq):
    """duplicate rows, a query equal to a decoded row, a zero row (where the quantizer has a zero value) and a zero query
    -- cosine's EPSILON rule on either side -- and NaN / +-inf in queries"""
    rng = np.random.default_rng(5 + metric)
    n, d = 700, 48
    codes = _codes(n, d, sq, rng)
    tab = R.table(sq)
    zero = np.flatnonzero(tab == 0.0)
    if zero.size:
        codes[11] = zero[0]  # the zero row
        codes[300] = zero[0]
    codes[40:50] = codes[60]  # ten copies of one row
    Q = _queries(8, d, sq, codes, rng)
    Q[1] = R.decode(sq, codes[60])
    Q[3, d // 2] = np.nan
    Q[4, 0] = np.inf
    Q[5, -1] = -np.inf
    Q[6] = np.inf
    ix = _index(codes, sq, metric)
    for topk in (1, 10, 700):
        _assert_same(ix.search(Q, topk), R.search(metric, Q, sq, codes, topk))


@pytest.mark.parametrize("metric", K.METRICS)
def test_degenerate_quantizer_rows_sort_by_id(metric):
    """step = inf: v(0) = NaN, v(c > 0) = +inf; the NaN distances sort last by row id, reported as 0x7FC00000"""
    sq = R.QUANTIZERS[3]
    rng = np.random.default_rng(9)
    codes = rng.integers(0, 2, (9000, 20), dtype=np.uint8)  # more equal keys than the candidate sort holds
    Q = rng.standard_normal((3, 20)).astype(F)
    got = _index(codes, sq, metric).search(Q, 50)
    _assert_same(got, R.search(metric, Q, sq, codes, 50))


@pytest.mark.parametrize("sq", [(0.0, 1.0, 2), (-3.0, 5.0, 17)])
def test_codes_at_or_above_levels_decode_by_the_formula(sq):
    rng = np.random.default_rng(21)
    codes = rng.integers(0, 256, (1500, 40), dtype=np.uint8)
    codes[3] = 255
    Q = (rng.standard_normal((6, 40)) * 30).astype(F)
    for metric in K.METRICS:
        _assert_same(_index(codes, sq, metric).search(Q, 25), R.search(metric, Q, sq, codes, 25))


@pytest.mark.parametrize("d", [64, 36, 33])
def test_unaligned_host_codes_and_queries(d):
    """a codes buffer offset by one byte and a query buffer offset by one element"""
    import vq_amd

    rng = np.random.default_rng(d)
    sq = R.QUANTIZERS[0]
    n, nq = 777, 5
    buf = np.zeros(n * d + 1, np.uint8)
    codes = buf[1:].reshape(n, d)
    codes[:] = _codes(n, d, sq, rng)
    assert codes.ctypes.data % 2 == 1 or codes.ctypes.data % 4 != 0
    qbuf = np.zeros(nq * d + 1, F)
    Q = qbuf[1:].reshape(nq, d)
    Q[:] = _queries(nq, d, sq, codes, rng)
    for metric in (K.EUCLIDEAN, K.COSINE):
        ix = vq_amd.ScalarIndex.from_codes(codes, _quantizer(sq), vq_amd.Distance(NAMES[metric]))
        _assert_same(ix.search(Q, 10), R.search(metric, Q, sq, codes, 10))


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("d", [64, 33])
def test_device_buffers_unaligned(off, d):
    """create_device from a codes pointer offset by `off` bytes (the index keeps its own aligned copy), search_device
    with queries and results offset by `off` elements"""
    import torch

    from vq_amd import _lib

    rng = np.random.default_rng(10 * d + off)
    sq = R.QUANTIZERS[2]
    n, nq, topk = 2001, 9, 17
    codes = _codes(n, d, sq, rng)
    Q = _queries(nq, d, sq, codes, rng)
    dev = torch.device("cuda:0")
    cb = torch.zeros(n * d + off + 8, dtype=torch.uint8, device=dev)
    cb[off:off + n * d] = torch.from_numpy(codes.ravel()).to(dev)
    torch.cuda.synchronize()
    ix = _lib.SQIndex(None, False, n, d, sq[0], sq[1], sq[2], K.COSINE, dev_src=cb.data_ptr() + off)
    try:
        assert np.array_equal(ix.codes(), codes)
        qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
        qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
        ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
        db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ix.search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off)
        _lib.synchronize()
        torch.cuda.synchronize()
        ih, dh = ib.cpu().numpy(), db.cpu().numpy()
        got = (ih[off:off + nq * topk].view(np.uint32).reshape(nq, topk), dh[off:off + nq * topk].reshape(nq, topk))
        _assert_same(got, R.search(K.COSINE, Q, sq, codes, topk))
        assert (ih[:off] == 7).all() and (ih[off + nq * topk:] == 7).all()
        assert (dh[:off] == -1).all() and (dh[off + nq * topk:] == -1).all()
    finally:
        ix.close()


@pytest.mark.parametrize("sq", R.QUANTIZERS + [(1e-40, 3e-40, 256)])
def test_index_from_rows_keeps_the_quantizers_codes(sq):
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(31)
    q = _quantizer(sq)
    span = min(sq[1], 4.0) - max(sq[0], -4.0)
    X = (max(sq[0], -4.0) - 0.1 * span + 1.2 * span * rng.random((3001, 50))).astype(F)
    X[5, 3], X[6, 0], X[7, 1] = np.nan, np.inf, -np.inf
    want = q.quantize_batch(X)
    ix = vq_amd.ScalarIndex(X, q, vq_amd.Distance.cosine())
    assert np.array_equal(ix.codes(), want)
    Q = rng.standard_normal((4, 50)).astype(F)
    _assert_same(ix.search(Q, 10), R.search(K.COSINE, Q, sq, want, 10))
    # the device form of the same create
    xd = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    h = _lib.SQIndex(None, True, 3001, 50, q._min, q._max, q.levels, K.COSINE, dev_src=xd.data_ptr())
    try:
        assert np.array_equal(h.codes(), want)
    finally:
        h.close()


def test_info_reports_the_index():
    import ctypes as C

    from vq_amd import _lib

    codes = np.zeros((5, 3), np.uint8)
    h = _lib.SQIndex(codes, False, 5, 3, -3.0, 5.0, 17, K.MANHATTAN)
    n, d, lv, m = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int()
    mn, mx = C.c_float(), C.c_float()
    _lib.check(_lib.load().vqhip_sqindex_info(h.raw, C.byref(n), C.byref(d), C.byref(m), C.byref(mn), C.byref(mx), C.byref(lv)))
    assert (n.value, d.value, m.value, mn.value, mx.value, lv.value) == (5, 3, K.MANHATTAN, -3.0, 5.0, 17)
    _lib.check(_lib.load().vqhip_sqindex_info(h.raw, None, None, None, None, None, None))
    h.close()


# ---- large shapes: equal to FlatIndex over the decoded rows ---------------------------------------------------------
def _against_flat(n, d, nq, metrics, topk=10, seed=0):
    import vq_amd

    rng = np.random.default_rng(seed)
    sq = R.QUANTIZERS[0]
    q = _quantizer(sq)
    codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    codes[n - 5:] = codes[:5]
    V = q.dequantize_batch(codes)
    assert np.array_equal(V[:64].view(np.uint32), R.decode(sq, codes[:64]).view(np.uint32))
    Q = (rng.standard_normal((nq, d)) * 0.5).astype(F)
    Q[0] = V[2]
    for metric in metrics:
        dist = vq_amd.Distance(NAMES[metric])
        got = vq_amd.ScalarIndex.from_codes(codes, q, dist).search(Q, topk)
        want = vq_amd.FlatIndex(V, dist).search(Q, topk)
        _assert_same(got, want)


def test_1m_x_128_two_batches_equals_flat():
    """300 queries over 1M rows: the [batch][n] distances are bounded by 1 GB -- 256 queries per batch"""
    _against_flat(1_000_000, 128, 300, (K.EUCLIDEAN, K.COSINE), seed=1)


@pytest.mark.parametrize("nq", [1, 64])
def test_100k_x_128_equals_flat(nq):
    _against_flat(100_000, 128, nq, K.METRICS, seed=2 + nq)


# ---- rerank -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("c", [1, 10, 1024, 4096])
def test_rerank_equals_flat_rerank_over_decoded_rows(metric, c):
    import vq_amd

    rng = np.random.default_rng(100 * metric + c)
    n, nq = 5003, 5
    for d, sq in ((33, R.QUANTIZERS[0]), (64, R.QUANTIZERS[2])):
        q = _quantizer(sq)
        codes = _codes(n, d, sq, rng)
        V = q.dequantize_batch(codes)
        Q = _queries(nq, d, sq, codes, rng)
        cand = np.stack([rng.choice(n, c, replace=False) for _ in range(nq)])
        dist = vq_amd.Distance(NAMES[metric])
        ix = vq_amd.ScalarIndex.from_codes(codes, q, dist)
        for topk in sorted({1, min(10, c), c}):
            got = ix.rerank(Q, cand, topk)
            _assert_same(got, vq_amd.FlatIndex(V, dist).rerank(Q, cand, topk))
            _assert_same(got, R.rerank(metric, Q, sq, codes, cand, topk))


def test_rerank_id_past_n_is_refused():
    import vq_amd
    from vq_amd import _lib

    codes = np.zeros((20, 4), np.uint8)
    ix = vq_amd.ScalarIndex.from_codes(codes, _quantizer(R.QUANTIZERS[0]))
    q = np.zeros((2, 4), F)
    with pytest.raises(vq_amd.InvalidParameter, match="outside"):
        ix.rerank(q, np.array([[0, 1, 20], [2, 3, 4]]), 2)
    # the library's own check: the id is flagged on the device, never read
    h = _lib.SQIndex(codes, False, 20, 4, -1.0, 1.0, 256, K.EUCLIDEAN)
    try:
        with pytest.raises(vq_amd.FfiError, match="candidate row id") as e:
            h.rerank(q, np.array([[0, 1, 0xFFFFFFFF], [2, 3, 20]], np.uint32), 2)
        assert e.value.status == _lib.ERR_INVALID_INPUT
        i, _ = h.rerank(q, np.array([[0, 1, 19], [2, 3, 4]], np.uint32), 3)
        assert i.tolist() == [[0, 1, 19], [2, 3, 4]]
    finally:
        h.close()


# ---- the rerank keyword of the other indexes ---------------------------------------------------------------------------
def _rerank_pair(X, metric):
    import vq_amd

    sq = (-4.0, 4.0, 256)
    q = _quantizer(sq)
    dist = vq_amd.Distance(NAMES[metric])
    six = vq_amd.ScalarIndex(X, q, dist)
    return six, vq_amd.FlatIndex(q.dequantize_batch(q.quantize_batch(X)), dist)


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_pq_search_rerank_through_scalar_index(metric):
    import vq_amd
    from vq_amd.store import PQIndex

    rng = np.random.default_rng(11)
    n, m, k, sd = 6000, 4, 64, 6
    cb = rng.standard_normal((m, k, sd)).astype(F)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    X = rng.standard_normal((n, m * sd)).astype(F)
    Q = rng.standard_normal((7, m * sd)).astype(F)
    six, flat = _rerank_pair(X, metric)
    idx = PQIndex(cb, codes, vq_amd.Distance.squared_euclidean())
    _assert_same(idx.search(Q, 10, rerank=six, candidates=80), idx.search(Q, 10, rerank=flat, candidates=80))
    _assert_same(idx.search(Q, 10, rerank=six), idx.search(Q, 10, rerank=flat))
    pq = vq_amd.ProductQuantizer(X[:3000], 4, 16, 3, vq_amd.Distance.euclidean(), 5)
    pc = pq.encode(X)
    _assert_same(pq.search(pc, Q, 5, rerank=six, candidates=64), pq.search(pc, Q, 5, rerank=flat, candidates=64))


@pytest.mark.parametrize("residual", [False, True])
def test_ivf_search_rerank_through_scalar_index(residual):
    import vq_amd

    rng = np.random.default_rng(12)
    n, d = 6000, 32
    X = rng.standard_normal((n, d)).astype(F)
    coarse = X[rng.choice(n, 24, replace=False)]
    cb = (rng.standard_normal((8, 64, 4)) * 0.5).astype(F)
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean(), residual=residual)
    ix.add(X)
    six, flat = _rerank_pair(X, K.EUCLIDEAN)
    Q = rng.standard_normal((12, d)).astype(F)
    for nprobe, topk, cand in ((3, 10, None), (1, 50, 400), (24, 5, 64)):
        _assert_same(ix.search(Q, topk=topk, nprobe=nprobe, rerank=six, candidates=cand),
                     ix.search(Q, topk=topk, nprobe=nprobe, rerank=flat, candidates=cand))
    ix.close()


def test_binary_search_rerank_through_scalar_index():
    import vq_amd

    rng = np.random.default_rng(51)
    X = rng.standard_normal((4000, 64)).astype(F)
    Q = rng.standard_normal((12, 64)).astype(F)
    ix = vq_amd.BinaryIndex(X)
    six, flat = _rerank_pair(X, K.COSINE)
    _assert_same(ix.search(Q, 10, rerank=six, candidates=80), ix.search(Q, 10, rerank=flat, candidates=80))
    _assert_same(ix.search(Q, 10, rerank=six), ix.search(Q, 10, rerank=flat))


# ---- the device form and the file -----------------------------------------------------------------------------------
def test_search_device_with_torch_buffers_equals_search():
    import torch

    import vq_amd

    rng = np.random.default_rng(61)
    sq = R.QUANTIZERS[0]
    codes = _codes(30_000, 96, sq, rng)
    Q = _queries(40, 96, sq, codes, rng)
    ix = _index(codes, sq, K.EUCLIDEAN)
    want = ix.search(Q, 17)
    qd = torch.from_numpy(Q).cuda()
    idx = torch.empty((40, 17), dtype=torch.int32, device="cuda")
    dist = torch.empty((40, 17), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(qd.data_ptr(), 40, 17, idx.data_ptr(), dist.data_ptr())
    vq_amd._lib.synchronize()
    torch.cuda.synchronize()
    _assert_same((idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want)


def test_save_load_of_an_index_built_from_rows(tmp_path):
    import vq_amd

    rng = np.random.default_rng(71)
    q = _quantizer(R.QUANTIZERS[2])
    X = (rng.standard_normal((2500, 19)) * 2).astype(F)
    ix = vq_amd.ScalarIndex(X, q, vq_amd.Distance.manhattan())
    ix.save(tmp_path / "rows.vqsq")
    back = vq_amd.ScalarIndex.load(tmp_path / "rows.vqsq")
    assert np.array_equal(back.codes(), q.quantize_batch(X))
    assert back.distance == ix.distance and repr(back.quantizer) == repr(q)
    Q = rng.standard_normal((5, 19)).astype(F)
    _assert_same(back.search(Q, 10), ix.search(Q, 10))
    _assert_same(back.search(Q, 10), R.search(K.MANHATTAN, Q, R.QUANTIZERS[2], back.codes(), 10))
