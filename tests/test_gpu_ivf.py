"""Inverted-file PQ search on the MI355X (vq_amd.IVFPQIndex, vqhip_ivfpq_*, vq_amd/csrc/k_ivf.hip) against the numpy
statement of include/vqhip.h (tests/ref_ivf.py): indices equal, distances equal as uint32 bits.  All three metrics,
one- and two-byte codes, m * k at the table limit, topk 1 / 10 / 256 / 1024, nprobe 1 / some / nlist, nlist 1, 7, 256
and 4096; empty lists, one list holding every row, rows in an order unrelated to their lists, several adds, duplicate
codes, NaN / inf queries, cuts too dense for the LDS sort (the exact radix select), padding; nprobe == nlist against PQIndex.search on both sides of the one-scan ADC schedule;
probe against FlatIndex; rerank; the device form; and one 1M x 128 case."""
import numpy as np
import pytest

import ref_ivf as R
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)
NAMES = ["squared_euclidean", "euclidean", "manhattan"]


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _case(rng, n, nlist, m, k, sd, nq=8):
    X_lists = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    codes[n - 7:] = codes[:7]  # duplicate codes: ties by row id
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    Q[0] = X_lists[min(3, nlist - 1)]
    return X_lists, cb, lists, codes, Q


def _index(coarse, cb, metric, lists, codes):
    import vq_amd

    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance(NAMES[metric]))
    ix.add_codes(lists, codes)
    return ix


SHAPES = [
    (3001, 7, 8, 256, 4),     # one-byte codes in 8-byte words
    (2500, 256, 4, 300, 3),   # two-byte codes
    (2000, 1, 3, 16, 5),      # one list; m not a multiple of 8
    (6000, 4096, 8, 64, 2),   # many lists, most of them tiny or empty
    (1500, 7, 150, 256, 1),   # m * k = 38400, the table limit
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(orc, metric, shape):
    n, nlist, m, k, sd = shape
    rng = np.random.default_rng(n + nlist + metric)
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd)
    ix = _index(coarse, cb, metric, lists, codes)
    for nprobe in sorted({1, min(5, nlist), min(nlist, 1024)}):
        for topk in (1, 10, 256, 1024):
            want = R.search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk)
            _same(ix.search(Q, topk=topk, nprobe=nprobe), want)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_data_corners(orc, metric):
    rng = np.random.default_rng(40 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 4000, 16, 8, 256, 2, nq=6)
    lists[np.isin(lists, [2, 5, 11])] = 7  # empty lists, one large list
    Q[1, 3] = np.nan
    Q[2, 0] = np.inf
    Q[3, -1] = -np.inf
    codes[100:900] = codes[5]  # heavy ties (the cut's sort: S(q) holds at most 4000 rows here)
    for nprobe in (1, 3, 16):
        for topk in (10, 256):
            ix = _index(coarse, cb, metric, lists, codes)
            want = R.search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk)
            _same(ix.search(Q, topk=topk, nprobe=nprobe), want)
            ix.close()
    # one list holding every row
    one = np.full_like(lists, 9)
    ix = _index(coarse, cb, metric, one, codes)
    for nprobe in (1, 4):
        _same(ix.search(Q, topk=50, nprobe=nprobe), R.search(orc, metric, coarse, cb, one, codes, Q, nprobe, 50))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_dense_cut_radix_select(orc, metric):
    """cuts of more than 8192 positions go to k_adc_topk (topk.hpp), the exact radix select over (key, row id).  Every probed
    list here holds about 10000 rows, so |S(q)| > 8192 at every nprobe, and each query puts more than 8192 of them in one
    histogram bin: a NaN or +-inf component (all distances NaN / inf: the range collapses, every position in one bin), a
    query on a block of 27000 duplicate rows (more than 8192 equal smallest distances per list), and all codes equal."""
    rng = np.random.default_rng(90 + metric)
    n, nlist, m, k, sd = 30000, 3, 8, 64, 2
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd, nq=6)
    lists = (np.arange(n) % nlist).astype(np.uint32)  # 10000 rows per list
    dup = rng.permutation(n)[:27000]  # duplicates spread over every list (~9000 each), in no row order
    codes[dup] = codes[1]
    Q[1, 0] = np.nan
    Q[2, -1] = np.inf
    Q[3, 3] = -np.inf
    Q[4] = np.concatenate([cb[s, codes[1, s]] for s in range(m)])  # D = 0 on every duplicate
    same = np.broadcast_to(codes[7], codes.shape).copy()  # all codes equal
    for c in (codes, same):
        ix = _index(coarse, cb, metric, lists, c)
        for nprobe in (1, 3):
            for topk in (1, 1024):
                want = R.search(orc, metric, coarse, cb, lists, c, Q, nprobe, topk)
                _same(ix.search(Q, topk=topk, nprobe=nprobe), want)
        ix.close()


def test_adds_in_parts_equal_one_add_and_padding(orc):
    import vq_amd

    rng = np.random.default_rng(11)
    coarse, cb, lists, codes, Q = _case(rng, 3000, 32, 8, 256, 2, nq=10)
    whole = _index(coarse, cb, K.EUCLIDEAN, lists, codes)
    parts = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean())
    parts.add_codes(lists[:1000], codes[:1000])
    a = parts.search(Q, topk=20, nprobe=4)  # the device state exists before the next adds
    _same(a, R.search(orc, K.EUCLIDEAN, coarse, cb, lists[:1000], codes[:1000], Q, 4, 20))
    parts.add_codes(lists[1000:1001], codes[1000:1001])
    parts.add_codes(lists[1001:], codes[1001:])
    for nprobe, topk in ((4, 20), (1, 300), (32, 1024)):
        got = parts.search(Q, topk=topk, nprobe=nprobe)
        _same(got, whole.search(Q, topk=topk, nprobe=nprobe))
        _same(got, R.search(orc, K.EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, topk))
    # a query whose probed lists hold fewer than topk rows is padded with (0xFFFFFFFF, +inf)
    sizes = parts.list_sizes()
    assert np.array_equal(sizes, np.bincount(lists, minlength=32).astype(np.uint64))
    i, d = parts.search(Q, topk=1024, nprobe=1)
    P = parts.probe(Q, nprobe=1)
    for j in range(Q.shape[0]):
        s = int(sizes[P[j, 0]])
        assert s < 1024 and np.all(i[j, s:] == R.PAD_ID) and np.all(d[j, s:].view(np.uint32) == R.INF_BITS)
        assert np.all(i[j, :s] != R.PAD_ID) and np.all(lists[i[j, :s]] == P[j, 0])
    whole.close()
    parts.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [20000, 40000])
def test_all_lists_equal_pq_index_search(metric, n):
    import vq_amd
    from vq_amd.store import PQIndex

    rng = np.random.default_rng(n + metric)
    coarse, cb, lists, codes, Q = _case(rng, n, 64, 8, 256, 4, nq=40)
    ix = _index(coarse, cb, metric, lists, codes)
    pq = PQIndex(cb, codes, vq_amd.Distance(NAMES[metric]))
    for topk in (10, 300):
        _same(ix.search(Q, topk=topk, nprobe=64), pq.search(Q, topk))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_probe_equals_flat_search(metric):
    import vq_amd

    rng = np.random.default_rng(70 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 500, 256, 4, 16, 8, nq=33)
    coarse[10] = coarse[20]  # equal centroids: ties by list id
    Q[5] = coarse[10]
    ix = _index(coarse, cb, metric, lists, codes)
    flat = vq_amd.FlatIndex(coarse, vq_amd.Distance(NAMES[metric]))
    for nprobe in (1, 7, 256):
        got = ix.probe(Q, nprobe=nprobe)
        assert np.array_equal(got, flat.search(Q, nprobe)[0])
        assert np.array_equal(got, R.probe(metric, coarse, Q, nprobe))
    ix.close()


def test_rerank_equals_flat_rerank_of_hits():
    import vq_amd

    rng = np.random.default_rng(12)
    n, d = 6000, 32
    X = rng.standard_normal((n, d)).astype(F)
    coarse = X[rng.choice(n, 24, replace=False)]
    cb = rng.standard_normal((8, 64, 4)).astype(F)
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean())
    ix.add(X)
    flat = vq_amd.FlatIndex(X, vq_amd.Distance.euclidean())
    Q = rng.standard_normal((12, d)).astype(F)
    for nprobe, topk, cand in ((3, 10, None), (1, 50, 400), (24, 5, 64)):
        got = ix.search(Q, topk=topk, nprobe=nprobe, rerank=flat, candidates=cand)
        c = min(4 * topk, 1024, n) if cand is None else cand
        hits, _ = ix.search(Q, topk=c, nprobe=nprobe)
        for j in range(Q.shape[0]):
            r = int((hits[j] != R.PAD_ID).sum())
            t = min(topk, r)
            wi, wd = flat.rerank(Q[j:j + 1], hits[j:j + 1, :r], t)
            assert np.array_equal(got[0][j, :t], wi[0]) and np.array_equal(got[1][j, :t].view(np.uint32), wd[0].view(np.uint32))
            assert np.all(got[0][j, t:] == R.PAD_ID) and np.all(np.isinf(got[1][j, t:]))
    ix.close()
    # a query whose probed list holds fewer rows than the candidates keeps its padding: five rows around a far centroid
    X[:5] = F(50.0) + rng.standard_normal((5, d)).astype(F) * F(0.1)
    coarse = np.concatenate([np.full((1, d), 50.0, F), coarse[1:]])
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean())
    ix.add(X)
    flat = vq_amd.FlatIndex(X, vq_amd.Distance.euclidean())
    q = coarse[:1]
    assert int(ix.probe(q, 1)[0, 0]) == 0 and int(ix.list_sizes()[0]) == 5
    for topk, cand in ((10, 40), (3, 40), (5, 5)):
        i, dd = ix.search(q, topk=topk, nprobe=1, rerank=flat, candidates=cand)
        t = min(topk, 5)
        wi, wd = flat.rerank(q, np.arange(5, dtype=np.uint32)[None, :], t)
        assert np.array_equal(i[0, :t], wi[0]) and np.array_equal(dd[0, :t].view(np.uint32), wd[0].view(np.uint32))
        assert np.all(i[0, t:] == R.PAD_ID) and np.all(dd[0, t:].view(np.uint32) == R.INF_BITS)
    ix.close()


def test_search_device_equals_search():
    import torch

    rng = np.random.default_rng(13)
    coarse, cb, lists, codes, Q = _case(rng, 50000, 128, 8, 256, 4, nq=300)
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes)
    want = ix.search(Q, topk=64, nprobe=9)
    dq = torch.from_numpy(Q).cuda()
    di = torch.empty((300, 64), dtype=torch.int32, device="cuda")
    dd = torch.empty((300, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), 300, 64, di.data_ptr(), dd.data_ptr(), nprobe=9)
    from vq_amd import _lib

    _lib.load().vqhip_synchronize()
    _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), want)
    ix.close()


def test_large_1m_x_128(orc):
    rng = np.random.default_rng(2024)
    n, nlist, m, k, sd, nq = 1 << 20, 1024, 8, 256, 16, 256
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    w = rng.gamma(2.0, 1.0, nlist)  # uneven lists, as k-means leaves them
    lists = rng.choice(nlist, n, p=w / w.sum()).astype(np.uint32)
    codes = rng.integers(0, k, (n, m), dtype=np.uint8)
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes)
    got = ix.search(Q, topk=10, nprobe=32)
    _same(got, R.search(orc, K.EUCLIDEAN, coarse, cb, lists, codes, Q, 32, 10))
    ix.close()
