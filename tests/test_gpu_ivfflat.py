"""Inverted-file flat search on the MI355X (vq_amd.IVFFlatIndex, vqhip_ivfflat_*, vq_amd/csrc/k_ivfflat.hip) against the
numpy statement of include/vqhip.h (tests/ref_ivfflat.py): indices equal, distances equal as uint32 bits.  All five
metrics, f32 and f16 rows, dim 1 / 5 / 33 / 128 / 200, nlist 1 / 7 / 256 / 4096, nprobe 1 / 5 / nlist, topk 1 / 10 / 256 /
1024; nprobe == nlist against FlatIndex.search (one and several batches of the distance workspace); probe against
FlatIndex over the centroids; 1, 7, 129 and 1500 queries, queries that share every list and queries that share none, and
batches on both sides of the count (16 queries per list) from which a list goes to the tile kernel and of its 128-query
tile; empty lists, one list holding every row, rows in an order unrelated to their lists, duplicate rows, NaN / inf /
subnormal rows and queries, zero norms under the cosines, cuts too dense for the LDS sort, padding, an add after a
search; the device form; and one 1M x 128 case."""
import numpy as np
import pytest

import ref_ivfflat as R
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
DTYPES = [np.float32, np.float16]


def _same(got, want, rows=None):
    gi, gd = got
    wi, wd = want
    if rows is not None:
        gi, gd, wi, wd = gi[rows], gd[rows], wi[rows], wd[rows]
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _case(rng, n, nlist, dim, dtype, nq):
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)  # rows in an order unrelated to their lists
    rows = (coarse[lists] + F(0.5) * rng.standard_normal((n, dim)).astype(F)).astype(dtype)
    rows[n - 7:] = rows[:7]  # duplicate rows ...
    lists[n - 7:] = lists[:7]  # ... in the same lists: ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    Q[0] = coarse[min(3, nlist - 1)]
    return coarse, lists, rows, Q


def _index(coarse, metric, lists, rows, pieces=1):
    import vq_amd

    ix = vq_amd.IVFFlatIndex(coarse, vq_amd.Distance(NAMES[metric]), rows.dtype)
    for a in np.array_split(np.arange(len(lists)), pieces):
        ix.add_rows(lists[a], rows[a])
    return ix


SHAPES = [
    (3001, 7, 128),
    (2500, 256, 33),
    (2000, 1, 5),
    (6000, 4096, 1),   # many lists, most of them tiny or empty
    (1500, 7, 200),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(metric, shape, dtype):
    n, nlist, dim = shape
    rng = np.random.default_rng(n + nlist + metric)
    coarse, lists, rows, Q = _case(rng, n, nlist, dim, dtype, nq=40)  # (40 queries: lists on both kernels)
    ix = _index(coarse, metric, lists, rows, pieces=3)
    for nprobe in sorted({1, min(5, nlist), min(nlist, 1024)}):
        for topk in (1, 10, 256, 1024):
            _same(ix.search(Q, topk=topk, nprobe=nprobe), R.search(metric, coarse, lists, rows, Q, nprobe, topk))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", K.METRICS)
def test_all_lists_equal_flat_index(metric, dtype):
    import vq_amd

    rng = np.random.default_rng(7 + metric)
    coarse, lists, rows, Q = _case(rng, 20000, 64, 48, dtype, nq=33)
    ix = _index(coarse, metric, lists, rows)
    flat = vq_amd.FlatIndex(rows, vq_amd.Distance(NAMES[metric]))
    for topk in (1, 100):
        _same(ix.search(Q, topk=topk, nprobe=64), flat.search(Q, topk))
    ix.close()


def test_all_lists_equal_flat_index_several_batches():
    """1024 queries over 300000 rows: 1.2 GB of distances at nprobe == nlist, two batches of the workspace"""
    import vq_amd

    rng = np.random.default_rng(11)
    n, nlist, dim, nq = 300000, 32, 16, 1024
    coarse, lists, rows, Q = _case(rng, n, nlist, dim, np.float16, nq)
    ix = _index(coarse, K.EUCLIDEAN, lists, rows)
    flat = vq_amd.FlatIndex(rows, vq_amd.Distance.euclidean())
    _same(ix.search(Q, topk=10, nprobe=nlist), flat.search(Q, 10))
    ix.close()


@pytest.mark.parametrize("metric", K.METRICS)
def test_probe_is_flat_search_over_centroids(metric):
    import vq_amd

    rng = np.random.default_rng(3 + metric)
    coarse, lists, rows, Q = _case(rng, 500, 300, 24, np.float32, nq=50)
    ix = _index(coarse, metric, lists, rows)
    flat = vq_amd.FlatIndex(coarse, vq_amd.Distance(NAMES[metric]))
    for nprobe in (1, 8, 300):
        got = ix.probe(Q, nprobe)
        assert np.array_equal(got, flat.search(Q, nprobe)[0])
        assert np.array_equal(got, R.probe(metric, coarse, Q, nprobe))
    ix.close()


@pytest.mark.parametrize("nq", [1, 7, 129, 1500])
def test_query_counts(nq):
    rng = np.random.default_rng(nq)
    coarse, lists, rows, Q = _case(rng, 5000, 24, 40, np.float32, nq)
    ix = _index(coarse, K.SQUARED_EUCLIDEAN, lists, rows)
    for nprobe in (1, 6):
        _same(ix.search(Q, topk=20, nprobe=nprobe), R.search(K.SQUARED_EUCLIDEAN, coarse, lists, rows, Q, nprobe, 20))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 127, 128, 129, 300])
def test_every_query_probes_the_same_lists(nq, dtype):
    """nq queries beside one centroid: the lists they probe are each probed by all nq of them -- below 16 the positions
    kernel computes every pair, from 16 on the tile kernel, in one, two or three tiles of 128 queries"""
    rng = np.random.default_rng(100 + nq)
    coarse, lists, rows, _ = _case(rng, 4000, 12, 36, dtype, 1)
    Q = (coarse[5] + F(1e-3) * rng.standard_normal((nq, 36)).astype(F)).astype(F)
    ix = _index(coarse, K.EUCLIDEAN, lists, rows)
    P = ix.probe(Q, 3)
    assert np.all(P == P[0])
    _same(ix.search(Q, topk=30, nprobe=3), R.search(K.EUCLIDEAN, coarse, lists, rows, Q, 3, 30))
    ix.close()


def test_no_two_queries_share_a_list():
    rng = np.random.default_rng(55)
    coarse, lists, rows, _ = _case(rng, 6000, 200, 20, np.float32, 1)
    Q = coarse.copy()  # query l probes list l alone
    ix = _index(coarse, K.SQUARED_EUCLIDEAN, lists, rows)
    assert np.array_equal(ix.probe(Q, 1)[:, 0], np.arange(200))
    _same(ix.search(Q, topk=40, nprobe=1), R.search(K.SQUARED_EUCLIDEAN, coarse, lists, rows, Q, 1, 40))
    ix.close()


def test_kernel_variants_give_the_same_bits():
    """the same query alone (the positions kernel) and among 39 copies of itself (the tile kernel)"""
    rng = np.random.default_rng(77)
    coarse, lists, rows, Q = _case(rng, 3000, 5, 67, np.float32, 3)
    for metric in K.METRICS:
        ix = _index(coarse, metric, lists, rows)
        alone = ix.search(Q[1:2], topk=200, nprobe=2)
        many = ix.search(np.repeat(Q[1:2], 40, axis=0), topk=200, nprobe=2)
        for j in range(40):
            _same((many[0][j:j + 1], many[1][j:j + 1]), alone)
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", K.METRICS)
def test_data_corners(metric, dtype):
    rng = np.random.default_rng(40 + metric)
    dim = 12
    coarse, lists, rows, Q = _case(rng, 4000, 16, dim, dtype, nq=24)
    lists[np.isin(lists, [2, 5, 11])] = 7  # empty lists, one large list
    sp = K.special_rows(dim, rng)
    with np.errstate(over="ignore"):
        rows[50:50 + len(sp)] = sp.astype(dtype)  # NaN, +-inf, subnormals, a zero-norm row
    Q[1:1 + len(sp)] = sp  # ... and a zero-norm query
    rows[100:900] = rows[5]  # heavy ties
    for nprobe in (1, 3, 16):
        for topk in (10, 256):
            ix = _index(coarse, metric, lists, rows)
            _same(ix.search(Q, topk=topk, nprobe=nprobe), R.search(metric, coarse, lists, rows, Q, nprobe, topk))
            ix.close()
    one = np.full_like(lists, 9)  # one list holding every row
    ix = _index(coarse, metric, one, rows)
    for nprobe in (1, 4):
        _same(ix.search(Q, topk=50, nprobe=nprobe), R.search(metric, coarse, one, rows, Q, nprobe, 50))
    ix.close()


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.MANHATTAN, K.COSINE])
def test_dense_cut_radix_select(metric):
    """more than 8192 tied candidates at the cut: the exact radix select over (key, row id) (k_adc_topk, topk.hpp)"""
    rng = np.random.default_rng(90 + metric)
    n, nlist, dim = 30000, 3, 10
    coarse, _, rows, Q = _case(rng, n, nlist, dim, np.float32, nq=20)
    lists = (np.arange(n) % nlist).astype(np.uint32)  # 10000 rows per list
    rows[1000:28000] = rows[3]  # 27000 duplicates: 9000 per list
    Q[0] = rows[3]
    Q[1, 2] = np.nan  # every distance NaN
    Q[2, 0] = np.inf
    ix = _index(coarse, metric, lists, rows)
    for nprobe in (1, 3):
        for topk in (5, 1024):
            _same(ix.search(Q, topk=topk, nprobe=nprobe), R.search(metric, coarse, lists, rows, Q, nprobe, topk))
    ix.close()


def test_padding_past_the_probed_rows():
    rng = np.random.default_rng(12)
    coarse, lists, rows, Q = _case(rng, 300, 40, 9, np.float32, nq=20)
    lists[lists == 3] = 4  # Q[0] is centroid 3: its nearest list is empty
    ix = _index(coarse, K.COSINE, lists, rows)
    for nprobe in (1, 2):
        got = ix.search(Q, topk=100, nprobe=nprobe)
        _same(got, R.search(K.COSINE, coarse, lists, rows, Q, nprobe, 100))
        assert (got[0] == R.PAD_ID).any() and np.isposinf(got[1][got[0] == R.PAD_ID]).all()
    assert (ix.search(Q[:1], topk=5, nprobe=1)[0] == R.PAD_ID).all()
    ix.close()


def test_add_after_search_rebuilds():
    rng = np.random.default_rng(13)
    coarse, lists, rows, Q = _case(rng, 3000, 10, 17, np.float16, nq=30)
    ix = _index(coarse, K.MANHATTAN, lists[:1000], rows[:1000])
    _same(ix.search(Q, topk=10, nprobe=3), R.search(K.MANHATTAN, coarse, lists[:1000], rows[:1000], Q, 3, 10))
    assert np.array_equal(ix.add_rows(lists[1000:], rows[1000:]), np.arange(1000, 3000))
    _same(ix.search(Q, topk=10, nprobe=3), R.search(K.MANHATTAN, coarse, lists, rows, Q, 3, 10))
    ix.close()


def test_add_assigns_the_nearest_list():
    import vq_amd

    rng = np.random.default_rng(14)
    coarse, _, rows, Q = _case(rng, 2000, 9, 21, np.float32, nq=5)
    ix = vq_amd.IVFFlatIndex(coarse)
    ix.add(rows)
    from vq_amd.ivf import _nearest_lists

    assert np.array_equal(ix.list_ids, _nearest_lists(coarse, rows, K.EUCLIDEAN))
    _same(ix.search(Q, topk=10, nprobe=9), vq_amd.FlatIndex(rows).search(Q, 10))
    ix.close()


def test_device_form():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(15)
    coarse, lists, rows, Q = _case(rng, 4000, 20, 32, np.float32, nq=70)
    ix = _index(coarse, K.EUCLIDEAN, lists, rows)
    dq = torch.from_numpy(Q).cuda()
    di = torch.empty((70, 15), dtype=torch.int32, device="cuda")
    dd = torch.empty((70, 15), dtype=torch.float32, device="cuda")
    ix.search_device(dq.data_ptr(), 70, 15, di.data_ptr(), dd.data_ptr(), nprobe=4)
    torch.cuda.synchronize()
    from vq_amd import _lib

    _lib.synchronize()
    _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), R.search(K.EUCLIDEAN, coarse, lists, rows, Q, 4, 15))
    ix.close()


def test_one_million_rows():
    """1M x 128 clustered, nlist 1024, nprobe 32, 1024 queries searched; the statement checked for a fixed sample of 64"""
    rng = np.random.default_rng(16)
    n, nlist, dim, nq = 1_000_000, 1024, 128, 1024
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = coarse[lists] + F(0.6) * rng.standard_normal((n, dim), dtype=F)
    Q = coarse[rng.integers(0, nlist, nq)] + F(0.6) * rng.standard_normal((nq, dim), dtype=F)
    ix = _index(coarse, K.EUCLIDEAN, lists, rows)
    got = ix.search(Q, topk=10, nprobe=32)
    ix.close()
    sample = list(range(0, nq, 16))
    _same(got, R.search(K.EUCLIDEAN, coarse, lists, rows, Q, 32, 10, queries=sample), rows=sample)
