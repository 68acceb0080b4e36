"""Inverted-file binary search on the MI355X (vq_amd.IVFBinaryIndex, vqhip_ivfbin_*, vq_amd/csrc/k_ivfbin.hip).  Every
comparison is equality of indices and of distance bits: against the numpy statement of include/vqhip.h
(tests/ref_ivfbin.py) and against BinaryIndex at nprobe == nlist (the identity).  The three metrics and the (low, high)
pairs of tests/test_binary_host.py; W = 4 / 3 / 6 / 1 words (the 16-, 4- and 8-byte loaders), one bit in the last word,
one pad bit, dim 1, one word past the 32-word LDS chunk of the tile kernel, the largest row; batches on both sides of the
count (16 queries per list) from which a list goes to the tile kernel and of its 128-query tile (G), on each loader;
list lengths around the 64-row tile (R); add_rows / add; padding; the device form; rerank=; save / load; determinism."""
import functools

import numpy as np
import pytest

import ref_binary as B
import ref_ivfbin as R
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
G, ROWS = 128, 64  # the tile kernel's query tile and row tile
BQ = (0.0, 0, 1)


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _cut(want, topk):
    return want[0][:, :topk], want[1][:, :topk]


def _case(rng, n, nlist, dim, nq):
    """f32 rows (binarised by the test's quantizer) in an order unrelated to their lists, duplicates in the same list;
    queries with NaN and -0.0 elements"""
    coarse = rng.standard_normal((nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = rng.standard_normal((n, dim)).astype(F)
    rows[n - 7:] = rows[:7]    # duplicate rows ...
    lists[n - 7:] = lists[:7]  # ... in the same lists: ties by row id
    Q = rng.standard_normal((nq, dim)).astype(F)
    Q[0] = coarse[min(3, nlist - 1)]
    if nq > 4:
        Q[1, 0] = np.nan   # (probes lists 0 .. nprobe-1: every coarse distance is NaN)
        Q[2, dim // 2] = -0.0
        Q[3, :] = -0.0
    return coarse, lists, rows, Q


def _words(rows, thr):
    return B.pack(B.bits_f32(rows, thr))


def _index(coarse, metric, lists, words, bq=BQ, pieces=1, coarse_metric=K.EUCLIDEAN):
    import vq_amd

    ix = vq_amd.IVFBinaryIndex(coarse, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]), vq_amd.Distance(NAMES[coarse_metric]))
    for a in np.array_split(np.arange(len(lists)), pieces):
        ix.add_packed(lists[a], words[a])
    return ix


def _want(metric, coarse, lists, bq, words, dim, Q, nprobe, topk, coarse_metric=K.EUCLIDEAN, P=None):
    return R.search(metric, coarse_metric, coarse, lists, bq, words, dim, Q, nprobe, topk, P=P)


SHAPES = [
    (3001, 7, 128),    # W = 4, 16-byte loader
    (2500, 256, 96),   # W = 3, 4-byte loader
    (2000, 7, 192),    # W = 6, 8-byte loader
    (2000, 1, 5),      # W = 1, massive ties in H
    (1500, 7, 33),     # one bit in the last word
    (1500, 7, 31),     # one word, one pad bit
    (6000, 4096, 1),   # mostly empty lists
    (1500, 7, 1056),   # W = 33: one word past the tile kernel's 32-word chunk
    (600, 3, 8192),    # largest table and row
]
THRESHOLDS = {(0, 1): 0.0, (0, 255): 0.0, (254, 255): -0.5, (3, 200): 0.25}


@functools.lru_cache(maxsize=None)
def _shape_case(shape):
    """one case per shape, shared by every metric and (low, high): the data and the probes (the reference's costly part)"""
    n, nlist, dim = shape
    rng = np.random.default_rng(n + nlist + dim)
    coarse, lists, rows, Q = _case(rng, n, nlist, dim, nq=40)  # (40 queries: lists on both kernels)
    probes = {p: R.probe(K.EUCLIDEAN, coarse, Q, p) for p in sorted({1, min(5, nlist), min(nlist, 1024)})}
    return coarse, lists, rows, Q, probes


@pytest.mark.parametrize("low,high", R.LOW_HIGH)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(metric, shape, low, high):
    n, nlist, dim = shape
    coarse, lists, rows, Q, probes = _shape_case(shape)
    bq = (THRESHOLDS[(low, high)], low, high)
    words = _words(rows, bq[0])
    ix = _index(coarse, metric, lists, words, bq, pieces=3)
    kmax = min(n, 1024)
    for nprobe, P in probes.items():
        assert np.array_equal(ix.probe(Q, nprobe), P)
        want = _want(metric, coarse, lists, bq, words, dim, Q, nprobe, kmax, P=P)
        for topk in (1, 10, 256, kmax):
            _same(ix.search(Q, topk=topk, nprobe=nprobe), _cut(want, topk))
    ix.close()


@pytest.mark.parametrize("metric", R.METRICS)
def test_all_lists_equal_binary_index(metric):
    """identity 1"""
    import vq_amd

    rng = np.random.default_rng(9 + metric)
    coarse, lists, rows, Q = _case(rng, 6000, 64, 160, nq=33)
    bq = (0.1, 2, 9)
    words = _words(rows, bq[0])
    ix = _index(coarse, metric, lists, words, bq)
    bx = vq_amd.BinaryIndex.from_packed(words, 160, ix.quantizer, ix.distance)
    for topk in (1, 100):
        _same(ix.search(Q, topk=topk, nprobe=64), bx.search(Q, topk))
    ix.close()


def test_all_lists_equal_binary_index_two_query_batches():
    """1030 queries: more than the 1024 of a batch"""
    import vq_amd

    rng = np.random.default_rng(11)
    coarse, lists, rows, Q = _case(rng, 5000, 16, 40, nq=1030)
    words = _words(rows, 0.0)
    ix = _index(coarse, B.EUC, lists, words)
    bx = vq_amd.BinaryIndex.from_packed(words, 40, ix.quantizer, ix.distance)
    _same(ix.search(Q, topk=10, nprobe=16), bx.search(Q, 10))
    ix.close()


@pytest.mark.parametrize("topk", [1, 10, 1024])
def test_heavy_ties_go_to_the_lowest_ids(topk):
    """dim 3: at most 4 values of H over 5000 rows in two lists; every reported row is the lowest id among its equals"""
    rng = np.random.default_rng(5)
    coarse = np.array([[-1, -1, -1], [1, 1, 1], [40, 40, 40]], F)
    rows = rng.standard_normal((5000, 3)).astype(F)
    lists = (rng.random(5000) < 0.5).astype(np.uint32)  # lists 0 and 1; list 2 stays empty
    words = _words(rows, 0.0)
    Q = rng.standard_normal((20, 3)).astype(F)
    ix = _index(coarse, B.MAN, lists, words)
    for nprobe in (1, 2, 3):
        got = ix.search(Q, topk=topk, nprobe=nprobe)
        _same(got, _want(B.MAN, coarse, lists, BQ, words, 3, Q, nprobe, topk))
        P = ix.probe(Q, nprobe)
        H = B.hamming(B.pack(B.bits_f32(Q, 0.0)), words)
        for j in range(Q.shape[0]):
            S = np.flatnonzero(np.isin(lists, P[j]))
            h_last = H[j, got[0][j, -1]]
            # every member with a smaller H is reported, and of the last H the lowest ids
            assert set(S[H[j, S] < h_last]) <= set(got[0][j].tolist())
            at = S[H[j, S] == h_last]
            took = got[0][j][H[j, got[0][j]] == h_last]
            assert np.array_equal(took, at[:took.size])
    ix.close()


@pytest.mark.parametrize("dim", [128, 96, 192])  # the 16-, 4- and 8-byte loaders
@pytest.mark.parametrize("nq", [1, 15, 16, 17, G - 1, G, G + 1, 300])
def test_every_query_probes_the_same_lists(nq, dim):
    """nq queries beside one centroid: the lists they probe are each probed by all nq of them -- below 16 the positions
    kernel computes every pair, from 16 on the tile kernel, in one, two or three tiles of 128 queries"""
    rng = np.random.default_rng(100 + nq)
    coarse, lists, rows, _ = _case(rng, 4000, 12, dim, 1)
    words = _words(rows, 0.0)
    Q = (coarse[5] + F(0.3) * rng.standard_normal((nq, dim)).astype(F)).astype(F)
    ix = _index(coarse, B.EUC, lists, words)
    P = ix.probe(Q, 1)
    assert np.all(P == 5)
    _same(ix.search(Q, topk=30, nprobe=1), _want(B.EUC, coarse, lists, BQ, words, dim, Q, 1, 30))
    ix.close()


@pytest.mark.parametrize("dim", [256, 97, 70])  # the 16-, 4- and 8-byte loaders
def test_kernel_variants_give_the_same_bits(dim):
    """the same query alone (the positions kernel) and among 39 copies of itself (the tile kernel)"""
    rng = np.random.default_rng(77)
    coarse, lists, rows, Q = _case(rng, 3000, 5, dim, 3)
    words = _words(rows, 0.0)
    for metric in R.METRICS:
        ix = _index(coarse, metric, lists, words)
        alone = ix.search(Q[1:2], topk=200, nprobe=2)
        many = ix.search(np.repeat(Q[1:2], 40, axis=0), topk=200, nprobe=2)
        for j in range(40):
            _same((many[0][j:j + 1], many[1][j:j + 1]), alone)
        ix.close()


@pytest.mark.parametrize("nq", [3, 40])  # the positions kernel, the tile kernel
def test_list_lengths_around_the_row_tile(nq):
    """lists of R - 1, R, R + 1, 1, 0 and 2 R - 1 rows at W = 1 (dim 16) and W = 4 (dim 128): the lists after the first
    start at rows that are no multiple of the tile"""
    rng = np.random.default_rng(31)
    sizes = [ROWS - 1, ROWS, ROWS + 1, 1, 0, 2 * ROWS - 1]
    lists = np.repeat(np.arange(6), sizes).astype(np.uint32)
    n = len(lists)
    for dim in (16, 128):
        coarse, _, rows, _ = _case(rng, n, 6, dim, 1)
        perm = rng.permutation(n)
        pl, words = lists[perm], _words(rows, 0.0)
        Q = np.repeat(coarse, nq, axis=0) + F(0.1) * rng.standard_normal((6 * nq, dim)).astype(F)
        ix = _index(coarse, B.SQ, pl, words)
        assert ix.list_sizes().tolist() == sizes
        for nprobe in (1, 2, 6):
            _same(ix.search(Q, topk=70, nprobe=nprobe), _want(B.SQ, coarse, pl, BQ, words, dim, Q, nprobe, 70))
        ix.close()


def test_add_rows_packs_as_the_quantizer():
    import vq_amd

    rng = np.random.default_rng(41)
    coarse, lists, rows, Q = _case(rng, 3000, 10, 37, nq=30)
    rows[5, 3], rows[6, 0], rows[7, 1], rows[8, 2], rows[9, 4] = np.nan, np.inf, -np.inf, 0.5, -0.0
    bq = (0.5, 1, 4)
    ix = vq_amd.IVFBinaryIndex(coarse, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance.squared_euclidean())
    assert np.array_equal(ix.add_rows(lists[:1000], rows[:1000]), np.arange(1000))
    words = _words(rows, 0.5)
    assert np.array_equal(ix.packed(), words[:1000])
    want = _want(B.SQ, coarse, lists[:1000], bq, words[:1000], 37, Q, 3, 10)
    _same(ix.search(Q, topk=10, nprobe=3), want)
    # an add after a search rebuilds the device state
    assert np.array_equal(ix.add_rows(lists[1000:], rows[1000:].astype(np.float64)), np.arange(1000, 3000))
    assert np.array_equal(ix.packed(), words) and np.array_equal(ix.list_ids, lists)
    _same(ix.search(Q, topk=10, nprobe=3), _want(B.SQ, coarse, lists, bq, words, 37, Q, 3, 10))
    ix.close()
    assert np.array_equal(ix.packed(), words)  # the words outlive the handle
    _same(ix.search(Q, topk=10, nprobe=3), _want(B.SQ, coarse, lists, bq, words, 37, Q, 3, 10))
    ix.close()


@pytest.mark.parametrize("cm", [K.EUCLIDEAN, K.COSINE])
def test_add_assigns_the_nearest_list_under_the_coarse_distance(cm):
    import vq_amd

    rng = np.random.default_rng(14)
    coarse, _, rows, Q = _case(rng, 2000, 9, 21, nq=5)
    coarse *= rng.uniform(0.2, 5.0, (9, 1)).astype(F)  # norms differ: cosine and Euclidean assign differently
    ix = vq_amd.IVFBinaryIndex(coarse, coarse_distance=vq_amd.Distance(NAMES[cm]))
    flat = vq_amd.IVFFlatIndex(coarse, vq_amd.Distance(NAMES[cm]))
    assert np.array_equal(ix.add(rows), np.arange(2000))
    flat.add(rows)
    assert np.array_equal(ix.list_ids, flat.list_ids)
    assert np.array_equal(ix.probe(Q, 4), flat.probe(Q, 4))
    words = _words(rows, 0.0)
    assert np.array_equal(ix.packed(), words)
    _same(ix.search(Q, topk=10, nprobe=4), _want(B.MAN, coarse, ix.list_ids, BQ, words, 21, Q, 4, 10, coarse_metric=cm))
    _same(ix.search(Q, topk=10, nprobe=9), vq_amd.BinaryIndex(rows).search(Q, 10))
    ix.close()
    flat.close()


def test_padding_past_the_probed_rows():
    rng = np.random.default_rng(12)
    coarse, lists, rows, Q = _case(rng, 300, 40, 9, nq=20)
    lists[lists == 3] = 4  # Q[0] is centroid 3: its nearest list is empty
    words = _words(rows, 0.0)
    ix = _index(coarse, B.EUC, lists, words)
    for nprobe in (1, 2):
        got = ix.search(Q, topk=100, nprobe=nprobe)
        _same(got, _want(B.EUC, coarse, lists, BQ, words, 9, Q, nprobe, 100))
        assert (got[0] == R.PAD_ID).any() and np.isposinf(got[1][got[0] == R.PAD_ID]).all()
    assert (ix.search(Q[:1], topk=5, nprobe=1)[0] == R.PAD_ID).all()
    ix.close()


def test_device_form():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(15)
    coarse, lists, rows, Q = _case(rng, 4000, 20, 64, nq=70)
    words = _words(rows, 0.0)
    ix = _index(coarse, B.EUC, lists, words)
    host = ix.search(Q, topk=15, nprobe=4)
    dq = torch.from_numpy(Q).cuda()
    di = torch.empty((70, 15), dtype=torch.int32, device="cuda")
    dd = torch.empty((70, 15), dtype=torch.float32, device="cuda")
    ix.search_device(dq.data_ptr(), 70, 15, di.data_ptr(), dd.data_ptr(), nprobe=4)
    torch.cuda.synchronize()
    from vq_amd import _lib

    _lib.synchronize()
    _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), host)
    _same(host, _want(B.EUC, coarse, lists, BQ, words, 64, Q, 4, 15))
    ix.close()


@pytest.mark.parametrize("kind", ["flat", "scalar"])
def test_rerank_with_an_exact_index(kind):
    import vq_amd

    rng = np.random.default_rng(17)
    coarse, lists, rows, Q = _case(rng, 3000, 30, 24, nq=25)
    lists[lists == 3] = 4  # Q[0] probes an empty list first: fewer hits than candidates at nprobe 1
    ix = _index(coarse, B.MAN, lists, _words(rows, 0.0))
    sq = vq_amd.ScalarQuantizer(-4.0, 4.0, 256)
    exact = vq_amd.FlatIndex(rows) if kind == "flat" else vq_amd.ScalarIndex(rows, sq)
    for nprobe, cand in ((4, 40), (1, 20)):
        got = ix.search(Q, topk=10, nprobe=nprobe, rerank=exact, candidates=cand)
        hits = ix.search(Q, topk=cand, nprobe=nprobe)[0]
        for j in range(Q.shape[0]):
            real = hits[j][hits[j] != R.PAD_ID]
            t = min(10, real.size)
            if t:
                wi, wd = exact.rerank(Q[j:j + 1], real[None, :], t)
                _same((got[0][j:j + 1, :t], got[1][j:j + 1, :t]), (wi, wd))
            assert np.all(got[0][j, t:] == R.PAD_ID) and np.isposinf(got[1][j, t:]).all()
    ix.close()


def test_save_load_gives_the_same_search(tmp_path):
    import vq_amd

    rng = np.random.default_rng(19)
    coarse, lists, rows, Q = _case(rng, 2500, 11, 45, nq=20)
    bq = (0.25, 3, 200)
    words = _words(rows, 0.25)
    ix = _index(coarse, B.EUC, lists, words, bq, pieces=2, coarse_metric=K.COSINE)
    want = ix.search(Q, topk=12, nprobe=3)
    ix.save(tmp_path / "ix.bin")  # (with the handle open: the words come from it)
    back = vq_amd.IVFBinaryIndex.load(tmp_path / "ix.bin")
    assert back.coarse_distance.metric == K.COSINE
    _same(back.search(Q, topk=12, nprobe=3), want)
    _same(want, _want(B.EUC, coarse, lists, bq, words, 45, Q, 3, 12, coarse_metric=K.COSINE))
    ix.close()
    back.close()


def test_two_runs_give_the_same_arrays():
    rng = np.random.default_rng(23)
    coarse, lists, rows, Q = _case(rng, 8000, 20, 40, nq=200)
    rows[1000:3000] = rows[5]  # heavy ties
    words = _words(rows, 0.0)
    ix = _index(coarse, B.SQ, lists, words)
    a = ix.search(Q, topk=50, nprobe=6)
    b = ix.search(Q, topk=50, nprobe=6)
    _same(a, b)
    ix.close()
    ix2 = _index(coarse, B.SQ, lists, words)
    _same(ix2.search(Q, topk=50, nprobe=6), a)
    ix2.close()
