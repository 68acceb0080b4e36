"""Inverted-file scalar search on the MI355X (vq_amd.IVFScalarIndex, vqhip_ivfsq_*, vq_amd/csrc/k_ivfsq.hip).  Every
comparison is equality of indices and of distance bits: against the numpy statement of include/vqhip.h
(tests/ref_ivfsq.py), against IVFFlatIndex over the dequantized rows in the same lists (identity 1) and against
ScalarIndex at nprobe == nlist (identity 2).  All five metrics and the quantizers of tests/ref_sqindex.py (the degenerate
one included); dim 128 / 208 (16-byte loader, whole and 16-dimension last chunk), 36 (dword loader, 4 dimensions in the
last chunk), 5 / 33 / 1 (byte loader); batches on both sides of the count (16 queries per list) from which a list goes
to the tile kernel and of its 128-query tile, on each loader; list lengths around the 64-row tile; add_rows / add; padding;
the device form; rerank=; save / load; determinism."""
import numpy as np
import pytest

import ref_ivfsq as R
import ref_knn as K
import ref_sqindex as S

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
SQ = S.QUANTIZERS[2]  # (-3, 5, 17)


def _same(got, want, rows=None):
    gi, gd = got
    wi, wd = want
    if rows is not None:
        gi, gd, wi, wd = gi[rows], gd[rows], wi[rows], wd[rows]
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _cut(want, topk):
    """the statement at a smaller topk: the first topk columns of the sorted result"""
    return want[0][:, :topk], want[1][:, :topk]


def _case(rng, n, nlist, dim, nq, sq=SQ):
    """codes over the full byte range (codes >= levels occur), rows in an order unrelated to their lists, duplicates in
    the same list; the centroids and queries lie in the quantizer's range so that every list is probed by someone"""
    lo, hi = (sq[0], sq[1]) if abs(sq[0]) < 1e30 else (-1.0, 1.0)
    coarse = rng.uniform(lo, hi, (nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    codes[n - 7:] = codes[:7]  # duplicate rows ...
    lists[n - 7:] = lists[:7]  # ... in the same lists: ties by row id
    Q = rng.uniform(lo, hi, (nq, dim)).astype(F)
    Q[0] = coarse[min(3, nlist - 1)]
    return coarse, lists, codes, Q


def _index(coarse, metric, lists, codes, sq=SQ, pieces=1):
    import vq_amd

    ix = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*sq), vq_amd.Distance(NAMES[metric]))
    for a in np.array_split(np.arange(len(lists)), pieces):
        ix.add_codes(lists[a], codes[a])
    return ix


SHAPES = [
    (3001, 7, 128),    # 16-byte loader
    (2500, 256, 36),   # dword loader, 4 dimensions in the last chunk
    (2000, 1, 5),      # byte loader ...
    (1500, 7, 33),     # ... ragged last chunk
    (6000, 4096, 1),   # mostly empty lists
    (1500, 7, 208),    # 16-byte loader with a 16-dimension last chunk
]


@pytest.mark.parametrize("sq", S.QUANTIZERS)
@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(metric, shape, sq):
    n, nlist, dim = shape
    rng = np.random.default_rng(n + nlist + metric)
    coarse, lists, codes, Q = _case(rng, n, nlist, dim, nq=40, sq=sq)  # (40 queries: lists on both kernels)
    ix = _index(coarse, metric, lists, codes, sq, pieces=3)
    with np.errstate(all="ignore"):
        for nprobe in sorted({1, min(5, nlist), min(nlist, 1024)}):
            want = R.search(metric, coarse, lists, sq, codes, Q, nprobe, 1024)
            for topk in (1, 10, 256, 1024):
                _same(ix.search(Q, topk=topk, nprobe=nprobe), _cut(want, topk))
    ix.close()


@pytest.mark.parametrize("metric", K.METRICS)
def test_equals_ivfflat_over_dequantized_rows(metric):
    """identity 1: the same lists, the rows sq.dequantize_batch(codes), every nprobe and topk"""
    import vq_amd

    rng = np.random.default_rng(7 + metric)
    coarse, lists, codes, Q = _case(rng, 20000, 64, 48, nq=33)
    ix = _index(coarse, metric, lists, codes)
    flat = vq_amd.IVFFlatIndex(coarse, vq_amd.Distance(NAMES[metric]))
    flat.add_rows(lists, ix.quantizer.dequantize_batch(codes))
    for nprobe in (3, 64):
        assert np.array_equal(ix.probe(Q, nprobe), flat.probe(Q, nprobe))
        for topk in (1, 100):
            _same(ix.search(Q, topk=topk, nprobe=nprobe), flat.search(Q, topk=topk, nprobe=nprobe))
    ix.close()
    flat.close()


@pytest.mark.parametrize("metric", K.METRICS)
def test_all_lists_equal_scalar_index(metric):
    """identity 2"""
    import vq_amd

    rng = np.random.default_rng(9 + metric)
    coarse, lists, codes, Q = _case(rng, 20000, 64, 48, nq=33)
    ix = _index(coarse, metric, lists, codes)
    sx = vq_amd.ScalarIndex.from_codes(codes, ix.quantizer, ix.distance)
    for topk in (1, 100):
        _same(ix.search(Q, topk=topk, nprobe=64), sx.search(Q, topk))
    ix.close()


def test_all_lists_equal_scalar_index_two_query_batches():
    """1100 queries: more than the 1024 of a batch"""
    import vq_amd

    rng = np.random.default_rng(11)
    coarse, lists, codes, Q = _case(rng, 5000, 16, 20, nq=1100)
    ix = _index(coarse, K.EUCLIDEAN, lists, codes)
    sx = vq_amd.ScalarIndex.from_codes(codes, ix.quantizer, ix.distance)
    _same(ix.search(Q, topk=10, nprobe=16), sx.search(Q, 10))
    ix.close()


@pytest.mark.parametrize("dim", [48, 36, 33])  # the 16-byte, dword and byte loaders
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 127, 128, 129, 300])
def test_every_query_probes_the_same_lists(nq, dim):
    """nq queries beside one centroid: the lists they probe are each probed by all nq of them -- below 16 the positions
    kernel computes every pair, from 16 on the tile kernel, in one, two or three tiles of 128 queries"""
    rng = np.random.default_rng(100 + nq)
    coarse, lists, codes, _ = _case(rng, 4000, 12, dim, 1)
    Q = (coarse[5] + F(1e-3) * rng.standard_normal((nq, dim)).astype(F)).astype(F)
    ix = _index(coarse, K.EUCLIDEAN, lists, codes)
    P = ix.probe(Q, 3)
    assert np.all(P == P[0])
    _same(ix.search(Q, topk=30, nprobe=3), R.search(K.EUCLIDEAN, coarse, lists, SQ, codes, Q, 3, 30))
    ix.close()


@pytest.mark.parametrize("dim", [80, 68, 67])  # the 16-byte, dword and byte loaders
def test_kernel_variants_give_the_same_bits(dim):
    """the same query alone (the positions kernel) and among 39 copies of itself (the tile kernel)"""
    rng = np.random.default_rng(77)
    coarse, lists, codes, Q = _case(rng, 3000, 5, dim, 3)
    for metric in K.METRICS:
        ix = _index(coarse, metric, lists, codes)
        alone = ix.search(Q[1:2], topk=200, nprobe=2)
        many = ix.search(np.repeat(Q[1:2], 40, axis=0), topk=200, nprobe=2)
        for j in range(40):
            _same((many[0][j:j + 1], many[1][j:j + 1]), alone)
        ix.close()


@pytest.mark.parametrize("nq", [3, 40])  # the positions kernel, the tile kernel
def test_list_lengths_around_the_row_tile(nq):
    """lists of 63, 64, 65, 1, 0 and 127 rows at dim 16: the lists after the first start on 16-byte boundaries that are
    not 64-byte boundaries (row 63, 127, 192, ...)"""
    rng = np.random.default_rng(31)
    sizes = [63, 64, 65, 1, 0, 127]
    lists = np.repeat(np.arange(6), sizes).astype(np.uint32)
    n = len(lists)
    coarse, _, codes, _ = _case(rng, n, 6, 16, 1)
    perm = rng.permutation(n)
    lists, codes = lists[perm], codes[perm]
    Q = np.repeat(coarse, nq, axis=0) + F(1e-3) * rng.standard_normal((6 * nq, 16)).astype(F)
    for metric in (K.SQUARED_EUCLIDEAN, K.COSINE):
        ix = _index(coarse, metric, lists, codes)
        assert ix.list_sizes().tolist() == sizes
        for nprobe in (1, 2, 6):
            _same(ix.search(Q, topk=70, nprobe=nprobe), R.search(metric, coarse, lists, SQ, codes, Q, nprobe, 70))
        ix.close()


def test_add_rows_encodes_as_the_quantizer():
    import vq_amd

    rng = np.random.default_rng(41)
    coarse, lists, _, Q = _case(rng, 3000, 10, 17, nq=30)
    rows = rng.uniform(-4, 6, (3000, 17)).astype(F)  # past both ends of [-3, 5]
    rows[5, 3], rows[6, 0], rows[7, 1] = np.nan, np.inf, -np.inf
    sq = vq_amd.ScalarQuantizer(*SQ)
    ix = vq_amd.IVFScalarIndex(coarse, sq, vq_amd.Distance.manhattan())
    assert np.array_equal(ix.add_rows(lists[:1000], rows[:1000]), np.arange(1000))
    codes = sq.quantize_batch(rows)
    assert np.array_equal(ix.codes, codes[:1000])
    by_codes = _index(coarse, K.MANHATTAN, lists[:1000], codes[:1000])
    want = R.search(K.MANHATTAN, coarse, lists[:1000], SQ, codes[:1000], Q, 3, 10)
    _same(ix.search(Q, topk=10, nprobe=3), want)
    _same(by_codes.search(Q, topk=10, nprobe=3), want)
    by_codes.close()
    # an add after a search rebuilds the device state
    assert np.array_equal(ix.add_rows(lists[1000:], rows[1000:].astype(np.float64)), np.arange(1000, 3000))
    assert np.array_equal(ix.codes, codes) and np.array_equal(ix.list_ids, lists)
    _same(ix.search(Q, topk=10, nprobe=3), R.search(K.MANHATTAN, coarse, lists, SQ, codes, Q, 3, 10))
    ix.close()
    assert np.array_equal(ix.codes, codes)  # the codes outlive the handle
    _same(ix.search(Q, topk=10, nprobe=3), R.search(K.MANHATTAN, coarse, lists, SQ, codes, Q, 3, 10))
    ix.close()


def test_add_assigns_the_nearest_list():
    import vq_amd
    from vq_amd.ivf import _nearest_lists

    rng = np.random.default_rng(14)
    coarse, _, _, Q = _case(rng, 2000, 9, 21, nq=5)
    rows = rng.uniform(-3, 5, (2000, 21)).astype(F)
    sq = vq_amd.ScalarQuantizer(*SQ)
    ix = vq_amd.IVFScalarIndex(coarse, sq)
    assert np.array_equal(ix.add(rows), np.arange(2000))
    assert np.array_equal(ix.list_ids, _nearest_lists(coarse, rows, K.EUCLIDEAN))
    assert np.array_equal(ix.codes, sq.quantize_batch(rows))
    _same(ix.search(Q, topk=10, nprobe=9), vq_amd.ScalarIndex(rows, sq).search(Q, 10))
    ix.close()


def test_padding_past_the_probed_rows():
    rng = np.random.default_rng(12)
    coarse, lists, codes, Q = _case(rng, 300, 40, 9, nq=20)
    lists[lists == 3] = 4  # Q[0] is centroid 3: its nearest list is empty
    ix = _index(coarse, K.COSINE, lists, codes)
    for nprobe in (1, 2):
        got = ix.search(Q, topk=100, nprobe=nprobe)
        _same(got, R.search(K.COSINE, coarse, lists, SQ, codes, Q, nprobe, 100))
        assert (got[0] == R.PAD_ID).any() and np.isposinf(got[1][got[0] == R.PAD_ID]).all()
    assert (ix.search(Q[:1], topk=5, nprobe=1)[0] == R.PAD_ID).all()
    ix.close()


def test_device_form():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(15)
    coarse, lists, codes, Q = _case(rng, 4000, 20, 32, nq=70)
    ix = _index(coarse, K.EUCLIDEAN, lists, codes)
    host = ix.search(Q, topk=15, nprobe=4)
    dq = torch.from_numpy(Q).cuda()
    di = torch.empty((70, 15), dtype=torch.int32, device="cuda")
    dd = torch.empty((70, 15), dtype=torch.float32, device="cuda")
    ix.search_device(dq.data_ptr(), 70, 15, di.data_ptr(), dd.data_ptr(), nprobe=4)
    torch.cuda.synchronize()
    from vq_amd import _lib

    _lib.synchronize()
    _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), host)
    _same(host, R.search(K.EUCLIDEAN, coarse, lists, SQ, codes, Q, 4, 15))
    ix.close()


@pytest.mark.parametrize("kind", ["flat", "scalar"])
def test_rerank_with_an_exact_index(kind):
    import vq_amd

    rng = np.random.default_rng(17)
    coarse, lists, codes, Q = _case(rng, 3000, 30, 24, nq=25)
    lists[lists == 3] = 4  # Q[0] probes an empty list first: fewer hits than candidates at nprobe 1
    ix = _index(coarse, K.EUCLIDEAN, lists, codes)
    rows = ix.quantizer.dequantize_batch(codes) + F(0.01) * rng.standard_normal((3000, 24)).astype(F)  # "the original rows"
    exact = vq_amd.FlatIndex(rows) if kind == "flat" else vq_amd.ScalarIndex.from_codes(codes, vq_amd.ScalarQuantizer(-3.0, 5.0, 256))
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
    coarse, lists, codes, Q = _case(rng, 2500, 11, 28, nq=20)
    ix = _index(coarse, K.COSINE_UNCLAMPED, lists, codes, pieces=2)
    want = ix.search(Q, topk=12, nprobe=3)
    ix.save(tmp_path / "ix.bin")  # (with the handle open: the codes come from it)
    back = vq_amd.IVFScalarIndex.load(tmp_path / "ix.bin")
    _same(back.search(Q, topk=12, nprobe=3), want)
    _same(want, R.search(K.COSINE_UNCLAMPED, coarse, lists, SQ, codes, Q, 3, 12))
    ix.close()
    back.close()


def test_two_runs_give_the_same_arrays():
    rng = np.random.default_rng(23)
    coarse, lists, codes, Q = _case(rng, 8000, 20, 40, nq=200)
    codes[1000:3000] = codes[5]  # heavy ties
    ix = _index(coarse, K.COSINE, lists, codes)
    a = ix.search(Q, topk=50, nprobe=6)
    b = ix.search(Q, topk=50, nprobe=6)
    _same(a, b)
    ix.close()
    ix2 = _index(coarse, K.COSINE, lists, codes)
    _same(ix2.search(Q, topk=50, nprobe=6), a)
    ix2.close()
