"""Exact k-NN search and rerank on the MI355X (vq_amd.FlatIndex, vqhip_flat_*, vq_amd/csrc/k_knn.hip) against the
numpy statement of include/vqhip.h (tests/ref_knn.py): indices equal, distances equal as uint32 bits.  All five
metrics, f32 and f16 rows, d around the 32-dimension chunks, n off every tile, topk 1 / 10 / 1024 and n = topk,
several query batches, duplicate rows, NaN / inf / zero rows, a cut too dense for the candidate sort (the radix
select), the device form at unaligned pointers, rerank, PQ search with rerank, evalcli --recall-full and a sampled
1M x 128 check."""
import numpy as np
import pytest

import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32


def _assert_same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _data(n, d, rng, nq=5):
    X = (rng.standard_normal((n, d)) * 1.5).astype(F)
    sp = K.special_rows(d, rng)
    X[7:7 + len(sp)] = sp
    X[n - 3:] = X[20:23]  # exact duplicates of rows 20..22: ties by row index
    X[100 % n] = X[7 % n] if n > 100 else X[100 % n]
    Q = (rng.standard_normal((nq, d))).astype(F)
    Q[0] = X[21]  # a query equal to a duplicated row
    if nq > 3:
        Q[3] = 0.0  # the zero query (cosine: the EPSILON rule)
    return Q, X


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 127, 128, 129, 384, 768, 1000])
def test_search_matches_statement(metric, dtype, d):
    import vq_amd

    rng = np.random.default_rng(1000 * metric + d)
    Q, X = _data(1037, d, rng)
    with np.errstate(over="ignore"):
        Xt = X.astype(dtype)
    ix = vq_amd.FlatIndex(Xt, vq_amd.Distance(["squared_euclidean", "euclidean", "manhattan", "cosine",
                                               "cosine_unclamped"][metric]))
    got = ix.search(Q, 10)
    _assert_same(got, K.search(metric, Q, Xt.astype(F), 10))


@pytest.mark.parametrize("n, topk", [(1, 1), (10, 10), (1024, 1024), (1029, 1024), (1029, 1), (70, 65)])
@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_topk_edges(n, topk, metric):
    import vq_amd

    rng = np.random.default_rng(n + topk)
    Q = rng.standard_normal((3, 20)).astype(F)
    X = rng.standard_normal((n, 20)).astype(F)
    if n >= 30:
        X[n - 5:] = X[:5]
    ix = vq_amd.FlatIndex(X, vq_amd.Distance(["euclidean", "cosine"][metric == K.COSINE]))
    _assert_same(ix.search(Q, topk), K.search(metric, Q, X, topk))


def test_several_batches():
    """1100 queries over 300 007 rows: the [batch][n] distances are bounded by 1 GB -- 768 queries per batch"""
    import vq_amd

    rng = np.random.default_rng(3)
    X = rng.standard_normal((300_007, 4)).astype(F)
    Q = rng.standard_normal((1100, 4)).astype(F)
    ix = vq_amd.FlatIndex(X, vq_amd.Distance.squared_euclidean())
    got = ix.search(Q, 10)
    _assert_same(got, K.search(K.SQUARED_EUCLIDEAN, Q, X, 10))


@pytest.mark.parametrize("topk", [1, 1024])
def test_dense_ties_take_the_radix_select(topk):
    """20 000 equal rows (and a few NaN): every distance equal, the histogram cut holds them all -> exact radix select"""
    import vq_amd

    X = np.ones((20_000, 16), F)
    X[5] = np.nan
    X[19_999] = 0.5
    Q = np.zeros((2, 16), F)
    Q[1] = 1.0
    ix = vq_amd.FlatIndex(X, vq_amd.Distance.manhattan())
    _assert_same(ix.search(Q, topk), K.search(K.MANHATTAN, Q, X, topk))


def test_all_nan_distances():
    import vq_amd

    X = np.full((300, 8), np.nan, F)
    ix = vq_amd.FlatIndex(X)
    _assert_same(ix.search(np.zeros((2, 8), F), 5), K.search(K.EUCLIDEAN, np.zeros((2, 8), F), X, 5))


@pytest.mark.parametrize("off", [1, 3])
def test_search_device_unaligned(off):
    import torch

    import vq_amd

    rng = np.random.default_rng(off)
    d, nq, topk = 37, 9, 17
    Q, X = _data(2001, d, rng, nq)
    ix = vq_amd.FlatIndex(X, vq_amd.Distance.cosine())
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    ix.search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off)
    vq_amd._lib.synchronize()
    torch.cuda.synchronize()
    ih, dh = ib.cpu().numpy(), db.cpu().numpy()
    got = (ih[off:off + nq * topk].view(np.uint32).reshape(nq, topk), dh[off:off + nq * topk].reshape(nq, topk))
    _assert_same(got, K.search(K.COSINE, Q, X, topk))
    assert (ih[:off] == 7).all() and (ih[off + nq * topk:] == 7).all()
    assert (dh[:off] == -1).all() and (dh[off + nq * topk:] == -1).all()


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("c, topk", [(1, 1), (100, 10), (100, 100), (4096, 50), (4096, 4096), (777, 300)])
def test_rerank_matches_brute_force_over_candidates(metric, c, topk):
    import vq_amd

    rng = np.random.default_rng(c + topk + metric)
    Q, X = _data(5003, 24, rng, 4)
    X[40:45] = X[41]  # ties among candidates
    rest = np.setdiff1d(np.arange(5003), np.arange(40, 45))  # rows 40..44 (equal) lead every list: ties
    cand = np.stack([np.concatenate([np.arange(40, 45), rng.permutation(rest)])[:c] for _ in range(4)])
    ix = vq_amd.FlatIndex(X.astype(np.float16) if metric == K.MANHATTAN else X,
                          vq_amd.Distance(["squared_euclidean", "euclidean", "manhattan", "cosine",
                                           "cosine_unclamped"][metric]))
    Xs = X.astype(np.float16).astype(F) if metric == K.MANHATTAN else X
    _assert_same(ix.rerank(Q, cand, topk), K.rerank(metric, Q, Xs, cand, topk))


def test_rerank_out_of_range_id_flagged_on_device():
    """the C ABI without the Python checks: an id >= n is reported by the device flag, never read"""
    import vq_amd
    from vq_amd import _lib

    X = np.random.default_rng(0).standard_normal((100, 8)).astype(F)
    fl = _lib.Flat(X, _lib.EUCLIDEAN)
    cand = np.array([[1, 2, 3, 0xFFFFFFF0], [4, 5, 6, 7]], np.uint32)
    with pytest.raises(vq_amd.FfiError, match="candidate row id"):
        fl.rerank(np.zeros((2, 8), F), cand, 2)
    idx, dist = fl.rerank(np.zeros((2, 8), F), cand[:, :3].copy(), 2)  # the handle works on
    _assert_same((idx, dist), K.rerank(K.EUCLIDEAN, np.zeros((2, 8), F), X, cand[:, :3], 2))
    fl.close()


def _pq_setup(rng, n=6000, m=4, k=64, sd=6):
    cb = rng.standard_normal((m, k, sd)).astype(F)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    X = rng.standard_normal((n, m * sd)).astype(F)
    return cb, codes, X


@pytest.mark.parametrize("flat_metric", [K.EUCLIDEAN, K.COSINE])
def test_pqindex_search_rerank(flat_metric):
    import vq_amd
    from vq_amd.store import PQIndex

    rng = np.random.default_rng(11)
    cb, codes, X = _pq_setup(rng)
    Q = rng.standard_normal((7, X.shape[1])).astype(F)
    idx = PQIndex(cb, codes, vq_amd.Distance.squared_euclidean())
    fi = vq_amd.FlatIndex(X, vq_amd.Distance(["euclidean", "cosine"][flat_metric == K.COSINE]))
    plain = idx.search(Q, 10)
    assert np.array_equal(plain[0], idx.search(Q, 10)[0])
    got = idx.search(Q, 10, rerank=fi, candidates=80)
    adc_idx, _ = idx.search(Q, 80)
    _assert_same(got, K.rerank(flat_metric, Q, X, adc_idx, 10))
    got = idx.search(Q, 10, rerank=fi)  # default 4 topk candidates
    _assert_same(got, K.rerank(flat_metric, Q, X, idx.search(Q, 40)[0], 10))


def test_productquantizer_search_rerank():
    import vq_amd

    rng = np.random.default_rng(12)
    X = rng.standard_normal((3000, 16)).astype(F)
    pq = vq_amd.ProductQuantizer(X, 4, 16, 3, vq_amd.Distance.euclidean(), 5)
    codes = pq.encode(X)
    Q = rng.standard_normal((5, 16)).astype(F)
    fi = vq_amd.FlatIndex(X, vq_amd.Distance.cosine())
    got = pq.search(codes, Q, 5, rerank=fi, candidates=64)
    _assert_same(got, K.rerank(K.COSINE, Q, X, pq.search(codes, Q, 64)[0], 5))


def test_evalcli_recall_full_matches_numpy():
    import vq_amd
    from vq_amd import _lib
    from vq_amd.evalcli import recall_at_k_full

    n, d, k = 5000, 32, 10
    X = _lib.synth_uniform_host(n, d, 66, 0)
    pq = vq_amd.ProductQuantizer(X, 4, 32, 4, vq_amd.Distance.euclidean(), 66)
    f16 = pq.quantize_batch(X)
    got = recall_at_k_full(X, f16, k)
    qi = np.arange(0, n, 5)
    A = f16.astype(F)
    t_idx, _ = K.search(K.SQUARED_EUCLIDEAN, X[qi], X, k + 1)
    a_idx, _ = K.search(K.SQUARED_EUCLIDEAN, A[qi], A, k + 1)

    def drop(row, i):
        hit = np.flatnonzero(row == i)
        return np.delete(row, hit[0]) if hit.size else row[:k]

    want = np.mean([len(np.intersect1d(drop(t_idx[j], i), drop(a_idx[j], i))) / k for j, i in enumerate(qi)])
    assert got == pytest.approx(want, abs=0) and 0.0 < got <= 1.0


def test_evalcli_recall_full_flag(capsys):
    from vq_amd import evalcli

    assert evalcli.main(["pq", "--samples", "2000", "--dim", "32", "--m", "4", "--k", "16", "--max-iters", "2",
                         "--recall-full"]) == 0
    assert "Recall@10 (exact, all rows):" in capsys.readouterr().out


def test_one_million_rows_sampled():
    """1M x 128, 4 queries, topk 100: every returned distance is vqhip_distance_batch's, and no sampled unreturned row
    orders before the 100th"""
    import vq_amd
    from vq_amd import _lib
    from vq_amd._pairwise import pairwise_distance

    n, d, topk = 1 << 20, 128, 100
    X = _lib.synth_uniform_host(n, d, 9, 0)
    rng = np.random.default_rng(9)
    Q = rng.random((4, d), dtype=F)
    for metric in (K.SQUARED_EUCLIDEAN, K.COSINE):
        ix = vq_amd.FlatIndex(X, vq_amd.Distance(["squared_euclidean", "cosine"][metric == K.COSINE]))
        idx, dist = ix.search(Q, topk)
        for j in range(4):
            rows = idx[j].astype(np.int64)
            assert len(set(rows.tolist())) == topk
            ref = pairwise_distance(metric, np.repeat(Q[j][None], topk, 0), X[rows])
            assert np.array_equal(dist[j].view(np.uint32), K.reported(ref).view(np.uint32))
            keys = K.key(dist[j])
            assert (np.diff(keys.astype(np.int64)) >= 0).all()
            sample = np.setdiff1d(rng.choice(n, 20_000, replace=False), rows)
            ds = pairwise_distance(metric, np.repeat(Q[j][None], sample.size, 0), X[sample])
            ks = K.key(ds)
            kth, rth = keys[-1], rows[-1]
            assert not ((ks < kth) | ((ks == kth) & (sample < rth))).any()
