"""Residual inverted-file PQ search on the MI355X (vq_amd.IVFPQIndex(..., residual=True), VQHIP_IVF_RESIDUAL,
k_ivf_rlut / k_ivf_rplan / k_ivf_rscan) against the numpy statement (tests/ref_ivf_residual.py): indices equal,
distances equal as uint32 bits.  All metrics; sub_dim 1 / 3 / 4 / 8 / 16 (the register and the generic table paths);
k 16 / 256 / 300; nlist up to 4096; nprobe 1 up to min(nlist, 1024); topk 1 up to 1024; many tiny and empty lists (scan
chunks across many slot boundaries); padding; cuts too dense for the LDS sort; the zero-centroid identity with a
non-residual index; adds in parts; the device form; rerank; a shape whose tables take several batches; 1M x 128; what
add stores; and the reconstruction error of a trained residual index against a non-residual one."""
import numpy as np
import pytest

import ref_ivf as R
import ref_ivf_residual as RR
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
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = (rng.standard_normal((m, k, sd)) * 0.5).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    codes[n - 7:] = codes[:7]  # duplicate codes: ties by row id within a list
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    Q[0] = coarse[min(3, nlist - 1)]
    return coarse, cb, lists, codes, Q


def _index(coarse, cb, metric, lists, codes, residual=True):
    import vq_amd

    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance(NAMES[metric]), residual=residual)
    ix.add_codes(lists, codes)
    return ix


SHAPES = [
    (3001, 7, 8, 256, 16),    # one-byte codes in 8-byte words, sub_dim 16 (register path)
    (2500, 256, 4, 300, 3),   # two-byte codes, generic path
    (2000, 1, 3, 16, 1),      # one list; m not a multiple of 8; sub_dim 1
    (6000, 4096, 8, 64, 2),   # many lists, most of them tiny or empty
    (1500, 7, 150, 256, 1),   # m * k = 38400, the table limit
    (2200, 64, 16, 256, 8),   # sub_dim 8 (register path)
    (2200, 64, 32, 16, 4),    # sub_dim 4, k 16
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(orc, metric, shape):
    n, nlist, m, k, sd = shape
    rng = np.random.default_rng(n + nlist + metric + 7)
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd)
    ix = _index(coarse, cb, metric, lists, codes)
    for nprobe in sorted({1, min(5, nlist), min(nlist, 1024)}):
        for topk in (1, 10, 256, 1024):
            want = RR.search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk)
            _same(ix.search(Q, topk=topk, nprobe=nprobe), want)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_tiny_lists_many_slot_boundaries_and_padding(orc, metric):
    """lists of 0-3 rows: a scan chunk crosses hundreds of slots; |S(q)| < topk pads"""
    rng = np.random.default_rng(20 + metric)
    n, nlist, m, k, sd = 1500, 1024, 8, 256, 4
    coarse, cb, _, codes, Q = _case(rng, n, nlist, m, k, sd, nq=5)
    lists = rng.choice(nlist // 2, n).astype(np.uint32) * 2  # odd lists empty, even lists ~3 rows
    ix = _index(coarse, cb, metric, lists, codes)
    sizes = ix.list_sizes()
    for nprobe in (1, 7, 300, 1024):
        for topk in (10, 1024):
            got = ix.search(Q, topk=topk, nprobe=nprobe)
            _same(got, RR.search(orc, metric, coarse, cb, lists, codes, Q, nprobe, topk))
            P = ix.probe(Q, nprobe=nprobe)
            for j in range(Q.shape[0]):
                s = int(sizes[P[j]].sum())
                if s < topk:
                    assert np.all(got[0][j, s:] == R.PAD_ID) and np.all(got[1][j, s:].view(np.uint32) == R.INF_BITS)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_nan_inf_queries_and_dense_cut(orc, metric):
    """equal codebook entries put every distance of a list on one value: cuts of more than 8192 positions take the
    exact radix select; NaN / inf queries collapse the histogram range"""
    rng = np.random.default_rng(50 + metric)
    n, nlist, m, k, sd = 30000, 3, 8, 64, 2
    coarse, cb, _, codes, Q = _case(rng, n, nlist, m, k, sd, nq=6)
    lists = (np.arange(n) % nlist).astype(np.uint32)
    flat_cb = cb.copy()
    flat_cb[:, :, :] = cb[:, :1, :]  # every centroid of a subspace equal: D constant per list
    Q[1, 0] = np.nan
    Q[2, -1] = np.inf
    Q[3, 3] = -np.inf
    for c in (cb, flat_cb):
        ix = _index(coarse, c, metric, lists, codes)
        for nprobe in (1, 3):
            for topk in (1, 1024):
                _same(ix.search(Q, topk=topk, nprobe=nprobe), RR.search(orc, metric, coarse, c, lists, codes, Q, nprobe, topk))
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_zero_centroids_equal_non_residual(metric):
    rng = np.random.default_rng(60 + metric)
    coarse, cb, lists, codes, Q = _case(rng, 5000, 64, 8, 256, 4, nq=20)
    Q[1, 2] = -0.0
    Q[2, 0] = np.nan
    Q[3, 1] = np.inf
    zero = np.zeros_like(coarse)
    res = _index(zero, cb, metric, lists, codes, residual=True)
    plain = _index(zero, cb, metric, lists, codes, residual=False)
    for nprobe in (1, 9, 64):
        assert np.array_equal(res.probe(Q, nprobe=nprobe), plain.probe(Q, nprobe=nprobe))
        for topk in (1, 33, 1024):
            _same(res.search(Q, topk=topk, nprobe=nprobe), plain.search(Q, topk=topk, nprobe=nprobe))
    res.close()
    plain.close()


def test_adds_in_parts_equal_one_add(orc):
    import vq_amd

    rng = np.random.default_rng(11)
    coarse, cb, lists, codes, Q = _case(rng, 3000, 32, 8, 256, 2, nq=10)
    whole = _index(coarse, cb, K.EUCLIDEAN, lists, codes)
    parts = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean(), residual=True)
    parts.add_codes(lists[:1000], codes[:1000])
    _same(parts.search(Q, topk=20, nprobe=4), RR.search(orc, K.EUCLIDEAN, coarse, cb, lists[:1000], codes[:1000], Q, 4, 20))
    parts.add_codes(lists[1000:1001], codes[1000:1001])
    parts.add_codes(lists[1001:], codes[1001:])
    for nprobe, topk in ((4, 20), (1, 300), (32, 1024)):
        got = parts.search(Q, topk=topk, nprobe=nprobe)
        _same(got, whole.search(Q, topk=topk, nprobe=nprobe))
        _same(got, RR.search(orc, K.EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, topk))
    whole.close()
    parts.close()


def test_search_device_equals_search():
    import torch
    from vq_amd import _lib

    rng = np.random.default_rng(13)
    coarse, cb, lists, codes, Q = _case(rng, 50000, 128, 8, 256, 4, nq=300)
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes)
    want = ix.search(Q, topk=64, nprobe=9)
    dq = torch.from_numpy(Q).cuda()
    di = torch.empty((300, 64), dtype=torch.int32, device="cuda")
    dd = torch.empty((300, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ix.search_device(dq.data_ptr(), 300, 64, di.data_ptr(), dd.data_ptr(), nprobe=9)
    _lib.load().vqhip_synchronize()
    _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), want)
    ix.close()


def test_rerank_equals_flat_rerank_of_hits():
    import vq_amd

    rng = np.random.default_rng(12)
    n, d = 6000, 32
    X = rng.standard_normal((n, d)).astype(F)
    coarse = X[rng.choice(n, 24, replace=False)]
    cb = (rng.standard_normal((8, 64, 4)) * 0.5).astype(F)
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean(), residual=True)
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


def test_tables_in_several_batches(orc):
    """m k = 38400 at nprobe 512: 78.6 MB of tables per query, so a batch holds 3 of the 7 queries"""
    rng = np.random.default_rng(14)
    n, nlist, m, k, sd = 4000, 512, 150, 256, 1
    coarse, cb, lists, codes, Q = _case(rng, n, nlist, m, k, sd, nq=7)
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes)
    for topk in (1, 100):
        _same(ix.search(Q, topk=topk, nprobe=512), RR.search(orc, K.SQUARED_EUCLIDEAN, coarse, cb, lists, codes, Q, 512, topk))
    ix.close()


def test_add_stores_residual_codes(orc):
    import vq_amd

    rng = np.random.default_rng(15)
    n, d, nlist = 3000, 48, 40
    X = rng.standard_normal((n, d)).astype(F)
    X[5, 7] = -0.0
    coarse = X[rng.choice(n, nlist, replace=False)] + F(0.01)
    for metric, k in ((K.SQUARED_EUCLIDEAN, 256), (K.MANHATTAN, 300)):
        cb = (rng.standard_normal((6, k, 8)) * 0.5).astype(F)
        ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance(NAMES[metric]), residual=True)
        ids = ix.add(X)
        assert np.array_equal(ids, np.arange(n, dtype=np.uint32))
        lists, codes = RR.encode(orc, metric, coarse, cb, X)
        assert np.array_equal(ix.list_ids, lists)
        assert np.array_equal(ix.codes.astype(np.int64), codes.astype(np.int64))


def test_train_residual_halves_reconstruction_error():
    import vq_amd

    rng = np.random.default_rng(16)
    n, d, centres = 100_000, 64, 1024
    C = rng.standard_normal((centres, d)).astype(F)
    X = (C[rng.integers(0, centres, n)] + rng.standard_normal((n, d)).astype(F) * F(0.3)).astype(F)
    mse = {}
    for residual in (False, True):
        ix = vq_amd.IVFPQIndex.train(X, 1024, 8, 256, max_iters=10, residual=residual)
        assert ix.residual == residual
        ix.add(X)
        if residual:
            rec = RR.reconstruct(ix.coarse_centroids, ix.codebooks, ix.list_ids, ix.codes)
        else:
            cb = ix.codebooks
            rec = np.concatenate([cb[s][ix.codes[:, s].astype(np.int64)] for s in range(ix.m)], axis=1)
        mse[residual] = float(np.mean((rec.astype(np.float64) - X) ** 2))
    assert mse[True] <= 0.5 * mse[False], mse


def test_large_1m_x_128(orc):
    rng = np.random.default_rng(2024)
    n, nlist, m, k, sd, nq = 1 << 20, 1024, 8, 256, 16, 128
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = (rng.standard_normal((m, k, sd)) * 0.5).astype(F)
    w = rng.gamma(2.0, 1.0, nlist)  # uneven lists, as k-means leaves them
    lists = rng.choice(nlist, n, p=w / w.sum()).astype(np.uint32)
    codes = rng.integers(0, k, (n, m), dtype=np.uint8)
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes)
    got = ix.search(Q, topk=10, nprobe=32)
    _same(got, RR.search(orc, K.EUCLIDEAN, coarse, cb, lists, codes, Q, 32, 10))
    ix.close()
