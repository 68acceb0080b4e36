"""Filtered inverted-file search on the MI355X (``allowed=`` of vq_amd.IVFFlatIndex / IVFScalarIndex,
vqhip_ivfflat_*_masked and vqhip_ivfsq_*_masked: the view kernels of vq_amd/csrc/ivf_view.hpp and the picked row sources
of ivf_tile.hpp) against the numpy statement of include/vqhip.h (tests/ref_ivf_filter.py): indices equal, distances equal
as uint32 bits, no tolerance anywhere.  Five metrics, f32 and f16 rows, an empty / a one-row / a large list, ten masks,
nprobe == nlist against the library's own masked FlatIndex, tile edges of the picked rows, the switch between the two
distance kernels, short and NaN results, the edges of the view's count scan, a view that follows the handle's rows, two
batches, the device forms at offset pointers, range search, the scalar index at its three load widths, seeded draws."""
import numpy as np
import pytest

import ref_filter as RF
import ref_ivf_filter as RIF
import ref_ivf_range as RR
import ref_ivfflat as RI
import ref_knn as K
import ref_range as R
import ref_sqindex as SI

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
N, NLIST = 1037, 7
BIG, ONE, EMPTY = 0, 5, 2  # the list with more than 128 rows, the list of one row, the list of none


def _dist(metric):
    import vq_amd

    return vq_amd.Distance(NAMES[metric])


def _same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


def _same_range(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), what


def _flat(coarse, metric, lists, rows):
    import vq_amd

    ix = vq_amd.IVFFlatIndex(coarse, _dist(metric), rows.dtype)
    ix.add_rows(lists, rows)
    return ix


def _base(d, rng, nq=24):
    """n = 1037 rows in 7 lists: list 2 empty, list 5 one row, list 0 about 300; the corner rows of ref_knn.special_rows at
    7.. and 130.., exact duplicates of rows 20..22 at 200..202 and at the end, in their lists; 24 queries, 18 of them beside
    centroid 0 (its list goes through the tile kernel at every nprobe), the others spread (the scan kernel)"""
    coarse = (rng.standard_normal((NLIST, d)) * 2).astype(F)
    lists = rng.choice(np.array([0, 0, 1, 3, 4, 6], np.uint32), N)
    lists[500] = ONE
    X = (coarse[lists] + rng.standard_normal((N, d)) * 0.7).astype(F)
    sp = K.special_rows(d, rng)
    for at in (7, 130):
        X[at:at + len(sp)] = sp
    for at in (200, N - 3):
        X[at:at + 3] = X[20:23]
        lists[at:at + 3] = lists[20:23]
    assert (lists == EMPTY).sum() == 0 and (lists == ONE).sum() == 1 and (lists == BIG).sum() > 128
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[:18] = coarse[0] + F(0.05) * rng.standard_normal((18, d)).astype(F)
    Q[0] = X[21]
    Q[18] = coarse[EMPTY]
    Q[19] = coarse[ONE]
    Q[20] = 0.0
    return coarse, lists, X, Q


def _masks(lists, rng):
    """the masks of the issue: name -> (bool mask, what is handed to the index)"""
    n = len(lists)

    def rand(p):
        m = rng.random(n) < p
        # the corner rows and the duplicates on both sides of the mask
        m[7:11], m[11:15] = True, False
        m[130:134], m[134:138] = False, True
        m[20], m[21], m[22] = True, False, True
        m[200], m[201], m[202] = False, True, False
        m[n - 3], m[n - 2], m[n - 1] = False, True, True
        return m

    one = lambda i: np.arange(n) == i
    half = rand(0.5)
    tail = RF.pack(half).copy()
    tail[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # every bit past n in the last word set
    ids = np.arange(n)
    out = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "row0": one(0), "last": one(n - 1), "half": rand(0.5),
           "3pc": rand(0.03), "no big list": lists != BIG, "one list": lists == 3, "ids 100..333": (ids >= 100) & (ids < 333)}
    out = {k: (m, m) for k, m in out.items()}
    out["words"] = (out["3pc"][0], RF.pack(out["3pc"][0]))
    out["half+tail"] = (half, tail)
    return out


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [1, 5, 129])
def test_search_and_range_match_statement(metric, dtype, d):
    rng = np.random.default_rng(1000 * metric + d)
    coarse, lists, X, Q = _base(d, rng)
    with np.errstate(over="ignore"):
        Xt = X.astype(dtype)
    ix = _flat(coarse, metric, lists, Xt)
    masks = _masks(lists, rng)
    r = R.kth_distance(metric, Q, np.nan_to_num(Xt.astype(F), nan=0.0, posinf=3e38, neginf=-3e38), 60)
    r[np.isnan(r)] = np.inf
    for nprobe in (1, 3, 7):
        plain = ix.search(Q, 10, nprobe)
        plain_r = ix.range_search(Q, r, nprobe)
        for name, (m, arg) in masks.items():
            what = f"{name}, nprobe {nprobe}"
            got = ix.search(Q, 10, nprobe, allowed=arg)
            _same(got, RIF.search(metric, coarse, lists, Xt, Q, nprobe, 10, m), what)
            rgot = ix.range_search(Q, r, nprobe, allowed=arg)
            _same_range(rgot, RIF.range_search(metric, coarse, lists, Xt, Q, nprobe, r, m), what)
            if name == "ones":
                _same(got, plain, "all ones against the unmasked call")
                _same_range(rgot, plain_r, "all ones against the unmasked call")
            if name == "zeros":
                assert (got[0] == 0xFFFFFFFF).all() and np.isposinf(got[1]).all()
                assert (rgot[0] == 0).all() and rgot[1].size == 0
            assert not np.isin(got[0], np.flatnonzero(~m)).any() and m[rgot[1]].all(), what
        _same(ix.search(Q, 10, nprobe), plain, "the unmasked call after masked ones")
    ix.close()


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_all_lists_equal_the_masked_flat_index(metric, dtype):
    """nprobe == nlist against FlatIndex.search(..., allowed=) and .range_search(..., allowed=): the library itself"""
    import vq_amd

    rng = np.random.default_rng(50 + metric)
    coarse, lists, X, Q = _base(48, rng)
    with np.errstate(over="ignore"):
        Xt = X.astype(dtype)
    ix = _flat(coarse, metric, lists, Xt)
    fx = vq_amd.FlatIndex(Xt, _dist(metric))
    for name, (m, arg) in _masks(lists, rng).items():
        for topk in (1, 100):
            _same(ix.search(Q, topk, NLIST, allowed=arg), fx.search(Q, topk, allowed=arg), name)
        for radius in (np.inf, 9.0 if metric < K.COSINE else 0.9):
            _same_range(ix.range_search(Q, radius, NLIST, allowed=arg), fx.range_search(Q, radius, allowed=arg), name)
    ix.close()


@pytest.mark.parametrize("count", [63, 64, 65, 129])
def test_tile_edges_of_the_picked_rows(count):
    """a list with exactly `count` allowed rows out of 300, read by the tile kernel (20 queries) and the scan kernel (3)"""
    rng = np.random.default_rng(count)
    n, d = 900, 37
    coarse = (rng.standard_normal((3, d)) * 3).astype(F)
    lists = (np.arange(n) % 3).astype(np.uint32)
    X = (coarse[lists] + rng.standard_normal((n, d))).astype(F)
    m = rng.random(n) < 0.3
    m[lists == 1] = False
    m[rng.permutation(np.flatnonzero(lists == 1))[:count]] = True
    assert int(m[lists == 1].sum()) == count
    Q = (coarse[1] + F(0.1) * rng.standard_normal((20, d))).astype(F)
    for metric in (K.EUCLIDEAN, K.COSINE):
        ix = _flat(coarse, metric, lists, X)
        for q in (Q, Q[:3]):
            assert (ix.probe(q, 1) == 1).all()
            for nprobe in (1, 3):
                _same(ix.search(q, count, nprobe, allowed=m), RIF.search(metric, coarse, lists, X, q, nprobe, count, m), f"nprobe {nprobe}")
                _same_range(ix.range_search(q, np.inf, nprobe, allowed=m),
                            RIF.range_search(metric, coarse, lists, X, q, nprobe, np.inf, m), f"nprobe {nprobe}")
        ix.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("nq", [15, 16, 17, 127, 128, 129])
def test_kernel_switch(nq, dtype):
    """nq queries beside one centroid: below 16 the scan kernel computes every pair, from 16 on the tile kernel"""
    rng = np.random.default_rng(100 + nq)
    coarse, lists, X, _ = _base(36, rng)
    with np.errstate(over="ignore"):
        Xt = np.nan_to_num(X, nan=0.5, posinf=2.0, neginf=-2.0).astype(dtype)
    Q = (coarse[4] + F(1e-3) * rng.standard_normal((nq, 36)).astype(F)).astype(F)
    m = _masks(lists, rng)["half"][0]
    ix = _flat(coarse, K.EUCLIDEAN, lists, Xt)
    P = ix.probe(Q, 3)
    assert np.all(P == P[0])
    _same(ix.search(Q, 30, 3, allowed=m), RIF.search(K.EUCLIDEAN, coarse, lists, Xt, Q, 3, 30, m))
    ix.close()


def test_kernel_variants_give_the_same_bits_under_a_mask():
    """the same query alone (the scan kernel) and among 39 copies of itself (the tile kernel), one mask"""
    rng = np.random.default_rng(77)
    coarse, lists, X, Q = _base(67, rng)
    m = _masks(lists, rng)["half"][0]
    for metric in K.METRICS:
        ix = _flat(coarse, metric, lists, X)
        alone = ix.search(Q[1:2], 200, 2, allowed=m)
        many = ix.search(np.repeat(Q[1:2], 40, axis=0), 200, 2, allowed=m)
        for j in range(40):
            _same((many[0][j:j + 1], many[1][j:j + 1]), alone)
        _same(alone, RIF.search(metric, coarse, lists, X, Q[1:2], 2, 200, m))
        ix.close()


def test_fewer_allowed_rows_than_topk():
    """7 allowed rows in S(q), 2 of them with NaN distances, topk 10: 5 finite, the 2 NaN rows in row order, 3 padding"""
    rng = np.random.default_rng(5)
    n, d = 500, 9
    coarse = np.stack([np.full(d, -4, F), np.full(d, 4, F)])
    lists = (np.arange(n) % 2).astype(np.uint32)
    X = (coarse[lists] + rng.standard_normal((n, d))).astype(F)
    X[300, 2] = np.nan
    X[78, 0] = np.nan
    X[10, 3] = np.nan  # a NaN row of the list that is not allowed
    allowed = [4, 78, 130, 132, 300, 420, 498]  # all in list 0
    m = np.zeros(n, bool)
    m[allowed] = True
    m[[1, 3, 5, 77]] = True  # allowed rows of the list that is not probed
    Q = (coarse[0] + rng.standard_normal((4, d))).astype(F)
    for nq in (4, 40):  # the scan kernel, the tile kernel
        q = np.resize(Q, (nq, d))
        ix = _flat(coarse, K.EUCLIDEAN, lists, X)
        idx, dist = ix.search(q, 10, 1, allowed=m)
        _same((idx, dist), RIF.search(K.EUCLIDEAN, coarse, lists, X, q, 1, 10, m))
        for j in range(nq):
            assert sorted(idx[j, :5].tolist()) == [4, 130, 132, 420, 498] and np.isfinite(dist[j, :5]).all()
            assert idx[j, 5:7].tolist() == [78, 300] and (dist[j, 5:7].view(np.uint32) == 0x7FC00000).all()
            assert (idx[j, 7:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, 7:]).all()
        ix.close()


def test_topk_1024_with_600_allowed():
    rng = np.random.default_rng(6)
    n, d = 1500, 7
    coarse = rng.standard_normal((4, d)).astype(F)
    lists = rng.integers(0, 4, n).astype(np.uint32)
    X = rng.standard_normal((n, d)).astype(F)
    m = np.zeros(n, bool)
    m[rng.permutation(n)[:600]] = True
    Q = rng.standard_normal((3, d)).astype(F)
    ix = _flat(coarse, K.MANHATTAN, lists, X)
    got = ix.search(Q, 1024, 4, allowed=m)
    _same(got, RIF.search(K.MANHATTAN, coarse, lists, X, Q, 4, 1024, m))
    assert (got[0][:, 600:] == 0xFFFFFFFF).all() and (got[0][:, :600] != 0xFFFFFFFF).all()
    _same(ix.search(Q, 1024, 2, allowed=m), RIF.search(K.MANHATTAN, coarse, lists, X, Q, 2, 1024, m))
    ix.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_view_scan_edges(n):
    """the mask's word edges, the edges of a wave, of a pass and of a block of the view's count (1024 positions)"""
    rng = np.random.default_rng(n)
    d, nlist = 6, 3
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((3, d)).astype(F)
    ix = _flat(coarse, K.EUCLIDEAN, lists, X)
    topk = min(n, 5)
    masks = [rng.random(n) < 0.5, np.ones(n, bool), np.arange(n) == n - 1, np.arange(n) == 0, np.arange(n) >= 32, np.zeros(n, bool)]
    for j, m in enumerate(masks):
        for nprobe in (1, nlist):
            _same(ix.search(Q, topk, nprobe, allowed=RF.pack(m)), RIF.search(K.EUCLIDEAN, coarse, lists, X, Q, nprobe, topk, m), f"mask {j}")
            _same_range(ix.range_search(Q, np.inf, nprobe, allowed=m),
                        RIF.range_search(K.EUCLIDEAN, coarse, lists, X, Q, nprobe, np.inf, m), f"mask {j}")
    ix.close()


def test_view_past_one_scan_block():
    """n = 2^20 + 77: 1025 count blocks, so the scan of the view's counts takes a second pass with a carry; allowed rows
    on both sides of position 2^20 in list order"""
    rng = np.random.default_rng(20)
    n, d, nlist = (1 << 20) + 77, 2, 3
    coarse = np.array([[-3, 0], [0, 3], [3, 0]], F)
    lists = (np.arange(n) % nlist).astype(np.uint32)
    X = (coarse[lists] + rng.standard_normal((n, d))).astype(F)
    Q = rng.standard_normal((3, d)).astype(F) * 2
    ix = _flat(coarse, K.SQUARED_EUCLIDEAN, lists, X)
    sparse = rng.random(n) < 0.0005
    sparse[n - 200:] = True  # the end of the last list: the positions past 2^20
    for name, m in (("sparse", sparse), ("tail", np.arange(n) >= n - 300), ("ones", np.ones(n, bool))):
        for nprobe in (1, 3):
            _same(ix.search(Q, 10, nprobe, allowed=m), RIF.search(K.SQUARED_EUCLIDEAN, coarse, lists, X, Q, nprobe, 10, m), name)
        if name != "ones":
            _same_range(ix.range_search(Q, np.inf, 3, allowed=m), RIF.range_search(K.SQUARED_EUCLIDEAN, coarse, lists, X, Q, 3, np.inf, m), name)
    ix.close()


def test_view_follows_the_call_and_the_rows():
    """unmasked, masked, unmasked on one handle; two masks in succession; an add between two masked calls"""
    rng = np.random.default_rng(13)
    coarse, lists, X, Q = _base(17, rng)
    X = np.nan_to_num(X, nan=0.0, posinf=1.0, neginf=-1.0)
    metric = K.MANHATTAN
    ix = _flat(coarse, metric, lists[:600], X[:600])
    first = ix.search(Q, 10, 3)
    _same(first, RI.search(metric, coarse, lists[:600], X[:600], Q, 3, 10))
    a, b = rng.random(600) < 0.5, rng.random(600) < 0.1
    _same(ix.search(Q, 10, 3, allowed=a), RIF.search(metric, coarse, lists[:600], X[:600], Q, 3, 10, a), "mask a")
    _same(ix.search(Q, 10, 3), first, "unmasked after masked")
    _same(ix.search(Q, 10, 3, allowed=b), RIF.search(metric, coarse, lists[:600], X[:600], Q, 3, 10, b), "mask b")
    _same(ix.search(Q, 10, 3, allowed=a), RIF.search(metric, coarse, lists[:600], X[:600], Q, 3, 10, a), "mask a again")
    _same_range(ix.range_search(Q, 25.0, 3, allowed=b), RIF.range_search(metric, coarse, lists[:600], X[:600], Q, 3, 25.0, b), "range b")
    _same_range(ix.range_search(Q, 25.0, 3), RR.search(metric, coarse, lists[:600], X[:600], Q, 3, 25.0), "unmasked range")
    assert np.array_equal(ix.add_rows(lists[600:], X[600:]), np.arange(600, N))
    import vq_amd

    with pytest.raises(vq_amd.DimensionMismatch):  # the mask of the index as it was
        ix.search(Q, 10, 3, allowed=a)
    c = rng.random(N) < 0.3
    _same(ix.search(Q, 10, 3, allowed=c), RIF.search(metric, coarse, lists, X, Q, 3, 10, c), "after add")
    _same_range(ix.range_search(Q, 25.0, 7, allowed=c), RIF.range_search(metric, coarse, lists, X, Q, 7, 25.0, c), "after add")
    ix.close()


@pytest.fixture(scope="module")
def two_batches():
    """1100 queries over 3000 rows: a batch holds at most 1024 queries"""
    rng = np.random.default_rng(3)
    n, d, nlist = 3000, 4, 6
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    X = (coarse[lists] + F(0.5) * rng.standard_normal((n, d))).astype(F)
    Q = rng.standard_normal((1100, d)).astype(F)
    m = rng.random(n) < 0.3
    return coarse, lists, X, Q, m, _flat(coarse, K.SQUARED_EUCLIDEAN, lists, X)


def test_two_batches(two_batches):
    coarse, lists, X, Q, m, ix = two_batches
    _same(ix.search(Q, 10, 2, allowed=m), RIF.search(K.SQUARED_EUCLIDEAN, coarse, lists, X, Q, 2, 10, m))


def test_range_two_batches_with_the_result_growing(two_batches):
    """a few thousand hits: the result buffers (1024 hits at first) grow in the first batch and again in the second"""
    coarse, lists, X, Q, m, ix = two_batches
    want = RIF.range_search(K.SQUARED_EUCLIDEAN, coarse, lists, X, Q, 2, 0.5, m)
    first, total = int(want[0][1024]), int(want[0][-1])
    assert 2 * 1024 < first < total < 10_000
    got = ix.range_search(Q, 0.5, 2, allowed=m)
    _same_range(got, want)
    assert m[got[1]].all()


@pytest.mark.parametrize("off", [1, 3])
def test_device_forms_at_offset_pointers(off):
    import torch

    import vq_amd

    rng = np.random.default_rng(off)
    d, nq, topk, nprobe = 37, 9, 17, 3
    coarse, lists, X, _ = _base(d, rng)
    Q = rng.standard_normal((nq, d)).astype(F)
    m = rng.random(N) < 0.3
    m[64:256] = False
    w = RF.pack(m)
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mb = torch.full((w.size + off + 8,), -1, dtype=torch.int32, device=dev)  # all ones around the mask
    mb[off:off + w.size] = torch.from_numpy(w.view(np.int32)).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    sq = SI.QUANTIZERS[0]
    codes = rng.integers(0, 256, (N, d)).astype(np.uint8)
    sx = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*sq), _dist(K.COSINE))
    sx.add_codes(lists, codes)
    for kind, ix, Xr in (("flat", _flat(coarse, K.COSINE, lists, X), X), ("scalar", sx, SI.decode(sq, codes))):
        ib.fill_(7)
        db.fill_(-1.0)
        ix.search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off, nprobe=nprobe,
                         dev_allowed=mb.data_ptr() + 4 * off)
        torch.cuda.synchronize()
        from vq_amd import _lib

        _lib.synchronize()
        gi = ib.cpu().numpy()
        gd = db.cpu().numpy()
        _same((gi[off:off + nq * topk].view(np.uint32).reshape(nq, topk), gd[off:off + nq * topk].reshape(nq, topk)),
              RIF.search(K.COSINE, coarse, lists, Xr, Q, nprobe, topk, m), kind)
        assert (gi[:off] == 7).all() and (gi[off + nq * topk:] == 7).all()
        assert (gd[:off] == -1.0).all() and (gd[off + nq * topk:] == -1.0).all()
        res = ix.range_search_device(qb.data_ptr() + 4 * off, nq, 0.8, nprobe=nprobe, dev_allowed=mb.data_ptr() + 4 * off)
        _same_range(res.read(), RIF.range_search(K.COSINE, coarse, lists, Xr, Q, nprobe, 0.8, m), kind)
        assert (mb.cpu().numpy()[off:off + w.size].view(np.uint32) == w).all()
        with pytest.raises(vq_amd.FfiError, match="aligned"):
            ix.search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr(), db.data_ptr(), nprobe=nprobe, dev_allowed=mb.data_ptr() + 2)
        ix.close()


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_range_radii(metric):
    """per-query radii with ties on the boundary, a radius that hits nothing, one that hits every allowed row, and the
    max_results error as the unmasked call reports it"""
    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(30 + metric)
    coarse, lists, X, Q = _base(5, rng)
    ix = _flat(coarse, metric, lists, X)
    m = _masks(lists, rng)["half"][0]
    Xa = np.nan_to_num(X[m], nan=0.0, posinf=3e38, neginf=-3e38)
    r = R.kth_distance(metric, Q, Xa, 25)  # the 25th allowed distance of each query: a hit exactly at the radius
    r[np.isnan(r)] = 1.0
    for nprobe in (2, 7):
        _same_range(ix.range_search(Q, r, nprobe, allowed=m), RIF.range_search(metric, coarse, lists, X, Q, nprobe, r, m), "per query")
        none = ix.range_search(Q, -1.0, nprobe, allowed=m)
        assert (none[0] == 0).all() and none[1].size == 0 and none[2].size == 0
        lims, idx, dist = ix.range_search(Q, np.inf, nprobe, allowed=m)
        _same_range((lims, idx, dist), RIF.range_search(metric, coarse, lists, X, Q, nprobe, np.inf, m), "radius +inf")
    P = RI.probe(metric, coarse, Q, 7)
    for j in range(Q.shape[0]):  # nprobe 7: exactly the allowed rows whose distance is not NaN
        dj = K.distances(metric, Q[j], X)
        assert np.isin(np.arange(NLIST), P[j]).all()
        assert idx[int(lims[j]):int(lims[j + 1])].tolist() == np.flatnonzero(m & ~np.isnan(dj)).tolist()
    want = RIF.range_search(metric, coarse, lists, X, Q, 3, np.inf, m)
    total = int(want[0][-1])
    with pytest.raises(vq_amd.FfiError) as e:
        ix.range_search(Q, np.inf, 3, max_results=total - 1, allowed=m)
    assert e.value.status == _lib.ERR_UNSUPPORTED and str(total) in str(e.value) and str(total - 1) in str(e.value)
    _same_range(ix.range_search(Q, np.inf, 3, max_results=total, allowed=m), want, "exactly at the cap")
    _same(ix.search(Q, 10, 3, allowed=m), RIF.search(metric, coarse, lists, X, Q, 3, 10, m), "the index is usable afterwards")
    ix.close()


@pytest.mark.parametrize("metric", [K.SQUARED_EUCLIDEAN, K.MANHATTAN, K.COSINE])
@pytest.mark.parametrize("d", [5, 20, 48])
def test_scalar_index_matches_statement_and_flat(metric, d):
    """d = 5, 20, 48: one, four and sixteen bytes per load of the code rows"""
    import vq_amd

    rng = np.random.default_rng(10 * metric + d)
    coarse, lists, _, Q = _base(d, rng)
    sq = SI.QUANTIZERS[2]
    codes = rng.integers(0, 17, (N, d)).astype(np.uint8)
    codes[200:203] = codes[20:23]
    codes[N - 3:] = codes[20:23]
    quant = vq_amd.ScalarQuantizer(*sq)
    Xd = SI.decode(sq, codes)
    Q = (Q * 0.5 + 1.0).astype(F)
    Q[0] = Xd[21]
    ix = vq_amd.IVFScalarIndex(coarse, quant, _dist(metric))
    ix.add_codes(lists, codes)
    fx = _flat(coarse, metric, lists, np.ascontiguousarray(quant.dequantize_batch(codes), dtype=F))
    sx = vq_amd.ScalarIndex.from_codes(codes, quant, _dist(metric))
    masks = _masks(lists, rng)
    r = R.kth_distance(metric, Q, Xd, 30)
    for nprobe in (1, 3, 7):
        for name, (m, arg) in masks.items():
            what = f"{name}, nprobe {nprobe}"
            got = ix.search(Q, 10, nprobe, allowed=arg)
            _same(got, RIF.sq_search(metric, coarse, lists, sq, codes, Q, nprobe, 10, m), what)
            _same(got, fx.search(Q, 10, nprobe, allowed=arg), what + " against the flat index")
            rgot = ix.range_search(Q, r, nprobe, allowed=arg)
            _same_range(rgot, RIF.sq_range_search(metric, coarse, lists, sq, codes, Q, nprobe, r, m), what)
            _same_range(rgot, fx.range_search(Q, r, nprobe, allowed=arg), what + " against the flat index")
            if nprobe == NLIST:
                _same(got, sx.search(Q, 10, allowed=arg), what + " against the masked ScalarIndex")
                _same_range(rgot, sx.range_search(Q, r, allowed=arg), what + " against the masked ScalarIndex")
            if name == "ones":
                _same(got, ix.search(Q, 10, nprobe), "all ones against the unmasked call")
    # rerank: the mask filters the first stage, so every candidate is an allowed row
    m = masks["half"][0]
    idx, dist = ix.search(Q, 5, 3, rerank=sx, candidates=20, allowed=m)
    real = idx != 0xFFFFFFFF
    assert m[idx[real]].all()
    first = ix.search(Q, 20, 3, allowed=m)[0]
    for j in range(Q.shape[0]):
        c = first[j][first[j] != 0xFFFFFFFF]
        if c.size == 20:
            wi, wd = K.rerank(metric, Q[j:j + 1], Xd, c[None, :], 5)
            assert np.array_equal(idx[j], wi[0]) and np.array_equal(dist[j].view(np.uint32), wd[0].view(np.uint32))
    ix.close()
    fx.close()


DRAWS = 40


def _draw(seed):
    rng = np.random.default_rng(91_000 + seed)
    n = int(rng.integers(1, 3001))
    d = int(rng.integers(1, 71))
    nlist = int(rng.integers(1, 41))
    nprobe = int(rng.integers(1, nlist + 1))
    metric = int(rng.integers(0, 5))
    kind = ["f32", "f16", "sq"][int(rng.integers(0, 3))]
    density = [0.0, -1.0, 0.01, 0.5, 1.0][int(rng.integers(0, 5))]  # -1: one row
    block = bool(rng.integers(0, 2))
    count = 1 if density < 0 else int(round(density * n))
    m = np.zeros(n, bool)
    if block:
        a = int(rng.integers(0, n - count + 1))
        m[a:a + count] = True
    else:
        m[rng.permutation(n)[:count]] = True
    return rng, n, d, nlist, nprobe, metric, kind, m, bool(rng.integers(0, 2))


@pytest.mark.parametrize("seed", range(DRAWS))
def test_random_draws(seed):
    import vq_amd

    rng, n, d, nlist, nprobe, metric, kind, m, ranged = _draw(seed)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    nq = [4, 40][int(rng.integers(0, 2))]  # 40: lists on the tile kernel
    Q = rng.standard_normal((nq, d)).astype(F)
    if kind == "sq":
        sq = SI.QUANTIZERS[int(rng.integers(0, 3))]
        codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
        X = SI.decode(sq, codes)
        ix = vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*sq), _dist(metric))
        ix.add_codes(lists, codes)
    else:
        X = (coarse[lists] + rng.standard_normal((n, d))).astype(F)
        if n > 8:
            X[n // 2] = np.nan
            X[n - 1] = X[0]
            lists[n - 1] = lists[0]
        Xt = X.astype(np.float16 if kind == "f16" else F)
        X = Xt.astype(F)
        ix = _flat(coarse, metric, lists, Xt)
    what = (f"seed {seed}: n {n} d {d} nlist {nlist} nprobe {nprobe} metric {metric} {kind} nq {nq} allowed {int(m.sum())} "
            f"{'range' if ranged else 'topk'}")
    if ranged:
        quant = float(rng.random())
        dall = np.stack([K.distances(metric, q, X) for q in Q])
        fin = np.where(np.isnan(dall), np.inf, dall)
        r = np.sort(fin, axis=1)[:, int(quant * (n - 1))].astype(F)  # the radius at the drawn quantile of the query's distances
        _same_range(ix.range_search(Q, r, nprobe, allowed=m), RIF.range_search(metric, coarse, lists, X, Q, nprobe, r, m), what)
    else:
        topk = int(rng.integers(1, min(n, 64) + 1))
        _same(ix.search(Q, topk, nprobe, allowed=RF.pack(m)), RIF.search(metric, coarse, lists, X, Q, nprobe, topk, m), what)
    ix.close()
