"""Filtered search on the MI355X (``allowed=`` of vq_amd.FlatIndex / ScalarIndex, vqhip_*_search_masked and
vqhip_*_range_search_masked, k_knn_dist_masked in vq_amd/csrc/knn_tile.hpp) against the numpy statement of
include/vqhip.h (tests/ref_filter.py): indices equal, distances equal as uint32 bits.  All five metrics, f32 and f16
rows, masks that skip whole row tiles and masks with edges inside tiles, sizes at which the mask has fewer words than
the last tile spans, fewer allowed rows than topk, stale workspace slots, dense ties under a mask, several batches, the
device form at offset pointers, range search, the scalar index, and seeded random draws."""
import numpy as np
import pytest

import ref_filter as RF
import ref_knn as K
import ref_range as R
import ref_sqindex as SI

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
N = 1037


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


def _data(n, d, rng, nq=5):
    """rows with the corner rows of ref_knn.special_rows at 7.., 130.. and 400.. and exact duplicates of rows 20..22 at
    200..202 and at the end; queries that equal a duplicated row, and the zero query"""
    X = (rng.standard_normal((n, d)) * 1.5).astype(F)
    sp = K.special_rows(d, rng)
    for at in (7, 130, 400):
        if at + len(sp) <= n:
            X[at:at + len(sp)] = sp
    if n > 210:
        X[200:203] = X[20:23]
        X[n - 3:] = X[20:23]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = X[21 % n]
    if nq > 3:
        Q[3] = 0.0
    return Q, X


def _masks(n, rng):
    """the masks of the issue over n = 1037 rows: name -> (bool mask, words handed to the index)"""
    def rand(p):
        m = rng.random(n) < p
        # the corner rows and the duplicates on both sides of the mask
        m[7:11], m[11:15] = True, False
        m[130:134], m[134:138] = False, True
        m[20], m[21], m[22] = True, False, True
        m[200], m[201], m[202] = False, True, False
        m[n - 3], m[n - 2], m[n - 1] = False, True, True
        return m

    def block(a, b):
        m = np.zeros(n, bool)
        m[a:b] = True
        return m

    one = lambda i: np.arange(n) == i
    half = rand(0.5)
    tail = RF.pack(half).copy()
    tail[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # every bit past n in the last word set
    out = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "row0": one(0), "last": one(n - 1), "half": rand(0.5),
           "3pc": rand(0.03), "tiles": block(128, 320), "edges": block(100, 333)}
    out = {k: (m, m) for k, m in out.items()}
    out["half+tail"] = (half, tail)
    return out


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("d", [1, 5, 129])
def test_search_matches_statement(metric, dtype, d):
    import vq_amd

    rng = np.random.default_rng(1000 * metric + d)
    Q, X = _data(N, d, rng)
    with np.errstate(over="ignore"):
        Xt = X.astype(dtype)
    Xw = Xt.astype(F)
    ix = vq_amd.FlatIndex(Xt, _dist(metric))
    plain = ix.search(Q, 10)
    for name, (m, arg) in _masks(N, rng).items():
        got = ix.search(Q, 10, allowed=arg)
        _same(got, RF.search(metric, Q, Xw, 10, m), name)
        if name == "ones":
            _same(got, plain, "all ones against the unmasked call")
        if name == "zeros":
            assert (got[0] == 0xFFFFFFFF).all() and np.isposinf(got[1]).all()
        assert not np.isin(got[0], np.flatnonzero(~m)).any(), name
    _same(ix.search(Q, 10), plain, "the unmasked call after masked ones")


@pytest.mark.parametrize("n", [1, 33, 64, 65, 96, 1040])
@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_word_boundary_sizes(n, metric):
    """n = 33, 65, 96: the last tile's second mask word does not exist; n = 1040: n % 4 == 0, the float4 stores"""
    import vq_amd

    rng = np.random.default_rng(n)
    Q = rng.standard_normal((3, 6)).astype(F)
    X = rng.standard_normal((n, 6)).astype(F)
    ix = vq_amd.FlatIndex(X, _dist(metric))
    topk = min(n, 5)
    masks = [rng.random(n) < 0.5, np.ones(n, bool), np.arange(n) == n - 1, np.arange(n) >= 32, np.arange(n) < 32, np.zeros(n, bool)]
    for j, m in enumerate(masks):
        w = RF.pack(m)
        assert w.shape == ((n + 31) // 32,)
        _same(ix.search(Q, topk, allowed=w), RF.search(metric, Q, X, topk, m), f"mask {j}")
        _same_range(ix.range_search(Q, np.inf, allowed=m), RF.range_search(metric, Q, X, np.inf, m), f"mask {j}")


def test_fewer_allowed_rows_than_topk():
    """7 allowed rows, 2 of them with NaN distances, topk 10: 5 finite, the 2 NaN rows in row order, 3 padding slots"""
    import vq_amd

    rng = np.random.default_rng(5)
    X = rng.standard_normal((500, 9)).astype(F)
    X[300, 2] = np.nan
    X[77, 0] = np.nan
    X[10, 3] = np.nan  # a NaN row that is not allowed
    allowed = [3, 77, 130, 131, 300, 420, 499]
    m = np.zeros(500, bool)
    m[allowed] = True
    Q = rng.standard_normal((4, 9)).astype(F)
    ix = vq_amd.FlatIndex(X, _dist(K.EUCLIDEAN))
    idx, dist = ix.search(Q, 10, allowed=m)
    _same((idx, dist), RF.search(K.EUCLIDEAN, Q, X, 10, m))
    for j in range(4):
        assert sorted(idx[j, :5].tolist()) == [3, 130, 131, 420, 499] and np.isfinite(dist[j, :5]).all()
        assert idx[j, 5:7].tolist() == [77, 300] and (dist[j, 5:7].view(np.uint32) == 0x7FC00000).all()
        assert (idx[j, 7:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, 7:]).all()


def test_topk_1024_with_600_allowed():
    import vq_amd

    rng = np.random.default_rng(6)
    X = rng.standard_normal((1029, 7)).astype(F)
    m = np.zeros(1029, bool)
    m[rng.permutation(1029)[:600]] = True
    Q = rng.standard_normal((3, 7)).astype(F)
    got = vq_amd.FlatIndex(X, _dist(K.MANHATTAN)).search(Q, 1024, allowed=m)
    _same(got, RF.search(K.MANHATTAN, Q, X, 1024, m))
    assert (got[0][:, 600:] == 0xFFFFFFFF).all() and (got[0][:, :600] != 0xFFFFFFFF).all()


def test_stale_workspace_of_an_unmasked_search():
    """the skipped tiles' slots hold the previous (unmasked) call's distances, its smallest among them: the queries equal
    disallowed rows, which must not appear"""
    import vq_amd

    rng = np.random.default_rng(7)
    n, d = 2000, 8
    X = rng.standard_normal((n, d)).astype(F)
    Q = X[[5, 70, 1999, 640]].copy()  # all in disallowed tiles
    m = np.zeros(n, bool)
    m[1024:1100] = True
    m[1500] = True
    ix = vq_amd.FlatIndex(X, _dist(K.SQUARED_EUCLIDEAN))
    first = ix.search(Q, 10)
    assert first[0][:, 0].tolist() == [5, 70, 1999, 640]
    got = ix.search(Q, 10, allowed=m)
    _same(got, RF.search(K.SQUARED_EUCLIDEAN, Q, X, 10, m))
    assert m[got[0]].all()
    rgot = ix.range_search(Q, np.inf, allowed=m)  # and the range stage over the same slots
    _same_range(rgot, RF.range_search(K.SQUARED_EUCLIDEAN, Q, X, np.inf, m))
    _same(ix.search(Q, 10), first)


@pytest.fixture(scope="module")
def ties():
    """20 000 equal rows under Manhattan (test_gpu_knn.py's dense ties), one index for the three masks"""
    import vq_amd

    X = np.ones((20_000, 16), F)
    X[5] = np.nan
    X[7000] = np.nan
    X[19_999] = 0.5
    Q = np.zeros((2, 16), F)
    Q[1] = 1.0
    return X, Q, vq_amd.FlatIndex(X, _dist(K.MANHATTAN))


def _tie_mask(which):
    rng = np.random.default_rng(11)
    m = np.zeros(20_000, bool)
    if which == "block":
        m[5000:] = True  # 15 000 tied allowed rows: the radix select, ties to the lowest allowed rows
    else:
        m[rng.permutation(20_000)[:9000 if which == "9000" else 4000]] = True  # 4000: more than 8192 tied positions, fewer allowed
    return m


@pytest.mark.parametrize("which", ["block", "9000", "4000"])
@pytest.mark.parametrize("topk", [1, 1024])
def test_dense_ties_under_a_mask(ties, which, topk):
    X, Q, ix = ties
    m = _tie_mask(which)
    got = ix.search(Q, topk, allowed=m)
    _same(got, RF.search(K.MANHATTAN, Q, X, topk, m))
    if which == "block" and topk == 1024:
        assert got[0][1].tolist() == list(range(5000, 6024))  # query 1: distance 0 to every equal row, the lowest allowed win


@pytest.fixture(scope="module")
def batches():
    """1100 queries over 300 007 rows, a random 10 % mask: 768 queries per batch, the second batch over stale slots"""
    import vq_amd

    rng = np.random.default_rng(3)
    X = rng.standard_normal((300_007, 4)).astype(F)
    Q = rng.standard_normal((1100, 4)).astype(F)
    m = rng.random(300_007) < 0.1
    return X, Q, m, vq_amd.FlatIndex(X, _dist(K.SQUARED_EUCLIDEAN))


def test_several_batches(batches):
    X, Q, m, ix = batches
    _same(ix.search(Q, 10, allowed=m), RF.search(K.SQUARED_EUCLIDEAN, Q, X, 10, m))


def test_range_several_batches_grow_twice(batches):
    """a few thousand hits: the result buffers (1024 hits at first) grow after the first batch and again after the second"""
    X, Q, m, ix = batches
    want = RF.range_search(K.SQUARED_EUCLIDEAN, Q, X, 0.06, m)
    first, total = int(want[0][768]), int(want[0][-1])
    assert 2 * 1024 < first < total < 10_000
    got = ix.range_search(Q, 0.06, allowed=m)
    _same_range(got, want)
    assert m[got[1]].all()


@pytest.mark.parametrize("off", [1, 3])
def test_device_form_at_offset_pointers(off):
    import torch

    import vq_amd

    rng = np.random.default_rng(off)
    d, nq, topk, n = 37, 9, 17, 2001
    Q, X = _data(n, d, rng, nq)
    m = rng.random(n) < 0.3
    m[64:256] = False
    w = RF.pack(m)
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mb = torch.full((w.size + off + 8,), -1, dtype=torch.int32, device=dev)  # all ones around the mask
    mb[off:off + w.size] = torch.from_numpy(w.view(np.int32)).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    for kind in ("flat", "scalar"):
        if kind == "flat":
            ix, Xr = vq_amd.FlatIndex(X, _dist(K.COSINE)), X
        else:
            sq = SI.QUANTIZERS[0]
            Xc = np.nan_to_num(X, nan=0.0, posinf=1.0, neginf=-1.0)
            ix = vq_amd.ScalarIndex(Xc, vq_amd.ScalarQuantizer(*sq), _dist(K.COSINE))
            Xr = SI.decode(sq, ix.codes())
        ib.fill_(7)
        db.fill_(-1.0)
        ix.search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off,
                         dev_allowed=mb.data_ptr() + 4 * off)
        torch.cuda.synchronize()
        gi = ib.cpu().numpy()
        gd = db.cpu().numpy()
        _same((gi[off:off + nq * topk].view(np.uint32).reshape(nq, topk), gd[off:off + nq * topk].reshape(nq, topk)),
              RF.search(K.COSINE, Q, Xr, topk, m), kind)
        assert (gi[:off] == 7).all() and (gi[off + nq * topk:] == 7).all()
        assert (gd[:off] == -1.0).all() and (gd[off + nq * topk:] == -1.0).all()
        res = ix.range_search_device(qb.data_ptr() + 4 * off, nq, 0.8, dev_allowed=mb.data_ptr() + 4 * off)
        _same_range(res.read(), RF.range_search(K.COSINE, Q, Xr, 0.8, m), kind)
        assert (mb.cpu().numpy()[off:off + w.size].view(np.uint32) == w).all()


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
@pytest.mark.parametrize("d", [5, 129])
def test_range_search_matches_statement(metric, d):
    import vq_amd

    rng = np.random.default_rng(100 * metric + d)
    Q, X = _data(N, d, rng)
    ix = vq_amd.FlatIndex(X, _dist(metric))
    r = R.kth_distance(metric, Q, X, 40)
    masks = _masks(N, rng)
    plain = ix.range_search(Q, r)
    for name in ("ones", "zeros", "tiles", "3pc", "edges", "half+tail"):
        m, arg = masks[name]
        got = ix.range_search(Q, r, allowed=arg)
        _same_range(got, RF.range_search(metric, Q, X, r, m), name)
        if name == "ones":
            _same_range(got, plain, "all ones against the unmasked call")
        if name == "zeros":
            assert (got[0] == 0).all() and got[1].size == 0
    m = masks["half"][0]
    lims, idx, dist = ix.range_search(Q, np.inf, allowed=m)
    _same_range((lims, idx, dist), RF.range_search(metric, Q, X, np.inf, m), "radius +inf")
    for j in range(Q.shape[0]):  # exactly the allowed rows whose distance is not NaN
        dj = K.distances(metric, Q[j], X)
        assert idx[int(lims[j]):int(lims[j + 1])].tolist() == np.flatnonzero(m & ~np.isnan(dj)).tolist()


def test_range_after_an_unmasked_topk_on_the_same_handle():
    """the skipped tiles' slots hold the distances of an unmasked top-k: none of them may hit"""
    import vq_amd

    rng = np.random.default_rng(9)
    n = 6000
    X = rng.standard_normal((n, 6)).astype(F)
    Q = X[[3, 4000, 5999]].copy()
    m = rng.random(n) < 0.5
    m[0:1024] = False  # whole tiles skipped, the first query's row among them
    ix = vq_amd.FlatIndex(X, _dist(K.EUCLIDEAN))
    ix.search(Q, 10)  # leaves every distance in the workspace
    got = ix.range_search(Q, 3.2, allowed=m)
    want = RF.range_search(K.EUCLIDEAN, Q, X, 3.2, m)
    unmasked = R.search(K.EUCLIDEAN, Q, X, 3.2)
    assert want[1].size > 2000 and (unmasked[1] < 1024).sum() > 300  # hits there are, and the skipped tiles would have had some
    _same_range(got, want)
    assert m[got[1]].all()


@pytest.mark.parametrize("metric", [K.SQUARED_EUCLIDEAN, K.COSINE])
@pytest.mark.parametrize("d", [1, 5, 129])
def test_scalar_index_matches_statement_and_flat(metric, d):
    import vq_amd

    rng = np.random.default_rng(10 * metric + d)
    sq = SI.QUANTIZERS[2]
    codes = rng.integers(0, 17, (N, d)).astype(np.uint8)
    codes[200:203] = codes[20:23]
    codes[N - 3:] = codes[20:23]
    quant = vq_amd.ScalarQuantizer(*sq)
    Xd = SI.decode(sq, codes)
    Q = rng.standard_normal((5, d)).astype(F)
    Q[0] = Xd[21]
    ix = vq_amd.ScalarIndex.from_codes(codes, quant, _dist(metric))
    fx = vq_amd.FlatIndex(np.ascontiguousarray(quant.dequantize_batch(codes), dtype=F), _dist(metric))
    for name, (m, arg) in _masks(N, rng).items():
        got = ix.search(Q, 10, allowed=arg)
        _same(got, RF.sq_search(metric, Q, sq, codes, 10, m), name)
        _same(got, fx.search(Q, 10, allowed=arg), name + " against the flat index")
    m = _masks(N, rng)["edges"][0]
    r = R.kth_distance(metric, Q, Xd, 30)
    got = ix.range_search(Q, r, allowed=m)
    _same_range(got, RF.sq_range_search(metric, Q, sq, codes, r, m))
    _same_range(got, fx.range_search(Q, r, allowed=m))


DRAWS = 40


def _draw(seed):
    rng = np.random.default_rng(77_000 + seed)
    n = int(rng.integers(1, 3001))
    d = int(rng.integers(1, 71))
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
    return rng, n, d, metric, kind, m, bool(rng.integers(0, 2))


@pytest.mark.parametrize("seed", range(DRAWS))
def test_random_draws(seed):
    import vq_amd

    rng, n, d, metric, kind, m, ranged = _draw(seed)
    Q = rng.standard_normal((4, d)).astype(F)
    if kind == "sq":
        sq = SI.QUANTIZERS[int(rng.integers(0, 3))]
        codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
        X = SI.decode(sq, codes)
        ix = vq_amd.ScalarIndex.from_codes(codes, vq_amd.ScalarQuantizer(*sq), _dist(metric))
    else:
        X = rng.standard_normal((n, d)).astype(F)
        if n > 8:
            X[n // 2] = np.nan
            X[n - 1] = X[0]
        Xt = X.astype(np.float16 if kind == "f16" else F)
        X = Xt.astype(F)
        ix = vq_amd.FlatIndex(Xt, _dist(metric))
    what = f"seed {seed}: n {n} d {d} metric {metric} {kind} allowed {int(m.sum())} {'range' if ranged else 'topk'}"
    if ranged:
        quant = float(rng.random())
        dall = np.stack([K.distances(metric, q, X) for q in Q])
        fin = np.where(np.isnan(dall), np.inf, dall)
        r = np.sort(fin, axis=1)[:, int(quant * (n - 1))].astype(F)  # the radius at the drawn quantile of the query's distances
        _same_range(ix.range_search(Q, r, allowed=m), RF.range_search(metric, Q, X, r, m), what)
    else:
        topk = int(rng.integers(1, min(n, 64) + 1))
        _same(ix.search(Q, topk, allowed=RF.pack(m)), RF.search(metric, Q, X, topk, m), what)
