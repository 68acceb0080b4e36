"""The asymmetric binary index on the MI355X (vq_amd.AsymmetricBinaryIndex, vqhip_abin_*, vq_amd/csrc/k_abin.hip with the
row source of bit_decode.hpp).  Every result is held three ways, each to indices and distance bits: against the numpy
statement (tests/ref_abin.py), against FlatIndex over the dequantized rows and against ScalarIndex over the bits as 0/1
bytes under ScalarQuantizer(low, high, 2).

The shapes are the smallest at which the kernel can go wrong: n on both sides of the 64-row tile and in several tiles
with a partial last one, d on both sides of the 32-dimension chunk (one word), in a partial last word and in 32 whole
words, nq on both sides of the 128-query tile, topk 1, 4 and min(n, 1024), three (low, high) pairs, all five metrics.
Rows without a set bit (a zero norm under cosine with low = 0: the EPSILON rule), rows of ones and duplicate rows (ties)
are planted; the queries hold NaN, +-inf and -0.0."""
import numpy as np
import pytest

import ref_abin as R
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
NS = [1, 63, 64, 65, 1501]
DIMS = [1, 31, 32, 33, 96, 100, 1024]
NQS = [1, 3, 129]


def _same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


def _same_range(got, want, what=""):
    for g, w, name in zip(got, want, ("lims", "idx", "dist")):
        assert g.shape == w.shape, f"{what}: {name} {g.shape} != {w.shape}"
        if name == "dist":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), f"{what}: {name}"


def _bits(n, d, rng):
    """bool (n, d): random rows with a row without a set bit, a row of ones and duplicates planted"""
    b = rng.random((n, d)) < 0.5
    if n >= 8:
        b[0] = False
        b[1] = True
        b[n - 1] = b[2]  # a tie across the whole index
        b[5] = b[4]      # a tie of neighbours
        b[n // 2] = False
    elif n == 1:
        b[0] = (d % 2 == 0)  # a row of ones or a row without a set bit
    return b


def _queries(nq, d, rng):
    Q = (rng.standard_normal((nq, d)) * 0.7 + 0.5).astype(F)
    Q[0, ::3] = -0.0
    if nq >= 3:
        Q[1, d // 2] = np.nan
        Q[2, 0] = np.inf
        Q[2, d - 1] = -np.inf if d > 1 else np.inf
    if nq >= 8:
        Q[3] = 0.0   # the zero query (cosine: the EPSILON rule)
        Q[4] = -0.0
        Q[5] = np.inf
        Q[6, d - 1] = np.nan
        Q[7] = 1.0   # parallel to a row of ones
    return Q


class _Case:
    """one set of rows under one (low, high) and metric: the three indexes over it"""

    def __init__(self, bits, low, high, metric):
        import vq_amd

        self.n, self.d = bits.shape
        self.low, self.high, self.metric = low, high, metric
        self.words = R.pack(bits)
        self.bq = vq_amd.BinaryQuantizer(0.0, low, high)
        self.dist = vq_amd.Distance(NAMES[metric])
        self.V = self.bq.dequantize_batch(self.bq.unpack_batch(self.words, self.d))
        assert np.array_equal(self.V.view(np.uint32), R.decode(self.words, self.d, low, high).view(np.uint32))
        self.abin = vq_amd.AsymmetricBinaryIndex.from_packed(self.words, self.d, self.bq, self.dist)
        self.flat = vq_amd.FlatIndex(self.V, self.dist)
        self.sq = vq_amd.ScalarIndex.from_codes(bits.astype(np.uint8), vq_amd.ScalarQuantizer(float(low), float(high), 2), self.dist)

    def matrix(self, Q):
        return R.distance_matrix(self.metric, Q, self.words, self.d, self.low, self.high)

    def three(self):
        return (("abin", self.abin), ("flat", self.flat), ("scalar", self.sq))


def _masks(n, rng):
    """random, contiguous, a 64-row tile without an allowed row (where there is more than one tile), all ones"""
    m_rand = rng.random(n) < 0.3
    m_run = np.zeros(n, bool)
    m_run[n // 3:n // 3 + max(1, n // 4)] = True
    m_hole = np.ones(n, bool)
    m_hole[:min(n, 64)] = False  # n <= 64: the empty mask, padding only
    if n > 128:
        m_hole[128:] = rng.random(n - 128) < 0.5
    return {"random": m_rand, "run": m_run, "empty tile": m_hole, "ones": np.ones(n, bool)}


def _radii(D):
    """per query a radius from its reference distances: below the least (no hit), the median, the greatest (every row
    whose distance is not NaN)"""
    r = np.zeros(D.shape[0], F)
    for j, row in enumerate(D):
        ok = row[~np.isnan(row)]
        if ok.size == 0:
            continue
        r[j] = (np.nextafter(ok.min(), F(-np.inf)), np.sort(ok)[ok.size // 2], ok.max())[j % 3]
    r[np.isnan(r)] = 0.0
    return r


def _check_calls(case, Q, rng, what):
    """search, filtered search, range search, filtered range search and rerank of one case, each three ways"""
    n = case.n
    D = case.matrix(Q)
    for topk in sorted({1, min(4, n), min(n, 1024)}):
        want = R.topk(D, topk)
        for name, ix in case.three():
            _same(ix.search(Q, topk), want, f"{what} search topk {topk} {name}")
    topk = min(4, n)
    for mname, m in _masks(n, rng).items():
        want = R.topk(D, topk, m)
        for name, ix in case.three():
            _same(ix.search(Q, topk, allowed=m), want, f"{what} search under the {mname} mask {name}")
    radii = _radii(D)
    want = R.ranged(D, radii)
    counts = np.diff(want[0].astype(np.int64))
    if Q.shape[0] >= 9:  # (the first eight queries hold the specials) the radii leave a query without a hit and one with hits
        assert counts.min() == 0 and counts.max() > 0
    for name, ix in case.three():
        _same_range(ix.range_search(Q, radii), want, f"{what} range {name}")
    m = _masks(n, rng)["random"]
    want = R.ranged(D, radii, m)
    for name, ix in case.three():
        _same_range(ix.range_search(Q, radii, allowed=m), want, f"{what} masked range {name}")
    for c in sorted({1, min(80, n)}):
        cand = np.stack([rng.choice(n, c, replace=False) for _ in range(Q.shape[0])])
        k = min(4, c)
        want = R.rerank(D, cand, k)
        for name, ix in case.three():
            _same(ix.rerank(Q, cand, k), want, f"{what} rerank c {c} {name}")


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_every_call_three_ways(metric, d):
    """every n of the grid at this (metric, d); nq and (low, high) rotate so that each meets every d and metric"""
    rng = np.random.default_rng(1000 * metric + d)
    di = DIMS.index(d)
    for ni, n in enumerate(NS):
        low, high = R.LOW_HIGH[(ni + di + metric) % 3]
        nq = NQS[(ni + di) % 3]
        case = _Case(_bits(n, d, rng), low, high, metric)
        _check_calls(case, _queries(nq, d, rng), rng, f"n {n} d {d} nq {nq} ({low}, {high}) {NAMES[metric]}")


@pytest.mark.parametrize("metric", K.METRICS)
def test_two_query_tiles_over_several_row_tiles(metric):
    """nq = 129 over n = 1501 at a partial last word, under every (low, high): the pairing the rotation above leaves out"""
    rng = np.random.default_rng(50 + metric)
    bits = _bits(1501, 100, rng)
    Q = _queries(129, 100, rng)
    for low, high in R.LOW_HIGH:
        case = _Case(bits, low, high, metric)
        D = case.matrix(Q)
        for topk in (1, 4, 1024):
            want = R.topk(D, topk)
            for name, ix in case.three():
                _same(ix.search(Q, topk), want, f"({low}, {high}) topk {topk} {name}")


def test_zero_norm_rows_take_the_epsilon_rule():
    """cosine with low = 0: a row without a set bit has norm 0 and distance exactly 1 from every query without NaN"""
    rng = np.random.default_rng(3)
    case = _Case(_bits(65, 33, rng), 0, 1, K.COSINE)
    Q = rng.standard_normal((3, 33)).astype(F)
    idx, dist = case.abin.search(Q, 65)
    for j in range(3):
        assert dist[j][idx[j] == 0][0] == F(1.0)
    _same((idx, dist), R.topk(case.matrix(Q), 65))


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_rerank_of_4096_candidates(metric):
    rng = np.random.default_rng(7 + metric)
    n, d, nq = 4100, 33, 3
    case = _Case(_bits(n, d, rng), 3, 200, metric)
    Q = _queries(nq, d, rng)
    D = case.matrix(Q)
    cand = np.stack([rng.choice(n, 4096, replace=False) for _ in range(nq)])
    for k in (1, 4096):
        want = R.rerank(D, cand, k)
        for name, ix in case.three():
            _same(ix.rerank(Q, cand, k), want, f"rerank of 4096, topk {k}, {name}")


def test_rerank_id_past_n_is_refused_as_the_siblings_refuse_it():
    import vq_amd
    from vq_amd import _lib

    words = np.zeros((20, 1), np.uint32)
    ix = vq_amd.AsymmetricBinaryIndex.from_packed(words, 4)
    q = np.zeros((2, 4), F)
    with pytest.raises(vq_amd.InvalidParameter, match="outside"):
        ix.rerank(q, np.array([[0, 1, 20], [2, 3, 4]]), 2)
    h = _lib.ABin(words, _lib.BINARY_PACKED, 20, 4, 0.0, 0, 1, K.EUCLIDEAN)
    try:
        with pytest.raises(vq_amd.FfiError, match="candidate row id") as e:
            h.rerank(q, np.array([[0, 1, 0xFFFFFFFF], [2, 3, 20]], np.uint32), 2)
        assert e.value.status == _lib.ERR_INVALID_INPUT
        i, _ = h.rerank(q, np.array([[0, 1, 19], [2, 3, 4]], np.uint32), 3)
        assert i.tolist() == [[0, 1, 19], [2, 3, 4]]
    finally:
        h.close()


@pytest.mark.parametrize("metric", [K.MANHATTAN, K.COSINE])
def test_device_forms_at_an_unaligned_query_pointer(metric):
    """search_device, its masked form and the two range forms with the queries, the mask and the results one element
    off a 16-byte boundary; a query pointer off a 4-byte boundary is refused"""
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(11 + metric)
    n, d, nq, topk, off = 1501, 100, 9, 4, 1
    case = _Case(_bits(n, d, rng), 3, 200, metric)
    Q = _queries(nq, d, rng)
    D = case.matrix(Q)
    m = _masks(n, rng)["random"]
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mw = vq_amd.pack_row_mask(m, n)
    mb = torch.zeros(mw.size + off + 8, dtype=torch.int32, device=dev)
    mb[off:off + mw.size] = torch.from_numpy(mw.view(np.int32)).to(dev)
    qp, mp = qb.data_ptr() + 4 * off, mb.data_ptr() + 4 * off
    assert qp % 16 != 0
    for allowed, want in ((None, R.topk(D, topk)), (mp, R.topk(D, topk, m))):
        ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
        db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        case.abin.search_device(qp, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off, allowed)
        _lib.synchronize()
        torch.cuda.synchronize()
        ih, dh = ib.cpu().numpy(), db.cpu().numpy()
        _same((ih[off:off + nq * topk].view(np.uint32).reshape(nq, topk), dh[off:off + nq * topk].reshape(nq, topk)), want)
        assert (ih[:off] == 7).all() and (ih[off + nq * topk:] == 7).all()
        assert (dh[:off] == -1).all() and (dh[off + nq * topk:] == -1).all()
    radii = _radii(D)
    _same_range(case.abin.range_search_device(qp, nq, radii).read(), R.ranged(D, radii))
    _same_range(case.abin.range_search_device(qp, nq, radii, dev_allowed=mp).read(), R.ranged(D, radii, m))
    ib = torch.zeros(nq * topk, dtype=torch.int32, device=dev)
    db = torch.zeros(nq * topk, dtype=torch.float32, device=dev)
    with pytest.raises(vq_amd.FfiError, match="4-byte aligned") as e:
        case.abin.search_device(qb.data_ptr() + 2, nq, topk, ib.data_ptr(), db.data_ptr())
    assert e.value.status == _lib.ERR_INVALID_INPUT


# ---- per index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 64])
def test_the_three_create_kinds_agree(d):
    """f32 rows, u8 codes and packed words of the same bits, from host and from device memory: the same words, the same
    search, and the words BinaryIndex keeps for the same source"""
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(d)
    n = 1501
    bq = vq_amd.BinaryQuantizer(0.25, 3, 200)
    X = rng.standard_normal((n, d)).astype(F)
    X[3, 2], X[4, 0], X[5, 1], X[6, 0] = np.nan, 0.25, np.inf, -0.0
    codes = bq.quantize_batch(X)
    words = R.pack(X >= F(0.25))
    assert np.array_equal(words, vq_amd.BinaryIndex(X, bq).packed())
    dist = vq_amd.Distance.cosine()
    Q = _queries(5, d, rng)
    want = R.search(K.COSINE, Q, words, d, 3, 200, 10)
    made = [vq_amd.AsymmetricBinaryIndex(X, bq, dist), vq_amd.AsymmetricBinaryIndex.from_codes(codes, bq, dist),
            vq_amd.AsymmetricBinaryIndex.from_packed(words, d, bq, dist)]
    for ix in made:
        _same(ix.search(Q, 10), want)
        assert np.array_equal(ix.packed(), words)
    for kind, src in ((_lib.BINARY_F32, X), (_lib.BINARY_U8, codes), (_lib.BINARY_PACKED, words)):
        t = torch.from_numpy(src.view(np.int32) if src.dtype == np.uint32 else src).cuda()
        torch.cuda.synchronize()
        h = _lib.ABin(None, kind, n, d, 0.25, 3, 200, K.COSINE, dev_src=t.data_ptr())
        try:
            assert np.array_equal(h.packed(), words)
            _same(h.search(Q, 10), want)
        finally:
            h.close()


def test_a_pad_bit_on_the_device_is_refused_and_leaves_the_index():
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(5)
    n, d = 70, 33
    words = R.pack(_bits(n, d, rng))
    bad = words.copy()
    bad[40, 1] |= np.uint32(1 << 7)
    t = torch.from_numpy(bad.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(vq_amd.FfiError, match="pad bit") as e:
        _lib.ABin(None, _lib.BINARY_PACKED, n, d, 0.0, 0, 1, K.EUCLIDEAN, dev_src=t.data_ptr())
    assert e.value.status == _lib.ERR_INVALID_INPUT
    ix = vq_amd.AsymmetricBinaryIndex.from_packed(words, d)
    Q = _queries(3, d, rng)
    before = ix.search(Q, 5)
    with pytest.raises(vq_amd.FfiError, match="pad bit"):
        ix.add_packed_device(t.data_ptr(), n)
    assert len(ix) == n and np.array_equal(ix.packed(), words)
    _same(ix.search(Q, 5), before)


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE, K.COSINE_UNCLAMPED])
def test_add_then_remove_equals_a_fresh_index(metric):
    """add (f32 rows), add_codes, add_packed and add_packed_device, then remove_rows of a random fifth with row 0 and
    row n - 1: every call equals a fresh index over the remaining rows, the moved cosine norms included"""
    import torch

    import vq_amd

    rng = np.random.default_rng(20 + metric)
    d = 100
    bq = vq_amd.BinaryQuantizer(0.0, 3, 200)
    dist = vq_amd.Distance(NAMES[metric])
    parts = [_bits(65, d, rng), _bits(700, d, rng), _bits(1, d, rng), _bits(130, d, rng), _bits(63, d, rng)]
    ix = vq_amd.AsymmetricBinaryIndex.from_packed(R.pack(parts[0]), d, bq, dist)
    X = np.where(parts[1], F(0.5), F(-0.5)).astype(F)
    assert ix.add(X).tolist() == list(range(65, 765))
    ix.add_codes(np.where(parts[2], np.uint8(200), np.uint8(199)))
    ix.add_packed(R.pack(parts[3]))
    t = torch.from_numpy(R.pack(parts[4]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    ix.add_packed_device(t.data_ptr(), 63)
    bits = np.concatenate(parts)
    n = bits.shape[0]
    assert len(ix) == n and np.array_equal(ix.packed(), R.pack(bits))
    Q = _queries(5, d, rng)
    _same(ix.search(Q, 10), R.search(metric, Q, R.pack(bits), d, 3, 200, 10), "after the adds")
    gone = rng.random(n) < 0.2
    gone[0] = gone[n - 1] = True
    kept = ix.remove_rows(gone)
    assert np.array_equal(kept, np.flatnonzero(~gone))
    left = bits[~gone]
    fresh = vq_amd.AsymmetricBinaryIndex.from_packed(R.pack(left), d, bq, dist)
    assert len(ix) == left.shape[0] and np.array_equal(ix.packed(), R.pack(left))
    D = R.distance_matrix(metric, Q, R.pack(left), d, 3, 200)
    m = rng.random(left.shape[0]) < 0.5
    radii = _radii(D)
    cand = np.stack([rng.choice(left.shape[0], 80, replace=False) for _ in range(5)])
    for name, x in (("mutated", ix), ("fresh", fresh)):
        _same(x.search(Q, 10), R.topk(D, 10), name)
        _same(x.search(Q, 10, allowed=m), R.topk(D, 10, m), name)
        _same_range(x.range_search(Q, radii), R.ranged(D, radii), name)
        _same(x.rerank(Q, cand, 10), R.rerank(D, cand, 10), name)


def test_save_load_of_an_index_built_from_rows(tmp_path):
    import vq_amd

    rng = np.random.default_rng(71)
    bq = vq_amd.BinaryQuantizer(0.5, 3, 200)
    X = rng.standard_normal((1501, 33)).astype(F)
    ix = vq_amd.AsymmetricBinaryIndex(X, bq, vq_amd.Distance.cosine())
    ix.save(tmp_path / "rows.vqabin")
    back = vq_amd.AsymmetricBinaryIndex.load(tmp_path / "rows.vqabin")
    words = R.pack(X >= F(0.5))
    assert np.array_equal(back.packed(), words) and np.array_equal(ix.packed(), words)
    assert back.distance == ix.distance and repr(back.quantizer) == repr(bq) and back.dim == 33 and len(back) == 1501
    Q = _queries(5, 33, rng)
    _same(back.search(Q, 10), ix.search(Q, 10))
    _same(back.search(Q, 10), R.search(K.COSINE, Q, words, 33, 3, 200, 10))


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_binary_search_reranked_through_the_asymmetric_twin(metric):
    """BinaryIndex.search(..., rerank=abin, candidates=80) = the Hamming short list rescored by the numpy statement"""
    import vq_amd

    rng = np.random.default_rng(51 + metric)
    n, d = 4000, 96
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((12, d)).astype(F)
    b = vq_amd.BinaryIndex(X)
    abin = vq_amd.AsymmetricBinaryIndex.from_packed(b.packed(), b.dim, b.quantizer, vq_amd.Distance(NAMES[metric]))
    short, _ = b.search(Q, 80)
    D = R.distance_matrix(metric, Q, b.packed(), d, 0, 1)
    _same(b.search(Q, 10, rerank=abin, candidates=80), R.rerank(D, short, 10))
    short, _ = b.search(Q, 40)
    _same(b.search(Q, 10, rerank=abin), R.rerank(D, short, 10))


def test_ivfpq_search_accepts_the_index_as_reranker():
    import vq_amd

    rng = np.random.default_rng(12)
    n, d = 3000, 32
    X = rng.standard_normal((n, d)).astype(F)
    coarse = X[rng.choice(n, 16, replace=False)]
    cb = (rng.standard_normal((8, 64, 4)) * 0.5).astype(F)
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean())
    ix.add(X)
    abin = vq_amd.AsymmetricBinaryIndex(X)
    flat = vq_amd.FlatIndex(R.decode(abin.packed(), d, 0, 1), vq_amd.Distance.euclidean())
    Q = rng.standard_normal((7, d)).astype(F)
    _same(ix.search(Q, topk=10, nprobe=4, rerank=abin, candidates=64), ix.search(Q, topk=10, nprobe=4, rerank=flat, candidates=64))
    ix.close()


def test_two_runs_are_identical():
    rng = np.random.default_rng(99)
    case = _Case(_bits(1501, 100, rng), 3, 200, K.COSINE)
    Q = _queries(129, 100, rng)
    radii = _radii(case.matrix(Q))
    a, b = case.abin.search(Q, 10), case.abin.search(Q, 10)
    _same(a, b)
    _same_range(case.abin.range_search(Q, radii), case.abin.range_search(Q, radii))
