"""The 4-bit scalar index on the MI355X (vq_amd.Scalar4Index, vqhip_sq4index_*, vq_amd/csrc/k_sq4index.hip with the row
source of nibble_decode.hpp).  Every result is held three ways, each to indices and distance bits: against the numpy
statement (tests/ref_sq4.py), against ScalarIndex over the same codes as bytes and against FlatIndex over the
dequantized rows.

The shapes are the smallest at which the kernel can go wrong: n on both sides of the 64-row tile and in several tiles
with a partial last one; d on both sides of a word (8 dimensions), of the 32-dimension chunk and of a chunk's last
partial word, and 32 whole chunks; nq on both sides of the 128-query tile; topk 1, 4 and min(n, 1024); four quantizers;
all five metrics.  Codes >= levels up to 15, rows of all-zero codes (a zero norm under cosine where min = 0: the EPSILON
rule) and duplicate rows (ties) are planted; the queries hold NaN, +-inf and -0.0.  One reference matrix per case is
shared by every call held to it."""
import numpy as np
import pytest

import ref_knn as K
import ref_sq4 as R

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
NS = [1, 63, 64, 65, 1501]
DIMS = [1, 7, 8, 9, 31, 32, 33, 40, 100, 1024]
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


def _codes(n, d, rng):
    """uint8 (n, d) over all 16 nibble values (so codes >= levels wherever levels < 16), with rows of zeros, a row of
    15s and duplicates planted"""
    c = rng.integers(0, 16, (n, d), dtype=np.uint8)
    if n >= 8:
        c[0] = 0
        c[1] = 15
        c[n - 1] = c[2]  # a tie across the whole index
        c[5] = c[4]      # a tie of neighbours
        c[n // 2] = 0
    elif n == 1:
        c[0] = 0 if d % 2 else c[0]
    return c


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
        Q[7] = 1.0
    return Q


class _Case:
    """one set of codes under one quantizer and metric: the three indexes over it"""

    def __init__(self, codes, quant, metric):
        import vq_amd

        self.n, self.d = codes.shape
        self.quant, self.metric = quant, metric
        self.codes = codes
        self.words = R.pack4(codes)
        self.sqz = vq_amd.ScalarQuantizer(*quant)
        self.dist = vq_amd.Distance(NAMES[metric])
        self.V = self.sqz.dequantize_batch(codes)
        assert np.array_equal(self.V.view(np.uint32), R.decode(self.words, self.d, *quant).view(np.uint32))
        self.sq4 = vq_amd.Scalar4Index.from_packed(self.words, self.d, self.sqz, self.dist)
        self.sq8 = vq_amd.ScalarIndex.from_codes(codes, self.sqz, self.dist)
        self.flat = vq_amd.FlatIndex(self.V, self.dist)

    def matrix(self, Q):
        return R.matrix_over(self.metric, Q, self.V)

    def three(self):
        return (("sq4", self.sq4), ("scalar", self.sq8), ("flat", self.flat))


def _masks(n, rng):
    """every row, none but one, a contiguous block, random"""
    m_one = np.zeros(n, bool)
    m_one[n // 2] = True
    m_run = np.zeros(n, bool)
    m_run[n // 3:n // 3 + max(1, n // 4)] = True
    return {"ones": np.ones(n, bool), "one row": m_one, "run": m_run, "random": rng.random(n) < 0.3}


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
    masks = _masks(n, rng)
    for mname, m in masks.items():
        want = R.topk(D, topk, m)
        for name, ix in case.three():
            _same(ix.search(Q, topk, allowed=m), want, f"{what} search under the {mname} mask {name}")
    radii = _radii(D)
    want = R.ranged(D, radii)
    for name, ix in case.three():
        _same_range(ix.range_search(Q, radii), want, f"{what} range {name}")
    want = R.ranged(D, radii, masks["random"])
    for name, ix in case.three():
        _same_range(ix.range_search(Q, radii, allowed=masks["random"]), want, f"{what} masked range {name}")
    for c in sorted({1, min(80, n)}):
        cand = np.stack([rng.choice(n, c, replace=False) for _ in range(Q.shape[0])])
        k = min(4, c)
        want = R.rerank(D, cand, k)
        for name, ix in case.three():
            _same(ix.rerank(Q, cand, k), want, f"{what} rerank c {c} {name}")


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_every_call_three_ways(metric, d):
    """every n of the grid at this (metric, d); nq and the quantizer rotate so that each meets every d and metric.  At
    d = 1024 the 129 queries meet n = 65, not n = 1501 (the reference matrix of that pair alone takes a second; two
    query tiles over several row tiles are the next test's)."""
    rng = np.random.default_rng(1000 * metric + d)
    di = DIMS.index(d)
    for ni, n in enumerate(NS):
        quant = R.QUANTIZERS[(ni + di + metric) % 4]
        nq = NQS[(ni + di) % 3]
        if d == 1024 and n == 1501:
            nq = 3
        if d == 1024 and n == 65:
            nq = 129
        case = _Case(_codes(n, d, rng), quant, metric)
        _check_calls(case, _queries(nq, d, rng), rng, f"n {n} d {d} nq {nq} {quant} {NAMES[metric]}")


@pytest.mark.parametrize("metric", K.METRICS)
def test_two_query_tiles_over_several_row_tiles(metric):
    """nq = 129 over n = 1501 at a chunk's last partial word, under every quantizer, topk up to 1024"""
    rng = np.random.default_rng(50 + metric)
    codes = _codes(1501, 100, rng)
    Q = _queries(129, 100, rng)
    for quant in R.QUANTIZERS:
        case = _Case(codes, quant, metric)
        D = case.matrix(Q)
        for topk in (1, 4, 1024):
            want = R.topk(D, topk)
            for name, ix in case.three():
                _same(ix.search(Q, topk), want, f"{quant} topk {topk} {name}")


def test_zero_norm_rows_take_the_epsilon_rule():
    """cosine with min = 0: a row of zero codes has norm 0 and distance exactly 1 from every query without NaN"""
    rng = np.random.default_rng(3)
    case = _Case(_codes(65, 33, rng), (0.0, 15.0, 16), K.COSINE)
    Q = rng.standard_normal((3, 33)).astype(F)
    idx, dist = case.sq4.search(Q, 65)
    for j in range(3):
        assert dist[j][idx[j] == 0][0] == F(1.0)
    _same((idx, dist), R.topk(case.matrix(Q), 65))


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_rerank_of_4096_candidates(metric):
    rng = np.random.default_rng(7 + metric)
    n, d, nq = 4100, 33, 3
    case = _Case(_codes(n, d, rng), (-3.5, 200.0, 5), metric)
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
    ix = vq_amd.Scalar4Index.from_packed(words, 4, vq_amd.ScalarQuantizer(-1.0, 1.0, 16))
    q = np.zeros((2, 4), F)
    with pytest.raises(vq_amd.InvalidParameter, match="outside"):
        ix.rerank(q, np.array([[0, 1, 20], [2, 3, 4]]), 2)
    h = _lib.SQ4Index(words, _lib.SQ4_PACKED, 20, 4, -1.0, 1.0, 16, K.EUCLIDEAN)
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
    case = _Case(_codes(n, d, rng), (-1.0, 1.0, 16), metric)
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
        case.sq4.search_device(qp, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off, allowed)
        _lib.synchronize()
        torch.cuda.synchronize()
        ih, dh = ib.cpu().numpy(), db.cpu().numpy()
        _same((ih[off:off + nq * topk].view(np.uint32).reshape(nq, topk), dh[off:off + nq * topk].reshape(nq, topk)), want)
        assert (ih[:off] == 7).all() and (ih[off + nq * topk:] == 7).all()
        assert (dh[:off] == -1).all() and (dh[off + nq * topk:] == -1).all()
    radii = _radii(D)
    _same_range(case.sq4.range_search_device(qp, nq, radii).read(), R.ranged(D, radii))
    _same_range(case.sq4.range_search_device(qp, nq, radii, dev_allowed=mp).read(), R.ranged(D, radii, m))
    ib = torch.zeros(nq * topk, dtype=torch.int32, device=dev)
    db = torch.zeros(nq * topk, dtype=torch.float32, device=dev)
    with pytest.raises(vq_amd.FfiError, match="4-byte aligned") as e:
        case.sq4.search_device(qb.data_ptr() + 2, nq, topk, ib.data_ptr(), db.data_ptr())
    assert e.value.status == _lib.ERR_INVALID_INPUT


# ---- per index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [33, 64])
def test_the_three_create_kinds_agree(d):
    """f32 rows, u8 codes and packed words of the same rows, from host and from device memory: the same words --
    pack4_codes(quantize_batch(rows)) -- and the same search.  d = 64 takes the pack kernel's 8-byte loads, d = 33 its
    byte loads and a partial last word."""
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(d)
    n = 1501
    quant = (-1.0, 1.0, 16)
    sqz = vq_amd.ScalarQuantizer(*quant)
    X = (rng.standard_normal((n, d)) * 0.6).astype(F)
    X[3, 2], X[4, 0], X[5, 1], X[6, 0], X[7, 1] = np.nan, 1.0, np.inf, -0.0, -np.inf
    codes = sqz.quantize_batch(X)
    assert int(codes.max()) == 15 and int(codes.min()) == 0
    words = vq_amd.ScalarQuantizer.pack4_codes(codes)
    assert np.array_equal(words, R.pack4(codes))
    dist = vq_amd.Distance.cosine()
    Q = _queries(5, d, rng)
    want = R.search(K.COSINE, Q, words, d, *quant, 10)
    made = [vq_amd.Scalar4Index(X, sqz, dist), vq_amd.Scalar4Index.from_codes(codes, sqz, dist),
            vq_amd.Scalar4Index.from_packed(words, d, sqz, dist)]
    for ix in made:
        _same(ix.search(Q, 10), want)
        assert np.array_equal(ix.packed(), words) and np.array_equal(ix.codes(), codes)
    for kind, src in ((_lib.SQ4_F32, X), (_lib.SQ4_U8, codes), (_lib.SQ4_PACKED, words)):
        t = torch.from_numpy(src.view(np.int32) if src.dtype == np.uint32 else src).cuda()
        torch.cuda.synchronize()
        h = _lib.SQ4Index(None, kind, n, d, *quant, K.COSINE, dev_src=t.data_ptr())
        try:
            assert np.array_equal(h.packed(), words)
            _same(h.search(Q, 10), want)
        finally:
            h.close()


def test_a_code_of_16_and_a_pad_nibble_on_the_device_are_refused_and_leave_the_index():
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(5)
    n, d = 70, 33
    quant = (-1.0, 1.0, 16)
    sqz = vq_amd.ScalarQuantizer(*quant)
    codes = _codes(n, d, rng)
    words = R.pack4(codes)
    bad_words = words.copy()
    bad_words[40, 4] |= np.uint32(1 << 4)  # dimension 33 of a row of 33
    bad_codes = codes.copy()
    bad_codes[69, 32] = 16
    tw = torch.from_numpy(bad_words.view(np.int32)).cuda()
    tc = torch.from_numpy(bad_codes).cuda()
    torch.cuda.synchronize()
    with pytest.raises(vq_amd.FfiError, match="pad nibble") as e:
        _lib.SQ4Index(None, _lib.SQ4_PACKED, n, d, *quant, K.EUCLIDEAN, dev_src=tw.data_ptr())
    assert e.value.status == _lib.ERR_INVALID_INPUT
    with pytest.raises(vq_amd.FfiError, match="code above 15") as e:
        _lib.SQ4Index(None, _lib.SQ4_U8, n, d, *quant, K.EUCLIDEAN, dev_src=tc.data_ptr())
    assert e.value.status == _lib.ERR_INVALID_INPUT
    for metric in (K.EUCLIDEAN, K.COSINE):
        ix = vq_amd.Scalar4Index.from_packed(words, d, sqz, vq_amd.Distance(NAMES[metric]))
        Q = _queries(3, d, rng)
        before = ix.search(Q, 5)
        with pytest.raises(vq_amd.FfiError, match="pad nibble"):
            ix.add_packed_device(tw.data_ptr(), n)
        with pytest.raises(vq_amd.FfiError, match="code above 15"):
            ix.add_codes_device(tc.data_ptr(), n)
        assert len(ix) == n and np.array_equal(ix.packed(), words)
        _same(ix.search(Q, 5), before)
        _same(before, R.search(metric, Q, words, d, *quant, 5))


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE, K.COSINE_UNCLAMPED])
def test_add_then_remove_equals_a_fresh_index(metric):
    """add (f32 rows), add_codes, add_packed, add_codes_device and add_packed_device, then remove_rows of a random fifth
    with row 0 and row n - 1: every call equals a fresh index over the remaining rows, the moved cosine norms included"""
    import torch

    import vq_amd

    rng = np.random.default_rng(20 + metric)
    d = 100
    quant = (0.0, 15.0, 16)
    sqz = vq_amd.ScalarQuantizer(*quant)
    dist = vq_amd.Distance(NAMES[metric])
    parts = [_codes(65, d, rng), _codes(700, d, rng), _codes(1, d, rng), _codes(130, d, rng), _codes(63, d, rng), _codes(9, d, rng)]
    ix = vq_amd.Scalar4Index.from_packed(R.pack4(parts[0]), d, sqz, dist)
    X = parts[1].astype(F)  # (0, 15, 16): the value c has code c
    assert np.array_equal(sqz.quantize_batch(X), parts[1])
    assert ix.add(X).tolist() == list(range(65, 765))
    ix.add_codes(parts[2])
    ix.add_packed(R.pack4(parts[3]))
    t = torch.from_numpy(R.pack4(parts[4]).view(np.int32)).cuda()
    tc = torch.from_numpy(parts[5]).cuda()
    torch.cuda.synchronize()
    ix.add_packed_device(t.data_ptr(), 63)
    assert ix.add_codes_device(tc.data_ptr(), 9).tolist() == list(range(959, 968))
    codes = np.concatenate(parts)
    n = codes.shape[0]
    assert len(ix) == n and np.array_equal(ix.packed(), R.pack4(codes))
    Q = _queries(5, d, rng)
    _same(ix.search(Q, 10), R.search(metric, Q, R.pack4(codes), d, *quant, 10), "after the adds")
    gone = rng.random(n) < 0.2
    gone[0] = gone[n - 1] = True
    kept = ix.remove_rows(gone)
    assert np.array_equal(kept, np.flatnonzero(~gone))
    left = codes[~gone]
    fresh = vq_amd.Scalar4Index.from_codes(left, sqz, dist)
    assert len(ix) == left.shape[0] and np.array_equal(ix.packed(), R.pack4(left))
    D = R.distance_matrix(metric, Q, R.pack4(left), d, *quant)
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
    quant = (-3.5, 200.0, 5)
    sqz = vq_amd.ScalarQuantizer(*quant)
    X = (rng.standard_normal((1501, 33)) * 80 + 90).astype(F)
    ix = vq_amd.Scalar4Index(X, sqz, vq_amd.Distance.cosine())
    ix.save(tmp_path / "rows.vqsq4")
    back = vq_amd.Scalar4Index.load(tmp_path / "rows.vqsq4")
    words = R.pack4(sqz.quantize_batch(X))
    assert np.array_equal(back.packed(), words) and np.array_equal(ix.packed(), words)
    assert back.distance == ix.distance and repr(back.quantizer) == repr(sqz) and back.dim == 33 and len(back) == 1501
    Q = _queries(5, 33, rng)
    _same(back.search(Q, 10), ix.search(Q, 10))
    _same(back.search(Q, 10), R.search(K.COSINE, Q, words, 33, *quant, 10))


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
def test_binary_search_reranked_through_the_index(metric):
    """BinaryIndex.search(..., rerank=sq4, candidates=80) = the Hamming short list rescored by the numpy statement"""
    import vq_amd

    rng = np.random.default_rng(51 + metric)
    n, d = 4000, 96
    quant = (-3.0, 3.0, 16)
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((12, d)).astype(F)
    b = vq_amd.BinaryIndex(X)
    sq4 = vq_amd.Scalar4Index(X, vq_amd.ScalarQuantizer(*quant), vq_amd.Distance(NAMES[metric]))
    D = R.distance_matrix(metric, Q, sq4.packed(), d, *quant)
    short, _ = b.search(Q, 80)
    _same(b.search(Q, 10, rerank=sq4, candidates=80), R.rerank(D, short, 10))
    short, _ = b.search(Q, 40)
    _same(b.search(Q, 10, rerank=sq4), R.rerank(D, short, 10))


def test_ivfpq_search_accepts_the_index_as_reranker():
    import vq_amd

    rng = np.random.default_rng(12)
    n, d = 3000, 32
    quant = (-3.0, 3.0, 16)
    X = rng.standard_normal((n, d)).astype(F)
    coarse = X[rng.choice(n, 16, replace=False)]
    cb = (rng.standard_normal((8, 64, 4)) * 0.5).astype(F)
    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance.euclidean())
    ix.add(X)
    sq4 = vq_amd.Scalar4Index(X, vq_amd.ScalarQuantizer(*quant))
    Q = rng.standard_normal((7, d)).astype(F)
    D = R.distance_matrix(K.EUCLIDEAN, Q, sq4.packed(), d, *quant)
    short, _ = ix.search(Q, topk=64, nprobe=4)
    assert (short != 0xFFFFFFFF).all()
    _same(ix.search(Q, topk=10, nprobe=4, rerank=sq4, candidates=64), R.rerank(D, short, 10))
    ix.close()


def test_two_runs_are_identical():
    rng = np.random.default_rng(99)
    case = _Case(_codes(1501, 100, rng), (-1.0, 1.0, 16), K.COSINE)
    Q = _queries(129, 100, rng)
    radii = _radii(case.matrix(Q))
    a, b = case.sq4.search(Q, 10), case.sq4.search(Q, 10)
    _same(a, b)
    _same_range(case.sq4.range_search(Q, radii), case.sq4.range_search(Q, radii))
