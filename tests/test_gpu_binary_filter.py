"""Filtered search of vq_amd.BinaryIndex on the MI355X (``filtered_search``, ``filtered_hamming_range_search`` and their
device forms; vqhip_binary_*_masked; k_bin_scan_masked, k_bin_pick_masked, k_bin_ties_masked and the masked k_bin_range in
vq_amd/csrc/k_binary.hip) against the numpy statement tests/ref_binary_filter.py: indices, lims, and distances as uint32
bits.  No tolerances."""
import numpy as np
import pytest

import ref_binary as B
import ref_binary_filter as S
import ref_binary_range as BR

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan"]
N = 1037  # three masked slices
BQ = (0.25, 3, 200)  # threshold, low, high


def _index(X, metric, bq=BQ):
    import vq_amd

    return vq_amd.BinaryIndex(X, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]))


def _same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


def _same_range(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: lims {got[0]} != {want[0]}"
    assert np.array_equal(got[1], want[1]), what
    assert got[2].dtype == F and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), what


def _data(n, d, rng, nq=5):
    """rows with exact duplicates of rows 20..22 at 200..202 and at the end; query 0 equals row 21"""
    X = rng.standard_normal((n, d)).astype(F)
    if n > 210:
        X[200:203] = X[20:23]
        X[n - 3:] = X[20:23]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = X[21 % n]
    return Q, X


def _masks(n, rng):
    """the nine masks of DESIGN.md section 24 over n rows: name -> (bool mask, the argument handed to the index)"""
    def rand(p):
        m = rng.random(n) < p
        m[20], m[21], m[22] = True, False, True  # duplicates on both sides of the mask; query 0 equals the disallowed row 21
        m[200], m[201], m[202] = False, True, False
        m[n - 3], m[n - 2], m[n - 1] = False, True, True
        return m

    def block(a, b):
        m = np.zeros(n, bool)
        m[a:b] = True
        return m

    one = lambda i: np.arange(n) == i
    half = rand(0.5)
    tail = S.pack(half).copy()
    tail[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # every bit past n in the last word set
    out = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "row0": one(0), "last": one(n - 1), "half": rand(0.5),
           "3pc": rand(0.03), "groups": block(128, 320), "edges": block(100, 333)}
    out = {k: (m, m) for k, m in out.items()}
    out["half+tail"] = (half, tail)
    return out


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("d", [1, 31, 32, 33, 100, 128, 1056, 1152])
def test_search_and_range_match_statement(metric, d):
    """W = 1, 1, 1, 2, 4, 4, 33, 36: both V4 forms at QG = 32 and both at QG = 8"""
    rng = np.random.default_rng(1000 * metric + d)
    Q, X = _data(N, d, rng)
    ix = _index(X, metric)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    radius = np.array([0, d // 2, d // 3, d + 7, d // 2 + 1], np.uint32)
    plain, plain_r = ix.search(Q, 10), ix.hamming_range_search(Q, radius)
    for name, (m, arg) in _masks(N, rng).items():
        got = ix.filtered_search(Q, arg, 10)
        _same(got, S.search(qw, words, d, BQ[1], BQ[2], metric, 10, m), name)
        assert not np.isin(got[0], np.flatnonzero(~m)).any(), name
        got_r = ix.filtered_hamming_range_search(Q, radius, arg)
        _same_range(got_r, S.range_search(qw, words, d, BQ[1], BQ[2], metric, radius, m), name)
        if name == "ones":
            _same(got, plain, "all ones against the unmasked search")
            _same_range(got_r, plain_r, "all ones against the unmasked range search")
        if name == "zeros":
            assert (got[0] == 0xFFFFFFFF).all() and np.isposinf(got[1]).all()
            assert not got_r[0].any() and got_r[1].size == 0
    _same(ix.search(Q, 10), plain, "the unmasked search after masked ones")
    _same_range(ix.hamming_range_search(Q, radius), plain_r, "the unmasked range search after masked ones")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, 511, 512, 513])
def test_small_n(n):
    """the last mask word missing, a wave's second word missing, the step and lane edges"""
    rng = np.random.default_rng(n)
    d = 70
    Q, X = _data(n, d, rng, 3)
    ix = _index(X, B.MAN)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    masks = {"ones": np.ones(n, bool), "half": rng.random(n) < 0.5, "last": np.arange(n) == n - 1, "first": np.arange(n) == 0}
    for name, m in masks.items():
        for topk in {1, min(n, 5)}:
            _same(ix.filtered_search(Q, S.pack(m), topk), S.search(qw, words, d, BQ[1], BQ[2], B.MAN, topk, m), f"{name} topk {topk}")
        _same_range(ix.filtered_hamming_range_search(Q, d // 2, m), S.range_search(qw, words, d, BQ[1], BQ[2], B.MAN, d // 2, m), name)


@pytest.mark.parametrize("d", [1, 300])
@pytest.mark.parametrize("allowed,topk", [(7, 10), (600, 1024), (0, 10), (1, 10), (0, 1024), (1, 1)])
def test_fewer_allowed_rows_than_topk(d, allowed, topk):
    """the under-full pick: total < topk.  d = 1: 2 bins, the last k_bin_pick thread has an empty bin range; d = 300: 301
    bins, two a thread, the last thread's range is not empty"""
    rng = np.random.default_rng(d + allowed)
    Q, X = _data(N, d, rng, 4)
    ix = _index(X, B.EUC)
    m = np.zeros(N, bool)
    m[rng.choice(N, allowed, replace=False)] = True
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    got = ix.filtered_search(Q, m, topk)
    _same(got, S.search(qw, words, d, BQ[1], BQ[2], B.EUC, topk, m))
    assert ((got[0] != 0xFFFFFFFF).sum(axis=1) == min(allowed, topk)).all()


def _heavy(rng, n=20000):
    """d = 4: 95 % of the rows are one pattern, so the cut of a query near it holds far more than 8192 rows"""
    bits = np.tile(np.array([1, 0, 1, 1], bool), (n, 1))
    other = rng.random(n) < 0.05
    bits[other] = rng.random((int(other.sum()), 4)) < 0.5
    X = np.where(bits, F(1.0), F(-1.0))
    Q = np.array([[1, -1, 1, 1], [1, 1, 1, 1], [-1, 1, -1, -1], [1, -1, -1, 1]], F)
    return Q, X, other


@pytest.mark.parametrize("allowed", [15000, 9000, 4000])
@pytest.mark.parametrize("topk", [10, 1024])
def test_heavy_cut(allowed, topk):
    """k_bin_ties_masked: the lowest allowed row ids among the ties at H*; 4000 allowed rows stay under the heavy bound,
    which is decided on allowed counts"""
    rng = np.random.default_rng(allowed + topk)
    Q, X, _ = _heavy(rng)
    n = X.shape[0]
    ix = _index(X, B.SQ, (0.0, 0, 1))
    m = np.zeros(n, bool)
    m[rng.choice(n, allowed, replace=False)] = True
    m[:40] = False  # the lowest ids among the ties are disallowed
    qw, words = B.pack(B.bits_f32(Q, 0.0)), B.pack(B.bits_f32(X, 0.0))
    _same(ix.filtered_search(Q, m, topk), S.search(qw, words, 4, 0, 1, B.SQ, topk, m))


@pytest.mark.parametrize("topk", [10, 1024])
def test_heavy_cut_with_five_allowed_ties(topk):
    """19 000 rows at H* without the mask, 5 of them allowed: not heavy under the mask"""
    rng = np.random.default_rng(topk)
    Q, X, other = _heavy(rng)
    n = X.shape[0]
    ix = _index(X, B.SQ, (0.0, 0, 1))
    m = other.copy()
    m[np.flatnonzero(~other)[[3, 700, 8000, 12345, -1]]] = True
    qw, words = B.pack(B.bits_f32(Q, 0.0)), B.pack(B.bits_f32(X, 0.0))
    _same(ix.filtered_search(Q, m, topk), S.search(qw, words, 4, 0, 1, B.SQ, topk, m))


def test_stale_state_on_one_handle():
    """hist, cnt, cand and range_ws are reused: nothing of the other call may show"""
    rng = np.random.default_rng(77)
    d = 96
    Q, X = _data(3000, d, rng, 40)
    ix = _index(X, B.MAN)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    m = rng.random(3000) < 0.02
    ones = np.ones(3000, bool)
    want_u, want_m = S.search(qw, words, d, BQ[1], BQ[2], B.MAN, 100, ones), S.search(qw, words, d, BQ[1], BQ[2], B.MAN, 100, m)
    r = d // 2 - 4
    want_ru, want_rm = BR.search(qw, words, d, BQ[1], BQ[2], B.MAN, r), S.range_search(qw, words, d, BQ[1], BQ[2], B.MAN, r, m)
    _same(ix.search(Q, 100), want_u, "unmasked first")
    _same(ix.filtered_search(Q, m, 100), want_m, "masked after unmasked")
    _same(ix.search(Q, 100), want_u, "unmasked after masked")
    _same(ix.filtered_search(Q[:3], m, 100), (want_m[0][:3], want_m[1][:3]), "fewer queries after more")
    _same_range(ix.hamming_range_search(Q, r), want_ru, "range unmasked first")
    _same_range(ix.filtered_hamming_range_search(Q, r, m), want_rm, "range masked after unmasked")
    _same_range(ix.hamming_range_search(Q, r), want_ru, "range unmasked after masked")
    _same(ix.filtered_search(Q, m, 100), want_m, "search after range")


@pytest.mark.parametrize("metric", [B.EUC, B.MAN])
def test_range_search_over_two_blocks(metric):
    """n = 8192 + 513: two blocks, the second partly filled; radii 0, mid and >= d; a mask that empties the first block"""
    rng = np.random.default_rng(metric)
    n, d = 8192 + 513, 48
    Q, X = _data(n, d, rng, 6)
    X[8192 + 100] = X[21]  # an exact match of query 0 in the second block
    ix = _index(X, metric)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    second = np.arange(n) >= 8192
    masks = {"second block only": second, "half": rng.random(n) < 0.5, "second block, sparse": second & (rng.random(n) < 0.1),
             "one wave of the first block": (np.arange(n) >= 4096 + 64) & (np.arange(n) < 4096 + 128)}
    for name, m in masks.items():
        for radius in (0, d // 2 - 3, np.array([0, d // 2, d, d + 5, 3, 1 << 31], np.uint32)):
            _same_range(ix.filtered_hamming_range_search(Q, radius, m), S.range_search(qw, words, d, BQ[1], BQ[2], metric, radius, m),
                        f"{name}, radius {radius}")


def test_batches():
    """1100 queries over 20 000 rows under a 3 % mask: two search batches, and the range result grows"""
    rng = np.random.default_rng(11)
    n, d, nq = 20000, 64, 1100
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    ix = _index(X, B.SQ)
    m = rng.random(n) < 0.03
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    _same(ix.filtered_search(Q, m, 10), S.search(qw, words, d, BQ[1], BQ[2], B.SQ, 10, m))
    got = ix.filtered_hamming_range_search(Q, 30, m)
    _same_range(got, S.range_search(qw, words, d, BQ[1], BQ[2], B.SQ, 30, m))
    assert got[1].size > 100000


@pytest.mark.parametrize("off", [1, 3])
def test_device_forms_at_offset_pointers(off):
    """the mask `off` words behind a 16-byte aligned allocation: only 4-byte aligned, two u32 reads a wave"""
    import torch

    rng = np.random.default_rng(off)
    d, nq, topk, n = 128, 9, 17, 2001
    Q, X = _data(n, d, rng, nq)
    m = rng.random(n) < 0.3
    m[64:256] = False
    w = S.pack(m)
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mb = torch.full((w.size + off + 8,), -1, dtype=torch.int32, device=dev)  # all ones around the mask
    assert mb.data_ptr() % 16 == 0
    mb[off:off + w.size] = torch.from_numpy(w.view(np.int32)).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    ix = _index(X, B.EUC)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    ix.filtered_search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off,
                              mb.data_ptr() + 4 * off)
    torch.cuda.synchronize()
    gi, gd = ib.cpu().numpy(), db.cpu().numpy()
    _same((gi[off:off + nq * topk].view(np.uint32).reshape(nq, topk), gd[off:off + nq * topk].reshape(nq, topk)),
          S.search(qw, words, d, BQ[1], BQ[2], B.EUC, topk, m))
    assert (gi[:off] == 7).all() and (gi[off + nq * topk:] == 7).all()
    assert (gd[:off] == -1.0).all() and (gd[off + nq * topk:] == -1.0).all()
    res = ix.filtered_hamming_range_search_device(qb.data_ptr() + 4 * off, nq, d // 2 - 5, mb.data_ptr() + 4 * off)
    _same_range(res.read(), S.range_search(qw, words, d, BQ[1], BQ[2], B.EUC, d // 2 - 5, m))
    assert (mb.cpu().numpy()[off:off + w.size].view(np.uint32) == w).all()


def test_range_and_topk_agree():
    """with h_q the H of the topk-th result of the filtered search, the first topk of the filtered range slice sorted by
    (H, row) is the filtered search's result"""
    rng = np.random.default_rng(3)
    n, d, topk = 3000, 100, 20
    Q, X = _data(n, d, rng, 6)
    ix = _index(X, B.MAN, (0.0, 0, 1))  # D = H
    m = rng.random(n) < 0.2
    idx, dist = ix.filtered_search(Q, m, topk)
    lims, ridx, rdist = ix.filtered_hamming_range_search(Q, dist[:, -1].astype(np.uint32), m)
    for j in range(Q.shape[0]):
        sl = slice(int(lims[j]), int(lims[j + 1]))
        order = np.lexsort((ridx[sl], rdist[sl]))[:topk]
        assert np.array_equal(ridx[sl][order], idx[j]) and np.array_equal(rdist[sl][order], dist[j])


def test_rerank_sees_allowed_rows_only():
    """fewer allowed rows than candidates: the first stage is padded, the reranker gets the real hits"""
    import vq_amd

    rng = np.random.default_rng(9)
    n, d = 1500, 40
    Q, X = _data(n, d, rng, 5)
    ix = _index(X, B.MAN, (0.0, 0, 1))
    flat = vq_amd.FlatIndex(X)
    for allowed in (6, 25, 400):
        m = np.zeros(n, bool)
        m[rng.choice(n, allowed, replace=False)] = True
        idx, dist = ix.filtered_search(Q, m, 10, rerank=flat, candidates=40)
        first, _ = ix.filtered_search(Q, m, 40)
        for j in range(Q.shape[0]):
            cand = first[j][first[j] != 0xFFFFFFFF]
            k = min(10, cand.size)
            wi, wd = flat.rerank(Q[j:j + 1], cand[None, :], k)
            assert np.array_equal(idx[j, :k], wi[0]) and np.array_equal(dist[j, :k].view(np.uint32), wd[0].view(np.uint32))
            assert (idx[j, k:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, k:]).all()
            assert m[idx[j, :k]].all()


@pytest.mark.parametrize("seed", range(40))
def test_seeded_draws(seed):
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 3001))
    d = int(rng.integers(1, 1201))
    metric = int(rng.integers(0, 3))
    p = float(rng.choice([0.0, 0.001, 0.01, 0.1, 0.5, 0.9, 1.0]))
    topk = int(rng.integers(1, min(n, 1024) + 1))
    nq = int(rng.integers(1, 40))
    radius = rng.integers(0, d + 2, nq).astype(np.uint32)
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    m = rng.random(n) < p
    ix = _index(X, metric)
    qw, words = B.pack(B.bits_f32(Q, BQ[0])), B.pack(B.bits_f32(X, BQ[0]))
    what = f"n {n} d {d} metric {metric} p {p} topk {topk} nq {nq}"
    _same(ix.filtered_search(Q, m, topk), S.search(qw, words, d, BQ[1], BQ[2], metric, topk, m), what)
    _same_range(ix.filtered_hamming_range_search(Q, radius, m), S.range_search(qw, words, d, BQ[1], BQ[2], metric, radius, m), what)
