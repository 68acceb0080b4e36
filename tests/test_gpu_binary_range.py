"""Hamming-radius range search of the binary index on the MI355X (BinaryIndex.hamming_range_search,
vqhip_binary_range_search, k_bin_range in vq_amd/csrc/k_binary.hip) against the numpy statement of include/vqhip.h
(tests/ref_binary_range.py).  Every comparison is exact: lims equal, idx equal, dist equal as uint32 bits.  The three
metrics and the three sources, every d at which the kernels change (one word, the scalar and the 16-byte loader, the
last d of the group of 32 queries and the first of the group of 8), n around the waves, the 512-row steps and the
8192-row blocks with every lane emitting, nq around both group sizes, radii 0 / on a planted tie / d / d + 1 / 2^32 - 1,
empty and dense queries in one group, several batches with the result buffers growing, the batch that shrinks with n,
the cap, determinism, the device form, and consistency with search."""
import os
import re

import numpy as np
import pytest

import ref_binary as B
import ref_binary_range as BR

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_INIT_CAP = 1024  # kRangeInitCap, vq_amd/csrc/range.hpp (tests/test_gpu_range.py checks the value)
U32_MAX = (1 << 32) - 1
LOW_HIGH = [(0, 1), (0, 255), (254, 255), (3, 200)]
THR = 0.25


def _block():
    from vq_amd import _lib

    return _lib.BINARY_RANGE_BLOCK


def _assert_same(got, want):
    gl, gi, gd = got
    wl, wi, wd = want
    assert gl.dtype == np.uint64 and gi.dtype == np.uint32 and gd.dtype == F
    assert gl.shape == wl.shape and np.array_equal(gl, wl), f"lims differ: {gl[:8]} != {wl[:8]}"
    assert gi.shape == wi.shape
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[bad[0]]} != {wi[bad[0]]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _index(source, X, low, high, metric):
    """the index over the bits of X (x >= THR) from one of the three sources"""
    import vq_amd

    bq = vq_amd.BinaryQuantizer(THR, low, high)
    dist = vq_amd.Distance(NAMES[metric])
    bits = B.bits_f32(X, THR)
    if source == "rows":
        return vq_amd.BinaryIndex(X, bq, dist)
    if source == "codes":
        return vq_amd.BinaryIndex.from_codes(np.where(bits, np.uint8(high), np.uint8(low)), bq, dist)
    return vq_amd.BinaryIndex.from_packed(B.pack(bits), X.shape[1], bq, dist)


def _planted(n, d, nq, rng):
    """random rows and queries with, for query 0, exact duplicates (H = 0) at rows 5 and n - 1 and for query 1 a tie:
    three rows at exactly H = t and three at t + 1 (t = d // 2), every other row farther than t + 1 from it"""
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    X[5 % n] = Q[0]
    X[n - 1] = Q[0]
    t = d // 2
    if nq > 1 and n >= 16 and d >= 3:
        far = np.where(Q[1] >= THR, F(-1.0), F(1.0))  # every bit differs: H = d
        X[8:n - 1] = np.where(rng.random((n - 9, d)) < 0.1, Q[1], far)[:]  # H about 0.9 d > t + 1
        for k, row in enumerate((9, 11, 14, 10, 12, 15)):
            h = t if k < 3 else t + 1
            v = Q[1].copy()
            flip = rng.permutation(d)[:h]
            v[flip] = far[flip]
            X[row] = v
    return Q, X


def test_block_constant_is_the_kernels():
    text = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    assert int(re.search(r"#define VQHIP_BINARY_RANGE_BLOCK\s+(\d+)", text).group(1)) == _block() == 8192


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("d", [1, 31, 32, 33, 100, 128, 1024, 1056])
def test_matches_statement_on_every_source(metric, d):
    rng = np.random.default_rng(1000 * metric + d)
    low, high = LOW_HIGH[(d + metric) % 4]
    n, nq = 777, 7
    Q, X = _planted(n, d, nq, rng)
    t = d // 2
    radius = np.array([0, t, t + 1, d, d + 1, U32_MAX, max(t - 1, 0)], np.uint64)
    want = BR.search_rows(Q, X, THR, low, high, metric, radius)
    per = np.diff(want[0].astype(np.int64))
    assert per[0] >= 2 and (per[3:6] == n).all()  # the duplicates; every row for a radius >= d
    if d >= 3:
        h1 = want[1][want[0][1]:want[0][2]].tolist()
        assert {9, 11, 14} <= set(h1) and not {10, 12, 15} & set(h1)  # the tie at H = t is in, H = t + 1 is out
    for source in ("rows", "codes", "packed"):
        _assert_same(_index(source, X, low, high, metric).hamming_range_search(Q, radius), want)


@pytest.fixture(scope="module")
def edge_rows():
    rng = np.random.default_rng(2)
    return rng.standard_normal((2 * 8192 + 1, 40)).astype(F), rng.standard_normal((2, 40)).astype(F)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16385])
def test_wave_step_and_block_edges(n, edge_rows):
    """radius d: every lane position of every step and block emits, in row order; radius 0 at a query planted at row
    n - 1: one hit, in the last block's last row"""
    assert _block() == 8192
    X, Q = edge_rows[0][:n].copy(), edge_rows[1].copy()
    X[n - 1] = Q[1]
    if n > 1:
        X[:n - 1][(B.bits_f32(X[:n - 1], THR) == B.bits_f32(Q[1:2], THR)).all(axis=1)] = -Q[1]  # no other bit match
    radius = [40, 0]
    for metric, source in ((B.MAN, "rows"), (B.EUC, "packed")):
        got = _index(source, X, 0, 1, metric).hamming_range_search(Q, radius)
        assert got[0].tolist() == [0, n, n + 1] and np.array_equal(got[1][:n], np.arange(n, dtype=np.uint32))
        assert got[1][n] == n - 1 and got[2][n] == 0.0
        _assert_same(got, BR.search_rows(Q, X, THR, 0, 1, metric, radius))


@pytest.mark.parametrize("d,group", [(128, 32), (1024, 32), (1056, 8), (100, 32)])
def test_query_counts_around_the_group(d, group):
    rng = np.random.default_rng(d)
    X = rng.standard_normal((600, d)).astype(F)
    ix = _index("rows", X, 0, 255, B.SQ)
    for nq in (1, group - 1, group, group + 1):
        Q = rng.standard_normal((nq, d)).astype(F)
        radius = rng.integers(d // 2 - 6, d // 2 + 2, nq).astype(np.uint32)
        want = BR.search_rows(Q, X, THR, 0, 255, B.SQ, radius)
        assert 0 < want[0][-1] < nq * 600
        _assert_same(ix.hamming_range_search(Q, radius), want)


def test_empty_and_dense_queries_in_one_group():
    """40 queries over three blocks: most have radius 0 and no bit match (empty: the fill skips them, and the workgroups
    of the second query group have nothing at all), some have every row, one has hits in the last block only"""
    rng = np.random.default_rng(9)
    n, d = 2 * 8192 + 300, 64
    X = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((40, d)).astype(F)
    X[n - 7] = Q[5]
    X[n - 2] = Q[5]
    radius = np.zeros(40, np.uint32)
    radius[[2, 17]] = [d, U32_MAX]
    radius[9] = 20
    want = BR.search_rows(Q, X, THR, 0, 1, B.MAN, radius)
    per = np.diff(want[0].astype(np.int64))
    assert per[2] == n and per[17] == n and per[5] == 2 and (per[32:] == 0).all() and (per == 0).sum() >= 35
    ix = _index("packed", X, 0, 1, B.MAN)
    got = ix.hamming_range_search(Q, radius)
    _assert_same(got, want)
    _assert_same(ix.hamming_range_search(Q, radius), got)  # the same call again: identical arrays


@pytest.fixture(scope="module")
def several_batches():
    """1100 queries (batches of 1024) over 3001 x 32, radius 9: a few hits per query -- the statement, computed once"""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3001, 32)).astype(F)
    Q = rng.standard_normal((1100, 32)).astype(F)
    return X, Q, BR.search_rows(Q, X, THR, 0, 1, B.EUC, 9)


def test_several_batches_and_two_growths(several_batches):
    X, Q, want = several_batches
    first, total = int(want[0][1024]), int(want[0][-1])
    # the buffers grow after the first batch (to `first` hits) and again after the second
    assert first > 2 * RANGE_INIT_CAP and total > first
    ix = _index("rows", X, 0, 1, B.EUC)
    got = ix.hamming_range_search(Q, 9)
    _assert_same(got, want)
    _assert_same(ix.hamming_range_search(Q, np.full(1100, 9, np.uint32)), got)


def test_batch_shrinks_with_n():
    """129 blocks of rows: a batch of 1024 queries would have more than 2^17 count entries, so batches are 992 queries;
    1030 all-zero queries over rows of all ones but for planted rows with H = 0 .. 19 around the block and batch edges"""
    import vq_amd

    n, d, nq = 128 * 8192 + 5, 32, 1030
    words = np.full((n, 1), 0xFFFFFFFF, np.uint32)
    rows = [0, 511, 512, 8191, 8192, 8193, 64 * 8192 - 1, 64 * 8192, n - 8193, n - 2, n - 1]
    H = {r: (3 * k) % 20 for k, r in enumerate(rows)}
    for r, h in H.items():
        words[r, 0] = (1 << h) - 1
    radius = (np.arange(nq) % 23).astype(np.uint32)
    radius[991:993] = [4, 31]  # the last query of the first batch, the first of the second
    Q = np.full((nq, d), -1.0, F)  # all bits 0
    ix = vq_amd.BinaryIndex.from_packed(words, d, vq_amd.BinaryQuantizer(0.0), vq_amd.Distance.manhattan())
    lims, idx, dist = ix.hamming_range_search(Q, radius)
    want_i = [[r for r in sorted(H) if H[r] <= int(h)] for h in radius]
    assert np.array_equal(np.diff(lims.astype(np.int64)), [len(w) for w in want_i])
    assert np.array_equal(idx, np.array([r for w in want_i for r in w], np.uint32))
    assert np.array_equal(dist, np.array([H[r] for w in want_i for r in w], F))


@pytest.fixture(scope="module")
def dense_case():
    """40 queries over 5000 x 48 at radius d: 200 000 hits in one batch"""
    rng = np.random.default_rng(4)
    X = rng.standard_normal((5000, 48)).astype(F)
    Q = rng.standard_normal((40, 48)).astype(F)
    return X, Q, BR.search_rows(Q, X, THR, 3, 200, B.EUC, 48)


def test_cap(dense_case):
    import vq_amd
    from vq_amd import _lib

    X, Q, want = dense_case
    assert want[0][-1] == 200_000 > 2 * RANGE_INIT_CAP
    ix = _index("rows", X, 3, 200, B.EUC)
    with pytest.raises(vq_amd.FfiError) as e:
        ix.hamming_range_search(Q, 48, max_results=199_999)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "200000" in str(e.value) and "199999" in str(e.value)
    _assert_same(ix.hamming_range_search(Q, 48, max_results=200_000), want)
    with pytest.raises(vq_amd.FfiError) as e:
        ix.hamming_range_search(Q, 48, max_results=1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    gi, gd = ix.search(Q, 10)  # the index is usable afterwards
    wi, wd = B.search_rows(Q, X, THR, 3, 200, B.EUC, 10)
    assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _read_device(ptr, count, dtype):
    import torch

    from vq_amd import _lib

    t = torch.zeros(max(count, 1) * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if count:
        _lib.memcpy_device(t.data_ptr(), ptr, count * np.dtype(dtype).itemsize)
    _lib.synchronize()
    return t.cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype)


def test_device_form_at_an_offset_pointer():
    """queries at a device pointer offset by 4 bytes from an allocation; the RangeResult's device arrays are what read()
    returns"""
    import torch

    import vq_amd

    rng = np.random.default_rng(12)
    d, nq = 37, 9
    Q, X = _planted(2001, d, nq, rng)
    radius = np.array([0, 18, 19, d, 5, 12, 15, U32_MAX, 17], np.uint32)
    ix = _index("codes", X, 254, 255, B.SQ)
    want = BR.search_rows(Q, X, THR, 254, 255, B.SQ, radius)
    qb = torch.zeros(nq * d + 9, dtype=torch.float32, device="cuda:0")
    qb[1:1 + nq * d] = torch.from_numpy(Q.ravel()).to("cuda:0")
    torch.cuda.synchronize()
    res = ix.hamming_range_search_device(qb.data_ptr() + 4, nq, radius)
    assert isinstance(res, vq_amd.RangeResult) and res.nq == nq and res.total == int(want[0][-1])
    assert np.array_equal(res.lims, want[0])
    _assert_same(res.read(), want)
    pl, pi, pd = res.device_pointers()
    got = (_read_device(pl, nq + 1, np.uint64), _read_device(pi, res.total, np.uint32), _read_device(pd, res.total, F))
    _assert_same(got, want)
    empty = ix.hamming_range_search_device(qb.data_ptr() + 4, 0, np.empty(0, np.uint32))
    assert empty.total == 0 and empty.lims.tolist() == [0]
    assert all(a.size == b for a, b in zip(empty.read(), (1, 0, 0)))
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.hamming_range_search_device(qb.data_ptr() + 2, nq, radius)


@pytest.mark.parametrize("metric", B.METRICS)
def test_consistent_with_search(metric):
    """radius = the H of the 10th row search reports: sorted by (H, row), the range result starts with search's ten"""
    rng = np.random.default_rng(30 + metric)
    d = 96
    X = rng.standard_normal((5003, d)).astype(F)
    X[40:45] = X[41]
    Q = rng.standard_normal((6, d)).astype(F)
    Q[2] = X[41]
    ix = _index("rows", X, 0, 255, metric)
    si, sd = ix.search(Q, 10)
    H = B.hamming(B.pack(B.bits_f32(Q, THR)), B.pack(B.bits_f32(X, THR)))
    D = B.reported(d, 0, 255, metric)
    h10 = np.array([H[j, si[j, 9]] for j in range(6)], np.uint32)
    lims, idx, dist = ix.hamming_range_search(Q, h10)
    for j in range(6):
        a, b = int(lims[j]), int(lims[j + 1])
        assert b - a >= 10
        Hj = H[j, idx[a:b]]
        assert np.array_equal(dist[a:b].view(np.uint32), D[Hj].view(np.uint32))
        order = np.lexsort((idx[a:b], Hj))
        assert np.array_equal(idx[a:b][order][:10], si[j])
        assert np.array_equal(dist[a:b][order][:10].view(np.uint32), sd[j].view(np.uint32))
