"""One handle through a sequence of calls, on every resident index (FlatIndex f32 / f16, ScalarIndex from rows / from
codes, BinaryIndex from rows / from packed words) -- the steps of the host layer the three share (vq_amd/csrc/api_resident.hip,
"resident indexes: the shared host layer").  The workspaces q / idx / out belong to the handle and are used by search,
rerank and range search alike, so each step is compared with the numpy statements (tests/ref_knn.py, ref_sqindex.py,
ref_binary.py, ref_range.py): a workspace left at an earlier call's size, or holding an earlier call's data, shows as a
wrong result.  Every comparison is exact: indices equal, distances equal as uint32 bits.

n 300 and d 40: the rows do not fill the 64-lane waves and the packed rows have a pad (40 % 32 != 0); rows 297..299
duplicate rows 20..22 and query 0 equals row 21, so ties are settled by row id."""
import functools

import numpy as np
import pytest

import ref_binary as B
import ref_knn as K
import ref_range as R
import ref_sqbq as S
import ref_sqindex as SI

pytestmark = pytest.mark.gpu

F = np.float32
N, D, NQ = 300, 40, 17
SQ = SI.QUANTIZERS[2]  # (-3, 5, 17)
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
EXACT = ["flat_f32", "flat_f16", "sq_rows", "sq_codes"]
BINARY = ["bin_rows", "bin_packed"]


@functools.lru_cache(maxsize=None)
def _rows():
    rng = np.random.default_rng(300)
    X = (rng.standard_normal((N, D)) * 1.5).astype(F)
    X[N - 3:] = X[20:23]
    return X


@functools.lru_cache(maxsize=None)
def _stored(kind):
    """the rows as the index of `kind` holds them, f32: what the statement computes distances against"""
    if kind == "flat_f32":
        return _rows()
    if kind == "flat_f16":
        return _rows().astype(np.float16).astype(F)
    return SI.decode(SQ, S.sq_encode(*SQ, _rows()))  # both scalar sources: the same codes


@functools.lru_cache(maxsize=None)
def _queries(kind):
    Q = np.random.default_rng(17).standard_normal((NQ, D)).astype(F)
    Q[0] = _stored(kind)[21] if kind in EXACT else _rows()[21]
    return Q


@functools.lru_cache(maxsize=None)
def _full(kind, metric):
    """every query's complete order, [NQ][N]: the first topk columns are the statement's result for any topk"""
    if kind in BINARY:
        return B.search_rows(_queries(kind), _rows(), 0.0, 0, 1, metric, N)
    return K.search(metric, _queries(kind), _stored(kind), N)


def _index(kind, metric):
    import vq_amd

    dist = vq_amd.Distance(NAMES[metric])
    if kind == "flat_f32":
        return vq_amd.FlatIndex(_rows(), dist)
    if kind == "flat_f16":
        return vq_amd.FlatIndex(_rows().astype(np.float16), dist)
    if kind == "sq_rows":
        return vq_amd.ScalarIndex(_rows(), vq_amd.ScalarQuantizer(*SQ), dist)
    if kind == "sq_codes":
        return vq_amd.ScalarIndex.from_codes(S.sq_encode(*SQ, _rows()), vq_amd.ScalarQuantizer(*SQ), dist)
    if kind == "bin_rows":
        return vq_amd.BinaryIndex(_rows(), distance=dist)
    return vq_amd.BinaryIndex.from_packed(B.pack(B.bits_f32(_rows(), 0.0)), D, distance=dist)


def _assert_same(got, want):
    (gi, gd), (wi, wd) = got, want
    assert gi.dtype == np.uint32 and gd.dtype == F
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), np.ascontiguousarray(wd).view(np.uint32))


def _cut(full, rows, topk):
    return full[0][rows, :topk], full[1][rows, :topk]


def _search_steps(ix, kind, metric):
    import torch

    import vq_amd

    Q, full = _queries(kind), _full(kind, metric)
    assert ix._ix is None
    first = ix.search(Q[:3], 4)
    _assert_same(first, _cut(full, slice(0, 3), 4))
    handle = ix._ix
    _assert_same(ix.search(Q, N), full)  # topk = n, and q / idx / out grow past the first call's sizes
    _assert_same(ix.search(Q[5], 1), _cut(full, slice(5, 6), 1))
    idx, dist = ix.search(np.empty((0, D), F), 4)
    assert idx.shape == (0, 4) and idx.dtype == np.uint32 and dist.shape == (0, 4) and dist.dtype == F
    dev = torch.device("cuda:0")
    qb = torch.from_numpy(Q[:3].copy()).to(dev)
    ib = torch.full((3, 4), 7, dtype=torch.int32, device=dev)
    db = torch.full((3, 4), -1.0, dtype=torch.float32, device=dev)
    ix.search_device(qb.data_ptr(), 3, 4, ib.data_ptr(), db.data_ptr())
    vq_amd._lib.synchronize()
    torch.cuda.synchronize()
    got = (ib.cpu().numpy().view(np.uint32), db.cpu().numpy())
    _assert_same(got, first)
    assert ix._ix is handle  # one handle all along


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
@pytest.mark.parametrize("kind", EXACT)
def test_exact_index_one_handle_through_every_call(kind, metric):
    ix = _index(kind, metric)
    Q, X, full = _queries(kind), _stored(kind), _full(kind, metric)
    _search_steps(ix, kind, metric)
    handle = ix._ix
    # rerank: 9 distinct candidates per query; query 0's hold both copies of the row it equals
    rng = np.random.default_rng(9)
    cand = np.stack([rng.choice(N, 9, replace=False) for _ in range(3)]).astype(np.uint32)
    cand[0, :2] = (N - 2, 21)
    cand[0, 2:] = np.setdiff1d(np.arange(N), cand[0, :2])[rng.choice(N - 2, 7, replace=False)]
    _assert_same(ix.rerank(Q[:3], cand, 4), K.rerank(metric, Q[:3], X, cand, 4))
    # range search: one radius between the nearest rows of the queries, so that some hit and some do not
    nearest = np.sort(full[1][:, 0])
    radius = F(nearest[NQ // 2])
    want = R.search(metric, Q, X, radius)
    per_query = np.diff(want[0].astype(np.int64))
    assert (per_query == 0).any() and (per_query > 0).any()
    lims, idx, dist = ix.range_search(Q, radius)
    assert np.array_equal(lims, want[0]) and lims.dtype == np.uint64
    _assert_same((idx, dist), want[1:])
    # search again, over the q / idx / out the two calls above have used
    _assert_same(ix.search(Q[:3], 4), _cut(full, slice(0, 3), 4))
    _assert_same(ix.search(Q, N), full)
    assert ix._ix is handle


@pytest.mark.parametrize("kind", BINARY)
def test_binary_index_one_handle_through_every_call(kind):
    _search_steps(_index(kind, B.MAN), kind, B.MAN)


def test_flat_search_device_refuses_a_query_pointer_that_is_not_4_byte_aligned():
    """as the five other device-form entry points do (tests/test_gpu_range.py has the range case): refused before
    anything is launched, so the result buffers keep their fill"""
    import torch

    import vq_amd

    ix = _index("flat_f32", K.EUCLIDEAN)
    dev = torch.device("cuda:0")
    qb = torch.zeros(3 * D + 8, dtype=torch.float32, device=dev)
    ib = torch.full((3, 4), 7, dtype=torch.int32, device=dev)
    db = torch.full((3, 4), -1.0, dtype=torch.float32, device=dev)
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.search_device(qb.data_ptr() + 2, 3, 4, ib.data_ptr(), db.data_ptr())
    vq_amd._lib.synchronize()
    torch.cuda.synchronize()
    assert (ib.cpu().numpy() == 7).all() and (db.cpu().numpy() == -1.0).all()
    ix.search_device(qb.data_ptr() + 4, 3, 4, ib.data_ptr(), db.data_ptr())  # the handle works on
    vq_amd._lib.synchronize()
    torch.cuda.synchronize()
    _assert_same((ib.cpu().numpy().view(np.uint32), db.cpu().numpy()), K.search(K.EUCLIDEAN, np.zeros((3, D), F), _rows(), 4))
