"""Filtered inverted-file PQ search on the MI355X (``IVFPQIndex.masked_search[_device]``, vqhip_ivfpq_search_masked[_device]:
the view kernels of vq_amd/csrc/ivf_view.hpp and the picked scans k_ivf_scan<true> / k_ivf_rscan<true> of k_ivf.hip) against
the numpy statement of include/vqhip.h (tests/ref_pq_filter.py): indices equal, distances equal as uint32 bits, no
tolerance anywhere.  Plain and residual lists, three metrics, one- and two-byte codes, m % 8 != 0 and the table limit, an
empty / a one-row / a large list, eleven masks, ties on both sides of the mask, NaN / inf queries, the scan's block passes
and a chunk edge, the dense select, short results, nprobe == nlist against the filtered PQIndex, the edges of the view, a
view that follows the handle's rows, two batches, the device form at offset pointers, rerank with short queries, two
threads on one handle, seeded draws."""
import threading

import numpy as np
import pytest

import ref_filter as RF
import ref_ivf as R
import ref_ivf_residual as RR
import ref_knn as K
import ref_pq_filter as RPF

pytestmark = pytest.mark.gpu

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)
NAMES = ["squared_euclidean", "euclidean", "manhattan"]
KINDS = [False, True]  # residual
N, NLIST = 3001, 7
BIG, ONE, EMPTY = 0, 5, 2  # the list with more than 600 rows, the list of one row, the list of none
PAD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def orc():
    import oracle as O

    return O.get()


def _same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"{what}: first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


def _index(coarse, cb, metric, lists, codes, residual):
    import vq_amd

    ix = vq_amd.IVFPQIndex(coarse, cb, vq_amd.Distance(NAMES[metric]), residual=residual)
    ix.add_codes(lists, codes)
    return ix


def _unmasked(orc, residual, *args):
    return (RR.search if residual else R.search)(orc, *args)


def _code_dtype(k):
    return np.uint8 if k <= 256 else np.uint16


def _base(rng, m, k, sd, n=N, nq=8):
    """n = 3001 rows in 7 lists: list 2 empty, list 5 one row, list 0 more than 600; exact duplicates of rows 20..22 at
    200..202 and at the end, in their lists; queries beside the centroids of the big, the empty and the one-row list"""
    d = m * sd
    coarse = (rng.standard_normal((NLIST, d)) * 2).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.choice(np.array([0, 0, 1, 3, 4, 6], np.uint32), n)
    lists[500] = ONE
    codes = rng.integers(0, k, (n, m)).astype(_code_dtype(k))
    for at in (200, n - 3):
        codes[at:at + 3] = codes[20:23]
        lists[at:at + 3] = lists[20:23]
    assert (lists == EMPTY).sum() == 0 and (lists == ONE).sum() == 1 and (lists == BIG).sum() > n // 5
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = coarse[BIG] + F(0.05) * rng.standard_normal(d).astype(F)
    Q[1] = coarse[EMPTY]
    Q[2] = coarse[ONE]
    Q[3] = 0.0
    return coarse, cb, lists, codes, Q


def _masks(lists, rng):
    """the masks of test_gpu_ivf_filter.py: name -> (bool mask, what is handed to the index)"""
    n = len(lists)

    def rand(p):
        m = rng.random(n) < p
        m[20], m[21], m[22] = True, False, True  # the duplicates on both sides of the mask
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


SHAPES = [(8, 256, 4),   # one-byte codes in 8-byte words
          (4, 300, 3),   # two-byte codes
          (3, 16, 5)]    # m % 8 != 0


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_matches_statement(orc, shape, metric, residual):
    m, k, sd = shape
    rng = np.random.default_rng(1000 * metric + m)
    coarse, cb, lists, codes, Q = _base(rng, m, k, sd)
    ix = _index(coarse, cb, metric, lists, codes, residual)
    masks = _masks(lists, rng)
    for nprobe in (1, 3, 7):
        plain = ix.search(Q, 10, nprobe)
        for name, (mk, arg) in masks.items():
            what = f"{name}, nprobe {nprobe}"
            # one statement per (mask, nprobe) at topk 1024: a smaller topk is its prefix (one total order, padding last)
            want = RPF.ivf_search(orc, residual, metric, coarse, cb, lists, codes, Q, nprobe, 1024, mk)
            for topk in ((1, 10, 256, 1024) if name in ("half", "3pc", "one list", "half+tail") else (10,)):
                got = ix.masked_search(Q, arg, topk, nprobe)
                _same(got, (want[0][:, :topk], want[1][:, :topk]), f"{what}, topk {topk}")
                assert not np.isin(got[0], np.flatnonzero(~mk)).any(), what
                if name == "ones" and topk == 10:
                    _same(got, plain, "all ones against the unmasked call")
                if name == "zeros":
                    assert (got[0] == PAD).all() and np.isposinf(got[1]).all()
        _same(ix.search(Q, 10, nprobe), plain, "the unmasked call after masked ones")
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("metric", METRICS)
def test_ties_and_nonfinite_queries(orc, metric, residual):
    """blocks of equal codes on both sides of the mask (ties go to the lower allowed row id), NaN / +inf / -inf queries"""
    rng = np.random.default_rng(40 + metric)
    m, k, sd = 8, 64, 2
    coarse, cb, lists, codes, Q = _base(rng, m, k, sd)
    codes[100:900] = codes[5]
    Q[4, 3] = np.nan
    Q[5, 0] = np.inf
    Q[6, -1] = -np.inf
    mask = rng.random(N) < 0.5
    mask[100:130] = False
    mask[130:140] = True
    ix = _index(coarse, cb, metric, lists, codes, residual)
    for nprobe in (1, 3, 7):
        for topk in (10, 256):
            _same(ix.masked_search(Q, mask, topk, nprobe),
                  RPF.ivf_search(orc, residual, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask), f"nprobe {nprobe} topk {topk}")
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_scan_block_passes_and_chunk_edge(orc, count, residual):
    """a list with exactly `count` allowed rows of about 700: the scan's passes of 256 positions, and a chunk edge at 512"""
    rng = np.random.default_rng(count)
    m, k, sd = 8, 256, 2
    coarse, cb, lists, codes, Q = _base(rng, m, k, sd)
    big = np.flatnonzero(lists == BIG)
    assert big.size > count
    mask = rng.random(N) < 0.2
    mask[big] = False
    mask[rng.permutation(big)[:count]] = True
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes, residual)
    for nprobe in (1, 3):
        want = RPF.ivf_search(orc, residual, K.SQUARED_EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, 600, mask)
        got = ix.masked_search(Q, mask, 600, nprobe)
        _same(got, want, f"nprobe {nprobe}")
        if nprobe == 1:
            assert (got[0][0] != PAD).sum() == count  # the query beside the big list's centroid sees exactly its allowed rows
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("metric", [K.SQUARED_EUCLIDEAN, K.EUCLIDEAN])
def test_dense_select_over_tied_allowed_rows(orc, metric, residual):
    """n = 20000 in 2 lists; 12000 rows of list 0 share one code row and 9000 of them are allowed: more than 8192 ties at the
    cut, so the selection goes through the exact radix select over (key, row id) of the allowed positions"""
    rng = np.random.default_rng(7 + metric)
    n, m, k, sd = 20000, 8, 32, 2
    coarse = (rng.standard_normal((2, m * sd)) * 2).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = np.ones(n, np.uint32)
    tied = rng.permutation(n)[:12000]
    lists[tied] = 0
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    codes[tied] = codes[tied[0]]
    mask = rng.random(n) < 0.5
    mask[tied] = False
    mask[tied[:9000]] = True
    Q = rng.standard_normal((3, m * sd)).astype(F)
    Q[0] = coarse[0]
    Q[1] = coarse[1]
    ix = _index(coarse, cb, metric, lists, codes, residual)
    for nprobe in (1, 2):
        for topk in (10, 300):
            got = ix.masked_search(Q, mask, topk, nprobe)
            _same(got, RPF.ivf_search(orc, residual, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask), f"nprobe {nprobe} topk {topk}")
    assert np.array_equal(ix.masked_search(Q[:1], mask, 300, 1)[0][0], np.sort(tied[:9000])[:300])  # the lowest allowed ids of the tie
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_fewer_allowed_rows_than_topk(orc, residual):
    rng = np.random.default_rng(5)
    coarse, cb, lists, codes, Q = _base(rng, 8, 256, 2)
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:7]] = True
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes, residual)
    got = ix.masked_search(Q, mask, 10, NLIST)
    _same(got, RPF.ivf_search(orc, residual, K.EUCLIDEAN, coarse, cb, lists, codes, Q, NLIST, 10, mask))
    assert ((got[0] != PAD).sum(axis=1) == 7).all() and (got[0][:, 7:] == PAD).all() and np.isposinf(got[1][:, 7:]).all()
    _same(ix.masked_search(Q, mask, 10, 2), RPF.ivf_search(orc, residual, K.EUCLIDEAN, coarse, cb, lists, codes, Q, 2, 10, mask))
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_topk_1024_with_600_allowed(orc, residual):
    rng = np.random.default_rng(6)
    coarse, cb, lists, codes, Q = _base(rng, 8, 256, 2)
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:600]] = True
    ix = _index(coarse, cb, K.MANHATTAN, lists, codes, residual)
    got = ix.masked_search(Q, mask, 1024, NLIST)
    _same(got, RPF.ivf_search(orc, residual, K.MANHATTAN, coarse, cb, lists, codes, Q, NLIST, 1024, mask))
    assert ((got[0] != PAD).sum(axis=1) == 600).all()
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_table_limit(orc, residual):
    """m * k = 38400: the largest table the scans hold"""
    rng = np.random.default_rng(8)
    n, m, k, sd = 1500, 150, 256, 1
    coarse, cb, lists, codes, Q = _base(rng, m, k, sd, n=n, nq=4)
    mask = rng.random(n) < 0.4
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes, residual)
    for nprobe in (1, 4):
        _same(ix.masked_search(Q, mask, 20, nprobe),
              RPF.ivf_search(orc, residual, K.SQUARED_EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, 20, mask), f"nprobe {nprobe}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [20000, 40000])
def test_all_lists_equal_the_filtered_pqindex(orc, n, metric):
    """nprobe == nlist, non-residual: the filtered PQIndex over the same codes -- indices and distance bits -- and the dense
    statement.  At n = 40000 and topk 10 the unfiltered PQIndex takes the one-scan schedule, the filtered one the full pass."""
    from vq_amd.store import PQIndex

    import vq_amd

    rng = np.random.default_rng(n + metric)
    m, k, sd, nlist = 8, 256, 2, 5
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    codes[n - 7:] = codes[:7]
    Q = rng.standard_normal((6, m * sd)).astype(F)
    ix = _index(coarse, cb, metric, lists, codes, False)
    px = PQIndex(cb, codes, vq_amd.Distance(NAMES[metric]))
    for density in (0.5, 0.01):
        mask = rng.random(n) < density
        mask[:3], mask[n - 7:n - 4] = False, True
        for topk in (10, 300):
            got = ix.masked_search(Q, mask, topk, nlist)
            _same(got, px.search(Q, topk, allowed=mask), f"density {density} topk {topk}: against PQIndex")
            _same(got, RPF.dense_search(orc, metric, cb, codes, Q, topk, mask), f"density {density} topk {topk}: against the statement")
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1023, 1024, 1025])
def test_view_edges(orc, n, residual):
    rng = np.random.default_rng(n)
    m, k, sd, nlist = 4, 16, 2, 3
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    Q = rng.standard_normal((4, m * sd)).astype(F)
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes, residual)
    topk = min(n, 5)
    masks = [np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1, np.arange(n) == 0, rng.random(n) < 0.5]
    for j, mask in enumerate(masks):
        for nprobe in (1, nlist):
            _same(ix.masked_search(Q, mask, topk, nprobe),
                  RPF.ivf_search(orc, residual, K.EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, topk, mask), f"mask {j} nprobe {nprobe}")
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_view_follows_the_call_and_the_rows(orc, residual):
    """unmasked, masked, unmasked on one handle; two masks in succession; an add_codes between two masked calls"""
    import vq_amd

    rng = np.random.default_rng(13)
    metric = K.MANHATTAN
    coarse, cb, lists, codes, Q = _base(rng, 8, 256, 2)
    h = 1700
    ix = _index(coarse, cb, metric, lists[:h], codes[:h], residual)
    st = lambda n, mask: RPF.ivf_search(orc, residual, metric, coarse, cb, lists[:n], codes[:n], Q, 3, 10, mask)
    first = ix.search(Q, 10, 3)
    _same(first, _unmasked(orc, residual, metric, coarse, cb, lists[:h], codes[:h], Q, 3, 10))
    a, b = rng.random(h) < 0.5, rng.random(h) < 0.1
    _same(ix.masked_search(Q, a, 10, 3), st(h, a), "mask a")
    _same(ix.search(Q, 10, 3), first, "unmasked after masked")
    _same(ix.masked_search(Q, b, 10, 3), st(h, b), "mask b")
    _same(ix.masked_search(Q, a, 10, 3), st(h, a), "mask a again")
    assert np.array_equal(ix.add_codes(lists[h:], codes[h:]), np.arange(h, N))
    with pytest.raises(vq_amd.DimensionMismatch):  # the mask of the index as it was
        ix.masked_search(Q, a, 10, 3)
    c = rng.random(N) < 0.3
    _same(ix.masked_search(Q, c, 10, 3), st(N, c), "after add_codes")
    _same(ix.search(Q, 10, 3), _unmasked(orc, residual, metric, coarse, cb, lists, codes, Q, 3, 10), "unmasked after add_codes")
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_two_batches(orc, residual):
    """1100 queries over 3000 rows: a batch holds at most 1024 queries"""
    rng = np.random.default_rng(3)
    n, m, k, sd, nlist = 3000, 4, 32, 1, 6
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8)
    Q = rng.standard_normal((1100, m * sd)).astype(F)
    mask = rng.random(n) < 0.3
    ix = _index(coarse, cb, K.SQUARED_EUCLIDEAN, lists, codes, residual)
    got = ix.masked_search(Q, mask, 10, 2)
    # every query's padding-free result is an allowed row; the statement for the queries around the batch edge and a sample
    assert mask[got[0][got[0] != PAD]].all()
    sample = sorted({0, 1, 1022, 1023, 1024, 1025, 1099} | set(rng.integers(0, 1100, 40).tolist()))
    want = RPF.ivf_search(orc, residual, K.SQUARED_EUCLIDEAN, coarse, cb, lists, codes, Q, 2, 10, mask, queries=sample)
    _same((got[0][sample], got[1][sample]), (want[0][sample], want[1][sample]))
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
@pytest.mark.parametrize("off", [1, 3])
def test_device_form_at_offset_pointers(orc, off, residual):
    import torch

    import vq_amd
    from vq_amd import _lib

    rng = np.random.default_rng(off)
    m, k, sd, nq, topk, nprobe = 8, 256, 2, 9, 17, 3
    d = m * sd
    coarse, cb, lists, codes, _ = _base(rng, m, k, sd)
    Q = rng.standard_normal((nq, d)).astype(F)
    mask = rng.random(N) < 0.3
    mask[64:256] = False
    w = RF.pack(mask)
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mb = torch.full((w.size + off + 8,), -1, dtype=torch.int32, device=dev)  # all ones around the mask
    mb[off:off + w.size] = torch.from_numpy(w.view(np.int32)).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes, residual)
    ix.masked_search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off,
                            mb.data_ptr() + 4 * off, nprobe=nprobe)
    torch.cuda.synchronize()
    _lib.synchronize()
    gi = ib.cpu().numpy()
    gd = db.cpu().numpy()
    _same((gi[off:off + nq * topk].view(np.uint32).reshape(nq, topk), gd[off:off + nq * topk].reshape(nq, topk)),
          RPF.ivf_search(orc, residual, K.EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, topk, mask))
    assert (gi[:off] == 7).all() and (gi[off + nq * topk:] == 7).all()
    assert (gd[:off] == -1.0).all() and (gd[off + nq * topk:] == -1.0).all()
    assert (mb.cpu().numpy()[off:off + w.size].view(np.uint32) == w).all()
    with pytest.raises(vq_amd.FfiError, match="aligned"):
        ix.masked_search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr(), db.data_ptr(), mb.data_ptr() + 2, nprobe=nprobe)
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_rerank_filters_the_first_stage(orc, residual):
    """rerank= through a FlatIndex under a mask that leaves some queries short of `candidates`: the reranker sees allowed rows
    only, full queries are the exact top-k of their candidates, short ones keep their padding"""
    import vq_amd

    rng = np.random.default_rng(21)
    m, k, sd = 8, 256, 2
    coarse, cb, lists, codes, Q = _base(rng, m, k, sd)
    X = rng.standard_normal((N, m * sd)).astype(F)  # the rows behind the codes, as far as the reranker is concerned
    fx = vq_amd.FlatIndex(X, vq_amd.Distance("euclidean"))
    mask = np.zeros(N, bool)
    mask[np.flatnonzero(lists == BIG)[:300]] = True
    mask[np.flatnonzero(lists == 3)[:6]] = True  # a query whose probed list is list 3 has six candidates
    mask[500] = True                             # the one-row list
    ix = _index(coarse, cb, K.EUCLIDEAN, lists, codes, residual)
    topk, cand, nprobe = 5, 20, 1
    idx, dist = ix.masked_search(Q, mask, topk, nprobe, rerank=fx, candidates=cand)
    first = RPF.ivf_search(orc, residual, K.EUCLIDEAN, coarse, cb, lists, codes, Q, nprobe, cand, mask)[0]
    real = (first != PAD).sum(axis=1)
    assert (real == cand).any() and ((real > 0) & (real < cand)).any() and (real == 0).any()
    for j in range(Q.shape[0]):
        c = first[j][:real[j]]
        t = min(topk, c.size)
        assert (idx[j, t:] == PAD).all() and np.isposinf(dist[j, t:]).all()
        if t:
            wi, wd = K.rerank(K.EUCLIDEAN, Q[j:j + 1], X, c[None, :], t)
            assert np.array_equal(idx[j, :t], wi[0]) and np.array_equal(dist[j, :t].view(np.uint32), wd[0].view(np.uint32))
    assert mask[idx[idx != PAD]].all()
    ix.close()


@pytest.mark.parametrize("residual", KINDS)
def test_two_threads_on_one_handle(orc, residual):
    """one thread searches under a mask, the other without, on the same handle: each call against its statement"""
    rng = np.random.default_rng(31)
    metric = K.SQUARED_EUCLIDEAN
    coarse, cb, lists, codes, Q = _base(rng, 8, 256, 2)
    mask = rng.random(N) < 0.3
    ix = _index(coarse, cb, metric, lists, codes, residual)
    want_m = RPF.ivf_search(orc, residual, metric, coarse, cb, lists, codes, Q, 3, 10, mask)
    want_u = _unmasked(orc, residual, metric, coarse, cb, lists, codes, Q, 3, 10)
    _same(ix.search(Q, 10, 3), want_u)  # (the device state is built before the threads start)
    errors = []

    def run(call, want, what):
        try:
            for _ in range(12):
                _same(call(), want, what)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(lambda: ix.masked_search(Q, mask, 10, 3), want_m, "masked")),
               threading.Thread(target=run, args=(lambda: ix.search(Q, 10, 3), want_u, "unmasked"))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    ix.close()


DRAWS = 40


def _draw(seed):
    rng = np.random.default_rng(93_000 + seed)
    n = int(rng.integers(1, 3001))
    m, k, sd = [(8, 256, 2), (4, 300, 3), (3, 16, 5), (16, 64, 1), (1, 7, 4)][int(rng.integers(0, 5))]
    nlist = int(rng.integers(1, 41))
    nprobe = int(rng.integers(1, nlist + 1))
    metric = int(rng.integers(0, 3))
    residual = bool(rng.integers(0, 2))
    density = [0.0, -1.0, 0.01, 0.5, 1.0][int(rng.integers(0, 5))]  # -1: one row
    block = bool(rng.integers(0, 2))
    count = 1 if density < 0 else int(round(density * n))
    mask = np.zeros(n, bool)
    if block:
        a = int(rng.integers(0, n - count + 1))
        mask[a:a + count] = True
    else:
        mask[rng.permutation(n)[:count]] = True
    return rng, n, m, k, sd, nlist, nprobe, metric, residual, mask


@pytest.mark.parametrize("seed", range(DRAWS))
def test_random_draws(orc, seed):
    rng, n, m, k, sd, nlist, nprobe, metric, residual, mask = _draw(seed)
    coarse = rng.standard_normal((nlist, m * sd)).astype(F)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    codes = rng.integers(0, k, (n, m)).astype(_code_dtype(k))
    if n > 8:
        codes[n - 1] = codes[0]
        lists[n - 1] = lists[0]
    Q = rng.standard_normal((4, m * sd)).astype(F)
    topk = int(rng.integers(1, min(n, 64) + 1))
    what = (f"seed {seed}: n {n} m {m} k {k} sd {sd} nlist {nlist} nprobe {nprobe} metric {metric} residual {residual} "
            f"allowed {int(mask.sum())} topk {topk}")
    ix = _index(coarse, cb, metric, lists, codes, residual)
    _same(ix.masked_search(Q, RF.pack(mask), topk, nprobe),
          RPF.ivf_search(orc, residual, metric, coarse, cb, lists, codes, Q, nprobe, topk, mask), what)
    ix.close()
