"""Removing rows from IVFPQIndex, IVFFlatIndex, IVFScalarIndex and IVFBinaryIndex (include/vqhip.h, "removing rows from
an inverted file") against the one statement there is: after any sequence of adds and removals,
every call on the index returns bit for bit what a fresh index returns that was given the remaining list ids and rows in
one add.  Distances are compared as uint32 bits, at nprobe 1 and nprobe == nlist.  A removal behind a search runs on the
device and must leave the device state current: ``uploads`` does not move."""
import numpy as np
import pytest

import ivf_mutate_cases as IC
import ref_mutate as RM
from vq_amd import (DimensionMismatch, Distance, FlatIndex, InvalidParameter, IVFScalarIndex, ScalarIndex, _lib)

pytestmark = pytest.mark.gpu
F = np.float32
N0 = 1501  # not a multiple of 32 (a mask word), of 64 or of 1024 (a block of the view)
NQ, TOPK = 3, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_pair(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: distance bits differ"


def same_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: lims differ"
    assert np.array_equal(got[1], want[1]), f"{what}: indices differ"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{what}: distance bits differ"


def queries(kind):
    """one query beside the centroid of list 0, of list 1 and of the list that never holds a row"""
    c = IC.coarse(kind)[[0, 1, IC.EMPTY_LIST]]
    return (c + F(0.01) * np.random.default_rng(5).standard_normal(c.shape).astype(F)).astype(F)


def searches(kind, ix, Q, k, nprobe, mask, radii=None):
    """every search of the kind at one nprobe: name -> result; the radii of the range calls come from the first caller"""
    fam = IC.family(kind)
    out = {"probe": (ix.probe(Q, nprobe),), "search": ix.search(Q, k, nprobe)}
    if fam == "pq":
        out["masked search"] = ix.masked_search(Q, mask, k, nprobe)
        return out, None
    if fam == "bin":
        r = max(1, IC.dim(kind) // 2 - 2)
        out["filtered search"] = ix.filtered_search(Q, mask, k, nprobe)
        out["range"] = ix.hamming_range_search(Q, r, nprobe)
        out["filtered range"] = ix.filtered_hamming_range_search(Q, r, mask, nprobe)
        return out, None
    if radii is None:  # a handful of hits per query; a query without a real hit (padding: +inf) gets a radius of 1
        d = out["search"][1][:, min(k, 3) - 1]
        radii = np.where(np.isfinite(d), d, F(1.0)).astype(F)
    out["masked search"] = ix.search(Q, k, nprobe, allowed=mask)
    out["range"] = ix.range_search(Q, radii, nprobe)
    out["masked range"] = ix.range_search(Q, radii, nprobe, allowed=mask)
    return out, radii


def check_invariant(kind, ix, lists, rows, what, tmp_path=None, seed=7):
    """every call of the statement on `ix` against a fresh index given (lists, rows) in one add; returns the fresh one"""
    want = IC.same_host_state(kind, ix, lists, rows, what, tmp_path)
    n = lists.shape[0]
    Q = queries(kind)
    if n == 0:  # an empty inverted file: it probes, and no topk is legal
        assert np.array_equal(ix.probe(Q, 1), want.probe(Q, 1)), f"{what}: probe"
        with pytest.raises(InvalidParameter):
            ix.search(Q, 1, 1)
        return want
    rng = np.random.default_rng(seed + n)
    mask = rng.random(n) < 0.5
    mask[int(rng.integers(n))] = True
    k = min(n, TOPK)
    for nprobe in (1, IC.NLIST):
        exp, radii = searches(kind, want, Q, k, nprobe, mask)
        got, _ = searches(kind, ix, Q, k, nprobe, mask, radii)
        for name in exp:
            cmp = same_csr if "range" in name else same_pair if len(exp[name]) == 2 else None
            if cmp:
                cmp(got[name], exp[name], f"{what}, nprobe {nprobe}: {name}")
            else:
                assert np.array_equal(got[name][0], exp[name][0]), f"{what}, nprobe {nprobe}: {name}"
    if n < 1024:  # the bounds follow the current n
        with pytest.raises(InvalidParameter):
            ix.search(Q, n + 1, 1)
    with pytest.raises(DimensionMismatch):
        searches(kind, ix, Q, k, 1, np.ones(n + 1, bool))
    return want


def built(kind, seed=1, n=N0, search=True):
    """an index of n rows; search: its device state is built (one upload)"""
    lists, rows = IC.gen(kind, seed, n)
    ix = IC.make(kind)
    IC.add(ix, kind, lists, rows)
    if search:
        ix.search(queries(kind), TOPK, 1)
        assert ix._ix.uploads() == 1
    return ix, lists, rows


def removal_masks(lists):
    n = lists.shape[0]
    one = np.ones(n, bool)
    one[700] = False
    return {
        "random 20 %": np.random.default_rng(11).random(n) < 0.2,
        "rows 128..447": np.arange(128, 448),
        "row 0": np.array([0]),
        "row n - 1": np.array([n - 1], dtype=np.uint32),
        "one whole list": lists == 0,  # the query beside its centroid gets padding at nprobe 1
        "all but one": one,
        "every row": np.ones(n, bool),
    }


@pytest.mark.parametrize("kind", list(IC.KINDS))
def test_a_removal_on_the_device_equals_a_fresh_index(kind, tmp_path):
    lists0, rows0 = IC.gen(kind, 1, N0)
    for name, m in removal_masks(lists0).items():
        ix, lists, rows = built(kind)
        keep = RM.kept(N0, m)
        got = ix.remove_rows(m)
        assert got.dtype == np.uint32 and np.array_equal(got, keep), f"{kind}, {name}: kept differs"
        assert ix._ix.uploads() == 1, f"{kind}, {name}: the removal moved the upload counter"
        lists, rows = lists[keep], rows[keep]
        want = check_invariant(kind, ix, lists, rows, f"{kind}, {name}", tmp_path if name == "random 20 %" else None)
        assert ix._ix.uploads() == 1, f"{kind}, {name}: the search behind the removal paid an upload"
        if name == "one whole list":
            idx, _ = ix.search(queries(kind), TOPK, 1)
            assert (idx[0] == 0xFFFFFFFF).all(), "the query beside the emptied list's centroid found rows at nprobe 1"
        if name in ("every row", "random 20 %"):  # later adds work, and the search behind one uploads
            l2, r2 = IC.gen(kind, 31, 40)
            assert np.array_equal(IC.add(ix, kind, l2, r2), np.arange(keep.shape[0], keep.shape[0] + 40))
            lists, rows = np.concatenate([lists, l2]), np.concatenate([rows, r2])
            check_invariant(kind, ix, lists, rows, f"{kind}, {name}, then 40 rows added")
            assert ix._ix.uploads() == 2
        want.close()
        ix.close()


@pytest.mark.parametrize("kind", IC.ONE_PER_INDEX)
def test_the_host_path_and_a_closed_handle_give_the_same(kind):
    m = np.random.default_rng(12).random(N0) < 0.2
    keep = RM.kept(N0, m)
    # before any search, with and without the handle
    for handle in (False, True):
        ix, lists, rows = built(kind, search=False)
        if handle:
            ix._handle()
        assert np.array_equal(ix.remove_rows(m), keep)
        check_invariant(kind, ix, lists[keep], rows[keep], f"{kind}: removal before any search (handle: {handle})")
        assert ix._ix.uploads() == 1  # (check_invariant's first search)
    # behind an add that left the device state stale
    ix, lists, rows = built(kind, n=N0 - 40)
    l2, r2 = IC.gen(kind, 32, 40)
    IC.add(ix, kind, l2, r2)
    lists, rows = np.concatenate([lists, l2]), np.concatenate([rows, r2])
    assert np.array_equal(ix.remove_rows(m), keep) and ix._ix.uploads() == 1
    check_invariant(kind, ix, lists[keep], rows[keep], f"{kind}: removal behind an add")
    assert ix._ix.uploads() == 2
    # after close()
    ix, lists, rows = built(kind)
    ix.close()
    assert np.array_equal(ix.remove_rows(m), keep)
    check_invariant(kind, ix, lists[keep], rows[keep], f"{kind}: removal after close()")


def test_the_view_scan_carries_across_more_than_1024_blocks():
    """1 Mi + 1500 one-byte rows are 1026 blocks of 1024 positions: the view's scan takes 1024 block counts per pass"""
    n = (1 << 20) + 1500
    rng = np.random.default_rng(3)
    coarse = np.array([[-2.0], [0.0], [2.0]], F)
    codes = rng.integers(0, 256, (n, 1), dtype=np.uint8)
    lists = rng.integers(0, 3, n).astype(np.uint32)
    m = rng.random(n) < 0.5
    Q = np.array([[-1.9], [0.1], [2.5]], F)
    ix = IVFScalarIndex(coarse, IC.SQ, Distance.manhattan())
    ix.add_codes(lists, codes)
    ix.search(Q, TOPK, 3)
    assert np.array_equal(ix.remove_rows(m), np.flatnonzero(~m).astype(np.uint32))
    assert len(ix) == int((~m).sum()) and ix._ix.uploads() == 1
    fresh = IVFScalarIndex(coarse, IC.SQ, Distance.manhattan())
    fresh.add_codes(lists[~m], codes[~m])
    for nprobe in (1, 3):
        same_pair(ix.search(Q, TOPK, nprobe), fresh.search(Q, TOPK, nprobe), f"nprobe {nprobe}")
    radii = np.full(3, 0.05, F)
    same_csr(ix.range_search(Q, radii, 3), fresh.range_search(Q, radii, 3), "range")
    assert ix._ix.uploads() == 1
    assert np.array_equal(ix.codes, codes[~m])


@pytest.mark.parametrize("kind", IC.ONE_PER_INDEX)
def test_a_sequence_of_twelve_ops(kind, tmp_path):
    """12 ops: the first two take n from 1501 to 0 and up to 2999, the other ten are drawn -- an add, a removal (on the
    device: the check behind every op searches), an add and a removal together (on the host: the add left the device state
    stale).  The statement is checked behind each."""
    rng = np.random.default_rng(sum(map(ord, kind)))  # (a seed per kind that is the same in every process)
    ix, lists, rows = built(kind, seed=13)
    ops = ["remove_all", "add_many"] + [str(o) for o in rng.choice(["add", "remove", "add_remove"], 10)]
    for j, op in enumerate(ops):
        if op in ("add_many", "add", "add_remove"):
            b = 2999 if op == "add_many" else int(rng.choice([1, 70, 700]))
            l2, r2 = IC.gen(kind, 100 + j, b)
            IC.add(ix, kind, l2, r2)
            lists, rows = np.concatenate([lists, l2]), np.concatenate([rows, r2])
        if op in ("remove_all", "remove", "add_remove"):
            n = lists.shape[0]
            m = np.ones(n, bool) if op == "remove_all" else rng.random(n) < float(rng.choice([0.1, 0.6]))
            before = ix._ix.uploads()
            assert np.array_equal(ix.remove_rows(m), RM.kept(n, m))
            assert ix._ix.uploads() == before
            lists, rows = lists[~m], rows[~m]
        before = ix._ix.uploads()
        check_invariant(kind, ix, lists, rows, f"{kind}, op {j} ({op})", tmp_path if j in (0, 1, 11) else None, seed=j).close()
        assert ix._ix.uploads() == before + (op != "remove" and op != "remove_all"), f"{kind}, op {j} ({op}): uploads"


def pair_rows(d, seed):
    return np.random.default_rng(seed).standard_normal((N0, d)).astype(F)


@pytest.mark.parametrize("pair", ["ivfpq + flat", "ivfbin + scalar"])
def test_an_index_and_its_reranker_follow_the_same_removal(pair):
    kind = "pq_m8_k16" if pair == "ivfpq + flat" else "bin_d96"
    X = pair_rows(IC.dim(kind), 14)
    Q = queries(kind)
    S = np.random.default_rng(16).random(N0) < 0.3

    def make_pair(rows):
        ivf = IC.make(kind)
        ivf.add(rows)
        return ivf, (FlatIndex(rows, Distance.cosine()) if pair == "ivfpq + flat" else ScalarIndex(rows, IC.SQ))

    ivf, exact = make_pair(X)
    ivf.search(Q, TOPK, 2, rerank=exact, candidates=32)
    assert ivf._ix.uploads() == 1
    kept = ivf.remove_rows(S)
    assert np.array_equal(exact.remove_rows(S), kept) and ivf._ix.uploads() == 1
    got = ivf.search(Q, TOPK, 2, rerank=exact, candidates=32)
    fresh_ivf, fresh_exact = make_pair(X[kept])
    assert np.array_equal(fresh_ivf.list_ids, ivf.list_ids)
    same_pair(got, fresh_ivf.search(Q, TOPK, 2, rerank=fresh_exact, candidates=32), pair)
    assert ivf._ix.uploads() == 1


@pytest.mark.parametrize("kind", IC.ONE_PER_INDEX)
def test_save_and_load_behind_a_removal_on_the_device(kind, tmp_path):
    ix, lists, rows = built(kind, seed=18)
    m = np.random.default_rng(20).random(N0) < 0.4
    ix.remove_rows(m)
    fresh = IC.fresh(kind, lists[~m], rows[~m])
    assert IC.file_bytes(ix, tmp_path, "got") == IC.file_bytes(fresh, tmp_path, "want")
    back = type(ix).load(tmp_path / "got")
    Q = queries(kind)
    assert len(back) == int((~m).sum())
    for nprobe in (1, IC.NLIST):
        same_pair(back.search(Q, TOPK, nprobe), fresh.search(Q, TOPK, nprobe), f"{kind}: the loaded index")
        same_pair(ix.search(Q, TOPK, nprobe), fresh.search(Q, TOPK, nprobe), f"{kind}: the index itself")


def test_a_queued_device_search_completes_on_the_old_rows():
    """A search_device is queued on stream A behind a blocker; a removal, which swaps the buffers and frees the old ones,
    then runs on stream B.  A's result is the statement for the old rows, the next search the statement for the new.  One
    pass."""
    import torch

    kind = "flat32_d21_cos"
    ix, lists, rows = built(kind, seed=22)
    Q = queries(kind)
    m = np.random.default_rng(23).random(N0) < 0.5
    want_old = ix.search(Q, TOPK, IC.NLIST)  # (the workspaces of this search exist)
    qd = torch.from_numpy(Q).to("cuda:0")
    idx = torch.zeros((NQ, TOPK), dtype=torch.int32, device="cuda:0")
    dist = torch.zeros((NQ, TOPK), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        _lib.set_stream(a.cuda_stream)
        with torch.cuda.stream(a):
            torch.cuda._sleep(12_000_000)  # about 5 ms: the search is still queued when the removal enters
        ix.search_device(qd.data_ptr(), NQ, TOPK, idx.data_ptr(), dist.data_ptr(), IC.NLIST)
        busy = not a.query()
        _lib.set_stream(b.cuda_stream)
        ix.remove_rows(m)
    finally:
        _lib.set_stream(None)
    torch.cuda.synchronize()
    assert busy, "no overlap achieved: the search had run before the removal entered"
    same_pair((idx.cpu().numpy().view(np.uint32), dist.cpu().numpy()), want_old, "the queued search")
    assert ix._ix.uploads() == 1
    check_invariant(kind, ix, lists[~m], rows[~m], "behind the removal")
