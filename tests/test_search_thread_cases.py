"""The cases of the threaded search tests (tests/search_thread_cases.py) are valid calls and exercise what they claim.  No
GPU: the arguments against the bounds of include/vqhip.h, the masks, the schedule of the threads, and the statements of the
four prefixes, which must differ for "equals one prefix" to say anything."""
import numpy as np
import pytest

import search_thread_cases as T

ALL = tuple(T.KINDS)
IVF_KINDS = tuple(k for k in ALL if T.KINDS[k][0] in T.IVF)


def _check_variant(c, v, n0):
    """v is a valid call of include/vqhip.h on an index of n0 rows or more"""
    assert 1 <= v.nq and v.q0 + v.nq <= T.NQ
    if v.op in ("search", "search_masked", "search_codes"):
        assert 1 <= v.topk <= min(n0, 1024), v.describe()
    if c.ivf:
        assert 1 <= v.nprobe <= min(T.NLIST, 1024), v.describe()
    else:
        assert v.nprobe == 0
    if v.masked:
        assert c.family in T.EXACT and v.mask.dtype == np.bool_ and v.mask.shape == (T.N,)
    if v.op.startswith("range"):
        assert v.radii.dtype == np.float32 and v.radii.shape == (v.nq,) and not np.isnan(v.radii).any()
        assert v.radii[-1] == -1.0 and v.radii[-2] == np.inf
    if v.op == "hamming_range_search":
        assert v.radii.dtype == np.uint32 and v.radii.shape == (v.nq,)
        assert v.radii[0] == 0 and v.radii[-1] == T.D and v.radii[-2] == 0xFFFFFFFF
    if v.op == "rerank":
        assert v.cand.shape == (v.nq, T.RERANK_C) and v.cand.max() < n0 and 1 <= v.topk <= T.RERANK_C <= 4096
        assert all(np.unique(row).size == T.RERANK_C for row in v.cand)


def test_the_data_crosses_the_edges():
    d = T.base()
    assert T.N > 2048 and T.N % 32 and T.N % 64 and T.D == 33
    sizes = np.bincount(d["lists"], minlength=T.NLIST)
    assert T.NLIST == 37 and (sizes == 0).sum() == T.EMPTY_LISTS
    assert np.array_equal(d["queries"][3], d["coarse"][d["empty"][0]])  # a query at the centroid of an empty list
    assert np.isnan(d["queries"][2]).sum() == 1 and not d["queries"][1].any()
    for p in T.PREFIXES:  # every prefix ends in twins of rows 0..2, in their lists
        assert np.array_equal(d["rows"][p - 3:p], d["rows"][:3]) and np.array_equal(d["lists"][p - 3:p], d["lists"][:3])
    assert list(T.PREFIXES) == sorted(set(T.PREFIXES)) and T.PREFIXES[-1] == T.N
    assert len({b - a for a, b in zip(T.PREFIXES, T.PREFIXES[1:])}) == 3  # three uneven slices


def test_the_masks_are_what_they_claim():
    m = T.base()["masks"]
    sparse, half, few = m["sparse"], m["half"], m["few"]
    assert 0.004 < sparse.mean() < 0.02
    tiles = sparse[:T.N // 64 * 64].reshape(-1, 64).any(axis=1)
    assert (~tiles).sum() >= 5  # whole 64-row tiles without an allowed row
    assert sparse.sum() >= T.TOPK_MID  # (and still topk allowed rows: its padding comes from the probed lists alone)
    assert 0.45 < half.mean() < 0.55
    assert few.sum() == T.FEW < T.TOPK_MID  # fewer allowed rows than topk: padding slots
    assert sparse[T.N - 1]  # the last row, in the mask's ragged last word


@pytest.mark.parametrize("kind", ALL)
def test_every_variant_is_a_valid_call_with_a_statement(kind):
    c = T.case(kind)
    names = [v.name for v in c.variants]
    assert len(set(names)) == len(names)
    for v in c.variants:
        _check_variant(c, v, T.N)
        assert v.want is not None
        if v.op in ("search", "search_masked", "search_codes", "rerank"):
            assert v.want[0].shape == v.want[1].shape == (v.nq, v.topk)
            assert v.want[0].dtype == np.uint32 and v.want[1].dtype == np.float32
        elif v.op == "probe":
            assert v.want[0].shape == (v.nq, v.nprobe) and v.want[0].dtype == np.uint32
        else:
            lims, idx, dist = v.want
            assert lims.dtype == np.uint64 and lims.shape == (v.nq + 1,) and lims[-1] == idx.size == dist.size
    ops = {v.op for v in c.variants}
    shapes = {(v.nq, v.topk) for v in c.variants if v.op == "search"}
    assert shapes == {(nq, topk) for nq, topk, _ in T.SHAPES}
    if c.family in T.EXACT:
        assert {"search_masked", "range_search", "range_search_masked"} <= ops
        assert {v.name for v in c.variants if v.op == "search_masked"} == {"masked_sparse", "masked_half", "masked_few"}
        few = next(v for v in c.variants if v.name == "masked_few")
        pad = few.want[0] == np.uint32(0xFFFFFFFF)
        assert pad[:, T.FEW:].all() and few.mask.sum() < few.topk  # padding slots appear
        assert (few.want[1].view(np.uint32)[pad] == np.uint32(0x7F800000)).all()
    if c.family in ("flat", "sqindex"):
        assert "rerank" in ops
    if c.family in ("binary", "ivfbin"):
        assert "hamming_range_search" in ops
    if c.ivf:
        assert len({v.nprobe for v in c.variants if v.op == "probe"}) == 2
        assert len({v.nprobe for v in c.variants if v.op == "search"}) == 3  # the workspace W is sized by nprobe


def test_hamming_and_distance_radii_select_neither_none_nor_all():
    for kind in ALL:
        for v in T.case(kind).variants:
            if v.op in ("range_search", "hamming_range_search"):
                per = np.diff(v.want[0].astype(np.int64))
                if T.case(kind).ivf:  # (a query whose probed lists hold none of its KTH nearest rows has no hit)
                    assert 0 < np.median(per[4:-2]) and per[4:-2].max() < T.N, (kind, v.name)
                else:
                    assert 0 < per[4:-2].min() and per[4:-2].max() < T.N, (kind, v.name)
                if v.op == "range_search":
                    assert per[-1] == 0 and per[-2] > per[4:-2].min()  # the -1 and the +inf query
                else:                                                  # the dimension and 2^32 - 1: every (probed) row
                    assert min(per[-1], per[-2]) > per[4:-2].min() and (T.case(kind).ivf or per[-1] == per[-2] == T.N)


def test_the_metrics_cover_a_sum_and_a_cosine_per_exact_family():
    for fam in T.EXACT:
        metrics = {T.KINDS[k][1] for k in ALL if T.KINDS[k][0] == fam}
        assert metrics & {T.K.SQUARED_EUCLIDEAN, T.K.EUCLIDEAN, T.K.MANHATTAN} and metrics & {T.K.COSINE, T.K.COSINE_UNCLAMPED}
    assert {T.KINDS[k][2]["dtype"] for k in ALL if T.KINDS[k][0] == "flat"} == {"float32", "float16"}
    assert {T.KINDS[k][2]["residual"] for k in ALL if T.KINDS[k][0] == "ivfpq"} == {False, True}
    assert {T.KINDS[k][0] for k in ALL} == {"flat", "sqindex", "binary", "pq", "ivfpq", "ivfflat", "ivfsq", "ivfbin"}


@pytest.mark.parametrize("kind", ALL)
def test_the_schedule_puts_different_variants_side_by_side(kind):
    c = T.case(kind)
    nv = len(c.variants)
    sched = T.schedule(nv)
    assert len(sched) == T.THREADS and all(len(s) == T.ITERS for s in sched)
    for i in range(T.ITERS):
        col = [sched[t][i] for t in range(T.THREADS)]
        assert all(a != b for a, b in zip(col, col[1:]))      # neighbouring threads: never the same variant
        assert len(set(col)) == min(nv, T.THREADS)
    for s in sched:
        assert set(s) == set(range(nv))  # every thread makes every call
        if c.family in T.EXACT:  # a masked call directly before an unmasked search, and behind one: a leaked mask slot shows
            kinds = [c.variants[j].masked for j in s]
            ops = [c.variants[j].op for j in s]
            assert any(a and not b and ops[i + 1] == "search" for i, (a, b) in enumerate(zip(kinds, kinds[1:])))
            assert any(not a and b for a, b in zip(kinds, kinds[1:]))


@pytest.mark.parametrize("kind", IVF_KINDS)
def test_the_four_prefix_statements_differ(kind):
    a = T.add_case(kind)
    assert T.PREFIXES[0] >= max(v.topk for v in a.variants)
    for v in a.variants:
        for n in T.PREFIXES:
            _check_variant(a.case, v, n)
        assert len(v.want) == len(T.PREFIXES)
        for i in range(len(T.PREFIXES)):
            for j in range(i + 1, len(T.PREFIXES)):
                assert not T.same(v.want[i], v.want[j]), f"{kind} {v.name}: prefixes {i} and {j} give one result"
    assert [int(s.sum()) for s in a.sizes] == list(T.PREFIXES)
    if a.case.family in T.EXACT:
        assert {v.op for v in a.variants} == {"search", "range_search", "search_masked"}
        masked = next(v for v in a.variants if v.masked)
        assert masked.mask.shape == (T.N,)  # one mask of all N rows for every prefix: its bits past n are ignored


@pytest.mark.parametrize("kind", T.DEVICE_KINDS)
def test_the_device_cases_differ_between_the_two_threads(kind):
    c = T.case(kind)
    for masked in ((False, True) if c.family in ("ivfflat",) else (False,)):
        a, b = T.device_case(kind, masked)
        for v in (a, b):
            _check_variant(c, v, T.N)
        assert (a.nq, a.topk) != (b.nq, b.topk) and a.q0 + a.nq <= b.q0
        if masked:
            assert not np.array_equal(a.mask, b.mask)


@pytest.mark.parametrize("kind", T.REGROW_KINDS)
def test_the_regrowing_call_is_larger_in_every_workspace(kind):
    c = T.case(kind)
    small, big = T.regrow_case(kind)
    for v in (small, big):
        _check_variant(c, v, T.N)
    assert big.nq > small.nq and big.topk == 1024 > small.topk and big.masked and not small.masked
    assert big.nprobe >= small.nprobe and big.nq * big.topk > small.nq * small.topk
