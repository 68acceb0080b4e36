"""The lifecycle the three inverted-file indexes share (vq_amd/_ivf_common.py, the IvfLists layer of vq_amd/csrc/api_ivf.hip),
on the MI355X: IVFPQIndex, IVFFlatIndex (float32 and float16 rows) and IVFScalarIndex through the same steps -- search,
add, search again (the rebuild of the device lists after a search), close and search, list sizes, probe, and a query
whose only probed list is empty.  Every comparison is equality of indices and of distance bits; the expected values are
the numpy statements of tests/ref_ivf.py, tests/ref_ivfflat.py and tests/ref_ivfsq.py.

Shape: nlist 5 with list 2 left empty, dim 8, 37 rows and then 29 more with explicit list ids, 3 queries, topk 4,
nprobe 1 and 5 (= nlist); Euclidean, and cosine where the index has it (PQ has no ADC form of it)."""
import functools

import numpy as np
import pytest

import ref_ivf as I
import ref_ivfflat as RF
import ref_ivfsq as RS
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
NLIST, EMPTY, DIM, N1, N2, NQ, TOPK = 5, 2, 8, 37, 29, 3, 4
M, KC = 2, 16
SQ = (-3.0, 5.0, 17)
NPROBES = (1, NLIST)
CASES = [("pq", K.EUCLIDEAN), ("flat_f32", K.EUCLIDEAN), ("flat_f32", K.COSINE), ("flat_f16", K.EUCLIDEAN),
         ("flat_f16", K.COSINE), ("sq", K.EUCLIDEAN), ("sq", K.COSINE)]


@functools.lru_cache(maxsize=None)
def _case(kind, metric):
    """the inputs, and the statement's results after the first add and after both, per nprobe (computed once)"""
    rng = np.random.default_rng(5 + metric)
    n = N1 + N2
    coarse = rng.uniform(-2.0, 2.0, (NLIST, DIM)).astype(F)
    lists = rng.choice([l for l in range(NLIST) if l != EMPTY], n).astype(np.uint32)
    Q = rng.uniform(-2.0, 2.0, (NQ, DIM)).astype(F)
    Q[2] = coarse[EMPTY]  # its nearest centroid is the empty list's
    extra = ()
    if kind == "pq":
        extra = (rng.standard_normal((M, KC, DIM // M)).astype(F),)
        payload = rng.integers(0, KC, (n, M)).astype(np.uint8)
        payload[n - 3:], lists[n - 3:] = payload[:3], lists[:3]  # duplicates in the same lists: ties by row id

        def want(upto, nprobe):
            return I.brute_search(metric, coarse, extra[0], lists[:upto], payload[:upto], Q, nprobe, TOPK)
    elif kind == "sq":
        payload = rng.integers(0, 256, (n, DIM)).astype(np.uint8)
        payload[n - 3:], lists[n - 3:] = payload[:3], lists[:3]

        def want(upto, nprobe):
            return RS.search(metric, coarse, lists[:upto], SQ, payload[:upto], Q, nprobe, TOPK)
    else:
        payload = rng.uniform(-2.0, 2.0, (n, DIM)).astype(np.float16 if kind == "flat_f16" else F)
        payload[n - 3:], lists[n - 3:] = payload[:3], lists[:3]

        def want(upto, nprobe):
            return RF.search(metric, coarse, lists[:upto], payload[:upto], Q, nprobe, TOPK)
    with np.errstate(all="ignore"):
        wants = {(upto, p): want(upto, p) for upto in (N1, n) for p in NPROBES}
        probes = {p: I.probe(metric, coarse, Q, p) for p in NPROBES}
    assert probes[1][2, 0] == EMPTY and not np.any(lists == EMPTY)
    for a in (coarse, lists, Q, payload) + extra:
        a.setflags(write=False)
    return coarse, extra, lists, payload, Q, wants, probes


def _new(kind, metric):
    import vq_amd

    coarse, extra, *_ = _case(kind, metric)
    d = vq_amd.Distance(NAMES[metric])
    if kind == "pq":
        return vq_amd.IVFPQIndex(coarse, extra[0], d)
    if kind == "sq":
        return vq_amd.IVFScalarIndex(coarse, vq_amd.ScalarQuantizer(*SQ), d)
    return vq_amd.IVFFlatIndex(coarse, d, np.float16 if kind == "flat_f16" else np.float32)


def _add(ix, lists, payload):
    return ix.add_rows(lists, payload) if hasattr(ix, "rows") else ix.add_codes(lists, payload)


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert got[1].dtype == np.float32 and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("kind,metric", CASES)
def test_search_add_search_close_search(kind, metric):
    """(a) a search, an add and a search again equal a fresh index given every row in one add -- and the statement at
    both stages; (b) close() and the same search give the same arrays"""
    _, _, lists, payload, Q, wants, _ = _case(kind, metric)
    n = N1 + N2
    ix = _new(kind, metric)
    assert np.array_equal(_add(ix, lists[:N1], payload[:N1]), np.arange(N1, dtype=np.uint32))
    for p in NPROBES:
        _same(ix.search(Q, topk=TOPK, nprobe=p), wants[N1, p])
    assert np.array_equal(_add(ix, lists[N1:], payload[N1:]), np.arange(N1, n, dtype=np.uint32))
    fresh = _new(kind, metric)
    _add(fresh, lists, payload)
    for p in NPROBES:
        got = ix.search(Q, topk=TOPK, nprobe=p)
        _same(got, wants[n, p])
        _same(got, fresh.search(Q, topk=TOPK, nprobe=p))
    fresh.close()
    before = {p: ix.search(Q, topk=TOPK, nprobe=p) for p in NPROBES}
    ix.close()
    assert ix._ix is None and len(ix) == n
    for p in NPROBES:
        _same(ix.search(Q, topk=TOPK, nprobe=p), before[p])
        _same(before[p], wants[n, p])
    ix.close()


@pytest.mark.parametrize("kind,metric", CASES)
def test_list_sizes_probe_and_empty_list(kind, metric):
    """(c) list_sizes() of the index and of its handle agree and sum to n; (d) probe is FlatIndex(coarse).search;
    (e) the query that probes only the empty list gets padding in every slot"""
    import vq_amd

    coarse, _, lists, payload, Q, wants, probes = _case(kind, metric)
    n = N1 + N2
    ix = _new(kind, metric)
    _add(ix, lists[:N1], payload[:N1])
    _add(ix, lists[N1:], payload[N1:])
    sizes = ix.list_sizes()
    assert sizes.dtype == np.uint64 and sizes.shape == (NLIST,)
    assert np.array_equal(sizes, np.bincount(lists, minlength=NLIST)) and sizes.sum() == n and sizes[EMPTY] == 0
    assert np.array_equal(ix._handle().list_sizes(), sizes)
    flat = vq_amd.FlatIndex(coarse, vq_amd.Distance(NAMES[metric]))
    for p in NPROBES:
        got = ix.probe(Q, nprobe=p)
        assert got.dtype == np.uint32 and np.array_equal(got, probes[p])
        assert np.array_equal(got, flat.search(Q, p)[0])
    idx, dist = ix.search(Q, topk=TOPK, nprobe=1)
    assert np.all(idx[2] == np.uint32(0xFFFFFFFF)) and np.all(dist[2].view(np.uint32) == I.INF_BITS)
    assert np.all(wants[n, 1][0][2] == I.PAD_ID)  # (and so says the statement)
    _same((idx, dist), wants[n, 1])
    ix.close()
