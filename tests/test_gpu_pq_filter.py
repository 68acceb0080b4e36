"""Filtered ADC search on the MI355X (``PQIndex.search(allowed=)``, ``ProductQuantizer.search(allowed=)``,
vqhip_pq_adc_search_masked / _masked_device / _resident_masked: k_adc_scan_masked and the masked source of the selection stage,
vq_amd/csrc/k_adc.hip) against the numpy statement of include/vqhip.h (tests/ref_pq_filter.py): indices equal, distances equal
as uint32 bits, no tolerance anywhere.  Wave and block edges of n, the masks of test_gpu_ivfpq_filter.py plus masks that
leave whole 64-row groups empty, two-byte codes, m % 8 != 0, the table limit, dense ties among the allowed rows, short
results, the three C forms, the schedule a filtered call takes, rerank with short queries, seeded draws."""
import ctypes

import numpy as np
import pytest

import ref_filter as RF
import ref_knn as K
import ref_pq_filter as RPF

pytestmark = pytest.mark.gpu

F = np.float32
METRICS = (K.SQUARED_EUCLIDEAN, K.EUCLIDEAN, K.MANHATTAN)
NAMES = ["squared_euclidean", "euclidean", "manhattan"]
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


def _pqindex(cb, codes, metric):
    import vq_amd
    from vq_amd.store import PQIndex

    return PQIndex(cb, codes, vq_amd.Distance(NAMES[metric]))


def _case(rng, n, m, k, sd, nq=9):
    """nq = 9: a full batch of eight queries' tables in the LDS and a batch of one"""
    cb = rng.standard_normal((m, k, sd)).astype(F)
    codes = rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)
    if n > 16:
        codes[n - 3:] = codes[:3]  # duplicates: ties by row id
        codes[8:11] = codes[:3]
    Q = rng.standard_normal((nq, m * sd)).astype(F)
    Q[nq // 2] = 0.0
    return cb, codes, Q


def _masks(n, rng):
    """name -> (bool mask, what is handed to the index)"""
    def rand(p):
        m = rng.random(n) < p
        if n > 16:  # the duplicates on both sides of the mask
            m[0], m[1], m[2] = True, False, True
            m[8], m[9], m[10] = False, True, False
            m[n - 3], m[n - 2], m[n - 1] = False, True, True
        return m

    one = lambda i: np.arange(n) == i
    ids = np.arange(n)
    half = rand(0.5)
    tail = RF.pack(half).copy()
    if n % 32:
        tail[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # every bit past n in the last word set
    groups = ((ids // 64) % 3 == 0)  # whole 64-row groups empty between full ones
    out = {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "row0": one(0), "last": one(n - 1), "half": rand(0.5),
           "3pc": rand(0.03), "ids 100..333": (ids >= 100) & (ids < 333), "last partial wave": ids >= (n - 1) // 64 * 64,
           "groups": groups, "sparse groups": groups & (rng.random(n) < 0.1)}
    out = {k: (m, m) for k, m in out.items()}
    out["words"] = (out["3pc"][0], RF.pack(out["3pc"][0]))
    out["half+tail"] = (half, tail)
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099])
def test_search_matches_statement(orc, n, metric):
    rng = np.random.default_rng(10 * n + metric)
    cb, codes, Q = _case(rng, n, 8, 256, 2)
    px = _pqindex(cb, codes, metric)
    plain = px.search(Q, min(n, 10))
    for name, (mk, arg) in _masks(n, rng).items():
        want = RPF.dense_search(orc, metric, cb, codes, Q, min(n, 1024), mk)
        for topk in sorted({1, min(n, 10), min(n, 256), min(n, 1024)}) if name in ("half", "groups", "half+tail") else (min(n, 10),):
            got = px.search(Q, topk, allowed=arg)
            _same(got, (want[0][:, :topk], want[1][:, :topk]), f"{name}, topk {topk}")
            assert not np.isin(got[0], np.flatnonzero(~mk)).any(), name
            if name == "ones" and topk == min(n, 10):
                _same(got, plain, "all ones against the unfiltered call")
            if name == "zeros":
                assert (got[0] == PAD).all() and np.isposinf(got[1]).all()
    _same(px.search(Q, min(n, 10)), plain, "the unfiltered call after filtered ones")
    px._drop_encoder()


@pytest.mark.parametrize("metric", METRICS)
def test_one_scan_sized_store(orc, metric):
    """n = 40000, topk 10: the unfiltered call takes the one-scan schedule (no query, or few, through the full pass); every
    filtered call goes through the full pass, all nq queries of it, and the unfiltered call behind it is what it was"""
    n = 40000
    rng = np.random.default_rng(400 + metric)
    cb, codes, Q = _case(rng, n, 8, 256, 2)
    Q[4, 1] = np.nan
    Q[5, 0] = np.inf
    px = _pqindex(cb, codes, metric)
    plain = px.search(Q, 10)
    assert px._enc.adc_last_redone() < Q.shape[0]
    masks = _masks(n, rng)
    for name in ("ones", "zeros", "half", "3pc", "last partial wave", "sparse groups", "half+tail"):
        mk, arg = masks[name]
        got = px.search(Q, 10, allowed=arg)
        assert px._enc.adc_last_redone() == Q.shape[0], name
        _same(got, RPF.dense_search(orc, metric, cb, codes, Q, 10, mk), name)
        if name == "ones":
            _same(got, plain, "all ones against the unfiltered call")
    _same(px.search(Q, 10), plain, "the unfiltered call after filtered ones")
    px._drop_encoder()


@pytest.mark.parametrize("shape", [(4, 300, 3), (3, 16, 5), (150, 256, 1)])
def test_code_widths_and_the_table_limit(orc, shape):
    """two-byte codes; m % 8 != 0 (no 8-byte code words); m * k = 38400, one query's table per scan pass"""
    m, k, sd = shape
    n = 1500
    rng = np.random.default_rng(m * k)
    cb, codes, Q = _case(rng, n, m, k, sd, nq=5)
    masks = _masks(n, rng)
    for metric in (K.EUCLIDEAN, K.MANHATTAN):
        px = _pqindex(cb, codes, metric)
        for name in ("half", "3pc", "groups", "half+tail"):
            mk, arg = masks[name]
            _same(px.search(Q, 20, allowed=arg), RPF.dense_search(orc, metric, cb, codes, Q, 20, mk), f"{name} metric {metric}")
        px._drop_encoder()


@pytest.mark.parametrize("metric", [K.SQUARED_EUCLIDEAN, K.EUCLIDEAN])
def test_dense_select_over_tied_allowed_rows(orc, metric):
    """12000 of 20000 rows share one code row and 9000 of them are allowed: more than 8192 ties at the cut, so the selection
    goes through the radix select over (key, row id) of the allowed positions, and ties go to the lowest allowed rows"""
    rng = np.random.default_rng(70 + metric)
    n = 20000
    cb, codes, Q = _case(rng, n, 8, 32, 2, nq=3)
    tied = rng.permutation(n)[:12000]
    codes[tied] = codes[tied[0]]
    mask = rng.random(n) < 0.5
    mask[tied] = False
    mask[tied[:9000]] = True
    Q[0] = np.concatenate([cb[s][codes[tied[0], s]] for s in range(8)])  # the tied rows are its nearest
    px = _pqindex(cb, codes, metric)
    for topk in (10, 300):
        got = px.search(Q, topk, allowed=mask)
        _same(got, RPF.dense_search(orc, metric, cb, codes, Q, topk, mask), f"topk {topk}")
    assert np.array_equal(got[0][0], np.sort(tied[:9000])[:300])
    px._drop_encoder()


def test_fewer_allowed_rows_than_topk(orc):
    rng = np.random.default_rng(5)
    n = 4099
    cb, codes, Q = _case(rng, n, 8, 256, 2)
    px = _pqindex(cb, codes, K.EUCLIDEAN)
    for count, topk in ((7, 10), (600, 1024)):
        mask = np.zeros(n, bool)
        mask[rng.permutation(n)[:count]] = True
        got = px.search(Q, topk, allowed=mask)
        _same(got, RPF.dense_search(orc, K.EUCLIDEAN, cb, codes, Q, topk, mask), f"{count} allowed at topk {topk}")
        assert ((got[0] != PAD).sum(axis=1) == count).all() and np.isposinf(got[1][:, count:]).all()
    px._drop_encoder()


def test_three_c_forms_agree(orc):
    """host codes, device codes and the resident store: one result, the statement's; last_redone == nq after each"""
    import torch

    from vq_amd import _lib

    rng = np.random.default_rng(11)
    n, m, k, sd, topk = 4099, 8, 256, 2, 12
    cb, codes, Q = _case(rng, n, m, k, sd)
    mask = rng.random(n) < 0.2
    w = RF.pack(mask)
    want = RPF.dense_search(orc, K.MANHATTAN, cb, codes, Q, topk, mask)
    enc = _lib.PQEncoder(cb, _lib.MANHATTAN)
    try:
        _same(enc.adc_search(codes, Q, topk, allowed=w), want, "host codes")
        assert enc.adc_last_redone() == Q.shape[0]
        dev_codes = torch.from_numpy(codes).to("cuda:0")
        _same(enc.adc_search((dev_codes.data_ptr(), n), Q, topk, allowed=w), want, "device codes")
        assert enc.adc_last_redone() == Q.shape[0]
        enc.adc_set_codes(codes)
        _same(enc.adc_search(None, Q, topk, allowed=w), want, "resident")
        assert enc.adc_last_redone() == Q.shape[0]
        # a store replaced by a shorter one: the mask is that store's
        enc.adc_set_codes(codes[:1000])
        _same(enc.adc_search(None, Q, topk, allowed=RF.pack(mask[:1000])),
              RPF.dense_search(orc, K.MANHATTAN, cb, codes[:1000], Q, topk, mask[:1000]), "resident, replaced")
        # argument ranges on a real encoder
        L = _lib.load()
        f32p, u32p, u8p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        idx, dist = np.zeros((Q.shape[0], topk), np.uint32), np.zeros((Q.shape[0], topk), F)
        qp, wp, ip, dp = Q.ctypes.data_as(f32p), w.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), dist.ctypes.data_as(f32p)
        for bad_n in (0, 1 << 32):
            assert L.vqhip_pq_adc_search_masked(enc.raw, codes.ctypes.data_as(u8p), bad_n, qp, 2, 1, wp, ip, dp) == _lib.ERR_INVALID_INPUT
            assert L.vqhip_pq_adc_search_masked_device(enc.raw, ctypes.c_void_p(dev_codes.data_ptr()), bad_n, qp, 2, 1, wp, ip, dp) == _lib.ERR_INVALID_INPUT
        for bad_topk in (0, 1001, 1025):
            assert L.vqhip_pq_adc_search_resident_masked(enc.raw, qp, 2, bad_topk, wp, ip, dp) == _lib.ERR_INVALID_INPUT
            assert "topk" in _lib.last_error()
        enc.adc_set_codes(codes[:0])
        assert L.vqhip_pq_adc_search_resident_masked(enc.raw, qp, 2, 1, wp, ip, dp) == _lib.ERR_INVALID_INPUT
        assert "no codes loaded" in _lib.last_error()
    finally:
        enc.close()


def test_more_queries_than_one_group(orc):
    """70 queries over 4099 rows: two groups of launches (64 queries and 6), nine scan batches"""
    rng = np.random.default_rng(12)
    n = 4099
    cb, codes, Q = _case(rng, n, 8, 256, 2, nq=70)
    mask = rng.random(n) < 0.3
    px = _pqindex(cb, codes, K.SQUARED_EUCLIDEAN)
    _same(px.search(Q, 10, allowed=mask), RPF.dense_search(orc, K.SQUARED_EUCLIDEAN, cb, codes, Q, 10, mask))
    px._drop_encoder()


def test_product_quantizer_search_allowed(orc):
    import vq_amd
    from vq_amd.store import PQIndex

    rng = np.random.default_rng(13)
    n, m, k, sd = 2000, 4, 16, 4
    X = rng.standard_normal((n, m * sd)).astype(F)
    pq = vq_amd.ProductQuantizer(X, m, k, 2, vq_amd.Distance("euclidean"), 7)
    codes = pq.encode(X)
    Q = rng.standard_normal((5, m * sd)).astype(F)
    mask = rng.random(n) < 0.25
    want = RPF.dense_search(orc, K.EUCLIDEAN, pq.codebooks, codes, Q, 10, mask)
    _same(pq.search(codes, Q, 10, allowed=mask), want, "bools")
    _same(pq.search(codes, Q, 10, allowed=RF.pack(mask)), want, "words")
    _same(pq.search(codes, Q, 10, allowed=np.ones(n, bool)), pq.search(codes, Q, 10), "all ones against the unfiltered call")
    _same(PQIndex.from_quantizer(pq, X).search(Q, 10, allowed=mask), want, "PQIndex.from_quantizer")


def test_rerank_filters_the_first_stage(orc):
    """rerank= through a FlatIndex: with 300 allowed rows every query's 20 candidates are allowed rows and the result is
    their exact top-k; with 6 allowed rows every query is short and keeps its padding"""
    import vq_amd

    rng = np.random.default_rng(21)
    n, m, k, sd = 4099, 8, 256, 2
    cb, codes, Q = _case(rng, n, m, k, sd)
    X = rng.standard_normal((n, m * sd)).astype(F)
    fx = vq_amd.FlatIndex(X, vq_amd.Distance("euclidean"))
    px = _pqindex(cb, codes, K.EUCLIDEAN)
    pq_like = [lambda mask: px.search(Q, 5, rerank=fx, candidates=20, allowed=mask)]
    for count in (300, 6):
        mask = np.zeros(n, bool)
        mask[rng.permutation(n)[:count]] = True
        first = RPF.dense_search(orc, K.EUCLIDEAN, cb, codes, Q, 20, mask)[0]
        for call in pq_like:
            idx, dist = call(mask)
            for j in range(Q.shape[0]):
                c = first[j][first[j] != PAD]
                t = min(5, c.size)
                wi, wd = K.rerank(K.EUCLIDEAN, Q[j:j + 1], X, c[None, :], t)
                assert np.array_equal(idx[j, :t], wi[0]) and np.array_equal(dist[j, :t].view(np.uint32), wd[0].view(np.uint32))
                assert (idx[j, t:] == PAD).all() and np.isposinf(dist[j, t:]).all()
            assert mask[idx[idx != PAD]].all()
    px._drop_encoder()


DRAWS = 40


@pytest.mark.parametrize("seed", range(DRAWS))
def test_random_draws(orc, seed):
    rng = np.random.default_rng(94_000 + seed)
    n = int(rng.integers(1, 6001))
    m, k, sd = [(8, 256, 2), (4, 300, 3), (3, 16, 5), (16, 64, 1), (1, 7, 4)][int(rng.integers(0, 5))]
    metric = int(rng.integers(0, 3))
    density = [0.0, -1.0, 0.01, 0.5, 1.0][int(rng.integers(0, 5))]  # -1: one row
    block = bool(rng.integers(0, 2))
    count = 1 if density < 0 else int(round(density * n))
    mask = np.zeros(n, bool)
    if block:
        a = int(rng.integers(0, n - count + 1))
        mask[a:a + count] = True
    else:
        mask[rng.permutation(n)[:count]] = True
    nq = [1, 4, 13][int(rng.integers(0, 3))]
    cb, codes, Q = _case(rng, n, m, k, sd, nq=nq)
    topk = int(rng.integers(1, min(n, 64) + 1))
    what = f"seed {seed}: n {n} m {m} k {k} sd {sd} metric {metric} nq {nq} allowed {int(mask.sum())} topk {topk} block {block}"
    px = _pqindex(cb, codes, metric)
    _same(px.search(Q, topk, allowed=RF.pack(mask)), RPF.dense_search(orc, metric, cb, codes, Q, topk, mask), what)
    px._drop_encoder()
