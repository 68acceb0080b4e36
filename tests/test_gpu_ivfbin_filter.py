"""Filtered search of vq_amd.IVFBinaryIndex on the MI355X (``filtered_search``, ``filtered_hamming_range_search`` and
their device forms; vqhip_ivfbin_*_masked; the picked forms of k_ivfbin_tile and k_ivfbin_scan in
vq_amd/csrc/k_ivfbin.hip) against the numpy statement tests/ref_binary_filter.py and the four identities of DESIGN.md
section 24: indices, lims, and distances as uint32 bits.  No tolerances."""
import numpy as np
import pytest

import ref_binary as B
import ref_binary_filter as S
import ref_knn as K

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan"]
BQ = (0.25, 3, 200)
NLIST, N = 7, 1501
CM = K.EUCLIDEAN  # the coarse metric


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


def _case(rng, d, nq, n=N, nlist=NLIST):
    """rows in an order unrelated to their lists; list 2 is empty; duplicates within one list; query 0 equals row 21"""
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    lists[lists == 2] = 3
    rows = rng.standard_normal((n, d)).astype(F)
    rows[n - 7:] = rows[:7]
    lists[n - 7:] = lists[:7]
    Q = rng.standard_normal((nq, d)).astype(F)
    Q[0] = rows[21]
    return coarse, lists, rows, Q


def _masks(rng, lists):
    """name -> bool mask: list 4's rows all disallowed and list 5 with a single allowed row in every random mask"""
    n = lists.shape[0]

    def rand(p):
        m = rng.random(n) < p
        m[lists == 4] = False
        m[lists == 5] = False
        m[np.flatnonzero(lists == 5)[3]] = True
        m[0:7:2], m[1:7:2] = True, False  # the duplicates at the end on both sides of the mask
        m[n - 7::2], m[n - 6::2] = False, True
        m[21] = False  # query 0 equals a disallowed row
        return m

    return {"ones": np.ones(n, bool), "zeros": np.zeros(n, bool), "half": rand(0.5), "3pc": rand(0.03),
            "one list": lists == 1, "row0": np.arange(n) == 0}


def _index(coarse, metric, lists, words, bq=BQ):
    import vq_amd

    ix = vq_amd.IVFBinaryIndex(coarse, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]), vq_amd.Distance("euclidean"))
    ix.add_packed(lists, words)
    return ix


def _flat(words, d, metric, bq=BQ):
    import vq_amd

    return vq_amd.BinaryIndex.from_packed(words, d, vq_amd.BinaryQuantizer(*bq), vq_amd.Distance(NAMES[metric]))


@pytest.mark.parametrize("metric", B.METRICS)
@pytest.mark.parametrize("d", [1, 64, 96, 128, 1100])
@pytest.mark.parametrize("nq", [3, 40])
def test_search_and_range_match_statement(metric, d, nq):
    """W = 1, 2, 3, 4, 35: loaders 1, 2, 1, 4, 1 and two LDS chunks at d = 1100.  nq = 3: every list is under the tile
    kernel's minimum and takes the scan kernel; nq = 40 at nprobe == nlist: every list takes the tile kernel"""
    rng = np.random.default_rng(100 * metric + d)  # (the same data for both nq)
    coarse, lists, rows, Q = _case(rng, d, 40)
    Q = Q[:nq]
    words = B.pack(B.bits_f32(rows, BQ[0]))
    ix = _index(coarse, metric, lists, words)
    flat = _flat(words, d, metric)
    radius = np.resize(np.array([0, d // 2, d // 3, d + 7, d // 2 + 1], np.uint32), nq)
    for name, m in _masks(rng, lists).items():
        for nprobe in (1, 3, NLIST):
            what = f"{name} nprobe {nprobe}"
            got = ix.filtered_search(Q, m, 10, nprobe)
            _same(got, S.ivf_search(metric, CM, coarse, lists, BQ, words, d, Q, nprobe, 10, m), what)
            got_r = ix.filtered_hamming_range_search(Q, radius, m, nprobe)
            _same_range(got_r, S.ivf_range_search(metric, CM, coarse, lists, BQ, words, d, Q, nprobe, radius, m), what)
            if name == "ones":
                _same(got, ix.search(Q, 10, nprobe), what + ": all ones against the unmasked search")
                _same_range(got_r, ix.hamming_range_search(Q, radius, nprobe), what + ": all ones against the unmasked range")
            if name == "zeros":
                assert (got[0] == 0xFFFFFFFF).all() and np.isposinf(got[1]).all()
                assert not got_r[0].any() and got_r[1].size == 0
            if nprobe == NLIST:  # the filtered BinaryIndex over the words in add order
                _same(got, flat.filtered_search(Q, m, 10), what + ": against BinaryIndex")
                _same_range(got_r, flat.filtered_hamming_range_search(Q, radius, m), what + ": against BinaryIndex")


def test_scan_and_tile_kernels_give_the_same_bits():
    """the same (query, row) pairs through k_ivfbin_scan (3 queries) and k_ivfbin_tile (40 queries), picked"""
    rng = np.random.default_rng(8)
    d = 96
    coarse, lists, rows, Q = _case(rng, d, 40)
    words = B.pack(B.bits_f32(rows, BQ[0]))
    ix = _index(coarse, B.EUC, lists, words)
    m = rng.random(N) < 0.4
    big = ix.filtered_search(Q, m, 50, NLIST)
    small = ix.filtered_search(Q[:3], m, 50, NLIST)
    _same(small, (big[0][:3], big[1][:3]))
    big_r = ix.filtered_hamming_range_search(Q, d // 2, m, NLIST)
    small_r = ix.filtered_hamming_range_search(Q[:3], d // 2, m, NLIST)
    e = int(big_r[0][3])
    _same_range(small_r, (big_r[0][:4], big_r[1][:e], big_r[2][:e]))


def test_range_and_topk_agree():
    rng = np.random.default_rng(4)
    d, topk = 100, 20
    coarse, lists, rows, Q = _case(rng, d, 6)
    words = B.pack(B.bits_f32(rows, 0.0))
    ix = _index(coarse, B.MAN, lists, words, (0.0, 0, 1))  # D = H
    m = rng.random(N) < 0.5
    idx, dist = ix.filtered_search(Q, m, topk, 4)
    assert (idx != 0xFFFFFFFF).all()
    lims, ridx, rdist = ix.filtered_hamming_range_search(Q, dist[:, -1].astype(np.uint32), m, 4)
    for j in range(Q.shape[0]):
        sl = slice(int(lims[j]), int(lims[j + 1]))
        order = np.lexsort((ridx[sl], rdist[sl]))[:topk]
        assert np.array_equal(ridx[sl][order], idx[j]) and np.array_equal(rdist[sl][order], dist[j])


def test_mask_length_follows_a_second_add():
    import vq_amd

    rng = np.random.default_rng(6)
    d = 70
    coarse, lists, rows, Q = _case(rng, d, 5)
    words = B.pack(B.bits_f32(rows, BQ[0]))
    half = N // 2
    ix = _index(coarse, B.SQ, lists[:half], words[:half])
    m1 = rng.random(half) < 0.3
    _same(ix.filtered_search(Q, m1, 10, 3), S.ivf_search(B.SQ, CM, coarse, lists[:half], BQ, words[:half], d, Q, 3, 10, m1))
    ix.add_packed(lists[half:], words[half:])
    with pytest.raises(vq_amd.DimensionMismatch):
        ix.filtered_search(Q, m1, 10, 3)
    m2 = rng.random(N) < 0.3
    _same(ix.filtered_search(Q, m2, 10, 3), S.ivf_search(B.SQ, CM, coarse, lists, BQ, words, d, Q, 3, 10, m2))
    _same_range(ix.filtered_hamming_range_search(Q, d // 2, m2, 3),
                S.ivf_range_search(B.SQ, CM, coarse, lists, BQ, words, d, Q, 3, d // 2, m2))
    _same(ix.search(Q, 10, 3), S.ivf_search(B.SQ, CM, coarse, lists, BQ, words, d, Q, 3, 10, np.ones(N, bool)))


def test_rerank_with_fewer_allowed_rows_than_candidates():
    import vq_amd

    rng = np.random.default_rng(10)
    d = 40
    coarse, lists, rows, Q = _case(rng, d, 5)
    ix = _index(coarse, B.MAN, lists, B.pack(B.bits_f32(rows, 0.0)), (0.0, 0, 1))
    flat = vq_amd.FlatIndex(rows)
    for allowed in (6, 25, 700):
        m = np.zeros(N, bool)
        m[rng.choice(N, allowed, replace=False)] = True
        idx, dist = ix.filtered_search(Q, m, 10, NLIST, rerank=flat, candidates=40)
        first, _ = ix.filtered_search(Q, m, 40, NLIST)
        for j in range(Q.shape[0]):
            cand = first[j][first[j] != 0xFFFFFFFF]
            k = min(10, cand.size)
            wi, wd = flat.rerank(Q[j:j + 1], cand[None, :], k)
            assert np.array_equal(idx[j, :k], wi[0]) and np.array_equal(dist[j, :k].view(np.uint32), wd[0].view(np.uint32))
            assert (idx[j, k:] == 0xFFFFFFFF).all() and np.isposinf(dist[j, k:]).all()
            assert m[idx[j, :k]].all()


@pytest.mark.parametrize("off", [1, 3])
def test_device_forms_at_offset_pointers(off):
    import torch

    rng = np.random.default_rng(off)
    d, nq, topk, nprobe = 128, 9, 17, 3
    coarse, lists, rows, Q = _case(rng, d, nq)
    words = B.pack(B.bits_f32(rows, BQ[0]))
    m = rng.random(N) < 0.3
    m[64:256] = False
    w = S.pack(m)
    dev = torch.device("cuda:0")
    qb = torch.zeros(nq * d + off + 8, dtype=torch.float32, device=dev)
    qb[off:off + nq * d] = torch.from_numpy(Q.ravel()).to(dev)
    mb = torch.full((w.size + off + 8,), -1, dtype=torch.int32, device=dev)  # all ones around the mask
    mb[off:off + w.size] = torch.from_numpy(w.view(np.int32)).to(dev)
    ib = torch.full((nq * topk + off + 8,), 7, dtype=torch.int32, device=dev)
    db = torch.full((nq * topk + off + 8,), -1.0, dtype=torch.float32, device=dev)
    ix = _index(coarse, B.EUC, lists, words)
    ix.filtered_search_device(qb.data_ptr() + 4 * off, nq, topk, ib.data_ptr() + 4 * off, db.data_ptr() + 4 * off,
                              mb.data_ptr() + 4 * off, nprobe)
    torch.cuda.synchronize()
    gi, gd = ib.cpu().numpy(), db.cpu().numpy()
    _same((gi[off:off + nq * topk].view(np.uint32).reshape(nq, topk), gd[off:off + nq * topk].reshape(nq, topk)),
          S.ivf_search(B.EUC, CM, coarse, lists, BQ, words, d, Q, nprobe, topk, m))
    assert (gi[:off] == 7).all() and (gi[off + nq * topk:] == 7).all()
    assert (gd[:off] == -1.0).all() and (gd[off + nq * topk:] == -1.0).all()
    res = ix.filtered_hamming_range_search_device(qb.data_ptr() + 4 * off, nq, d // 2 - 5, mb.data_ptr() + 4 * off, nprobe)
    _same_range(res.read(), S.ivf_range_search(B.EUC, CM, coarse, lists, BQ, words, d, Q, nprobe, d // 2 - 5, m))
    assert (mb.cpu().numpy()[off:off + w.size].view(np.uint32) == w).all()


@pytest.mark.parametrize("seed", range(20))
def test_seeded_draws(seed):
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(1, 3001))
    d = int(rng.integers(1, 1201))
    nlist = int(rng.integers(1, 40))
    nprobe = int(rng.integers(1, nlist + 1))
    metric = int(rng.integers(0, 3))
    p = float(rng.choice([0.0, 0.01, 0.1, 0.5, 0.9, 1.0]))
    topk = int(rng.integers(1, min(n, 1024) + 1))
    nq = int(rng.integers(1, 60))
    radius = rng.integers(0, d + 2, nq).astype(np.uint32)
    coarse = rng.standard_normal((nlist, d)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    rows = rng.standard_normal((n, d)).astype(F)
    Q = rng.standard_normal((nq, d)).astype(F)
    m = rng.random(n) < p
    words = B.pack(B.bits_f32(rows, BQ[0]))
    ix = _index(coarse, metric, lists, words)
    what = f"n {n} d {d} nlist {nlist} nprobe {nprobe} metric {metric} p {p} topk {topk} nq {nq}"
    _same(ix.filtered_search(Q, m, topk, nprobe), S.ivf_search(metric, CM, coarse, lists, BQ, words, d, Q, nprobe, topk, m), what)
    _same_range(ix.filtered_hamming_range_search(Q, radius, m, nprobe),
                S.ivf_range_search(metric, CM, coarse, lists, BQ, words, d, Q, nprobe, radius, m), what)
