"""The inverted-file 4-bit scalar index on the MI355X (vq_amd.IVFScalar4Index, vqhip_ivfsq4_*, vq_amd/csrc/k_ivfsq4.hip: the
two distance kernels of ivf_tile.hpp over the row source NibbleRows of nibble_decode.hpp).  Every comparison is equality
of indices and of distance bits, for search, search(allowed=), range_search, range_search(allowed=) and search(rerank=):
  identity 1  against IVFScalarIndex over the same codes, one byte each, in the same lists, at every nprobe and topk;
  identity 2  against IVFFlatIndex over quantizer.dequantize_batch(codes) in the same lists;
  identity 3  at nprobe == nlist against Scalar4Index.from_codes(codes) on the same call;
  identity 4  after adds interleaved with remove_rows against a fresh index given the remaining rows in one add;
and against the numpy statement (tests/ref_ivfsq4.py).  n <= 1501; nlist 1 / 4 / 7 with one list empty; dim 1, 7, 8, 9 (a
word, its ends), 31, 32, 33 (the 32-dimension chunk of the tile), 40, 100 and 1100 (the scan kernel re-stages the query
past 1024 dimensions, and the last word holds four of them); 1, 3 and 129 queries; the quantizers of tests/ref_sq4.py;
five metrics; codes >= levels, rows of zero codes, duplicates across lists; NaN, +-inf and -0.0 in the queries."""
import numpy as np
import pytest

import ref_ivfsq4 as R
import ref_knn as K
import ref_sq4 as S4

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["squared_euclidean", "euclidean", "manhattan", "cosine", "cosine_unclamped"]
DIMS = [1, 7, 8, 9, 31, 32, 33, 40, 100, 1100]
NLISTS = [1, 4, 7]
NQS = [1, 3, 129]
EMPTY = 2  # the list without rows (where there is more than one list)


def _same(got, want, what=""):
    """search results (idx, dist) or range results (lims, idx, dist): equal arrays, the distances as bits"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = np.argwhere(gv != wv)
        assert bad.size == 0, f"{what}: first mismatch at {bad[0]}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def _case(seed, n, nlist, dim, nq, sq):
    """codes over every nibble value (codes >= levels occur), rows of zero codes, duplicates in one list and across lists,
    rows in an order unrelated to their lists, list EMPTY without rows; the centroids and most queries lie in the
    quantizer's range; queries with NaN, +inf, -inf and -0.0 where there are enough of them"""
    rng = np.random.default_rng(seed)
    lo, hi = float(sq[0]), float(sq[1])
    coarse = rng.uniform(lo, hi, (nlist, dim)).astype(F)
    lists = rng.integers(0, nlist, n).astype(np.uint32)
    if nlist > 1:
        lists[lists == EMPTY] = (EMPTY + 1) % nlist
    codes = rng.integers(0, 16, (n, dim)).astype(np.uint8)
    codes[3] = 0
    codes[n // 3] = 0
    codes[n - 7:] = codes[10:17]  # duplicate rows ...
    lists[n - 7:n - 3] = lists[10:14]  # ... four in the same lists: ties by row id
    lists[n - 3:] = (lists[14:17] + 3) % nlist  # ... three across lists
    if nlist > 1:
        lists[lists == EMPTY] = (EMPTY + 1) % nlist
    Q = rng.uniform(lo, hi, (nq, dim)).astype(F)
    Q[0] = coarse[min(3, nlist - 1)]
    if nq >= 3:
        Q[1, 0] = -0.0
        Q[2, dim // 2] = np.nan
    if nq >= 129:
        Q[5, 0], Q[6, dim - 1], Q[7] = np.inf, -np.inf, 0.0
        Q[8, dim - 1] = np.nan
    return coarse, lists, codes, Q


def _quantizer(sq):
    import vq_amd

    return vq_amd.ScalarQuantizer(*sq)


def _index(coarse, metric, lists, codes, sq, pieces=1, packed=False):
    import vq_amd

    ix = vq_amd.IVFScalar4Index(coarse, _quantizer(sq), vq_amd.Distance(NAMES[metric]))
    for j, a in enumerate(np.array_split(np.arange(len(lists)), pieces)):
        if packed or j % 2:
            ix.add_packed(lists[a], S4.pack4(codes[a]))
        else:
            ix.add_codes(lists[a], codes[a])
    return ix


def _sq8(coarse, metric, lists, codes, sq):
    import vq_amd

    ix = vq_amd.IVFScalarIndex(coarse, _quantizer(sq), vq_amd.Distance(NAMES[metric]))
    ix.add_codes(lists, codes)
    return ix


def _flat(coarse, metric, lists, codes, sq):
    import vq_amd

    ix = vq_amd.IVFFlatIndex(coarse, vq_amd.Distance(NAMES[metric]))
    ix.add_rows(lists, _quantizer(sq).dequantize_batch(codes))
    return ix


def _radii(dist, col):
    """one radius per query from a reference search's distances: the one in column `col` (so that about `col + 1` rows hit),
    1.0 where that is no finite number"""
    r = dist[:, min(col, dist.shape[1] - 1)].copy()
    r[~np.isfinite(r)] = 1.0
    return r


def _masks(n, seed):
    """all, none but one, a block, random"""
    rng = np.random.default_rng(seed)
    one = np.zeros(n, bool)
    one[n - 5] = True  # (one of the duplicated rows)
    block = np.zeros(n, bool)
    block[n // 4:n // 4 + 70] = True
    return {"all": np.ones(n, bool), "one": one, "block": block, "random": rng.random(n) < 0.4}


def _hold_to(ix, ref, Q, nprobes, topks, masks, what):
    """the four calls on ix against the same calls on the reference index (IVFScalarIndex or IVFFlatIndex over the same
    rows in the same lists): every nprobe and topk; the radii come from the reference's distances"""
    with np.errstate(all="ignore"):
        for nprobe in nprobes:
            assert np.array_equal(ix.probe(Q, nprobe), ref.probe(Q, nprobe)), f"{what}: probe at nprobe {nprobe}"
            for topk in topks:
                want = ref.search(Q, topk=topk, nprobe=nprobe)
                _same(ix.search(Q, topk=topk, nprobe=nprobe), want, f"{what}: search nprobe {nprobe} topk {topk}")
            radii = _radii(want[1], 9)  # (of the largest topk)
            _same(ix.range_search(Q, radii, nprobe=nprobe), ref.range_search(Q, radii, nprobe=nprobe), f"{what}: range nprobe {nprobe}")
            for name, m in masks.items():
                t = topks[len(topks) // 2]
                _same(ix.search(Q, topk=t, nprobe=nprobe, allowed=m), ref.search(Q, topk=t, nprobe=nprobe, allowed=m),
                      f"{what}: search nprobe {nprobe} mask {name}")
                _same(ix.range_search(Q, radii, nprobe=nprobe, allowed=m), ref.range_search(Q, radii, nprobe=nprobe, allowed=m),
                      f"{what}: range nprobe {nprobe} mask {name}")


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("di", range(len(DIMS)))
def test_identities_at_every_dim(di, metric):
    """identities 1, 2 and 3 for the four calls at every dim and metric; nlist, nq and the quantizer go round with them, so
    that each value meets every metric and several dims"""
    import vq_amd

    dim = DIMS[di]
    nlist, nq, sq = NLISTS[(di + metric) % 3], NQS[(di + 2 * metric) % 3], R.QUANTIZERS[(di + metric) % 4]
    n = 1501 if dim < 1000 else 700
    coarse, lists, codes, Q = _case(1000 * di + metric, n, nlist, dim, nq, sq)
    masks = _masks(n, di)
    nprobes = sorted({1, min(2, nlist), nlist})
    topks = [1, 4, min(n, 1024)]
    ix = _index(coarse, metric, lists, codes, sq, pieces=3)
    assert ix.list_sizes()[EMPTY if nlist > 1 else 0] == (0 if nlist > 1 else n)
    for make, what in ((_sq8, "IVFScalarIndex"), (_flat, "IVFFlatIndex")):
        ref = make(coarse, metric, lists, codes, sq)
        _hold_to(ix, ref, Q, nprobes, topks, masks if make is _sq8 else {"random": masks["random"]}, what)
        ref.close()
    s4 = vq_amd.Scalar4Index.from_codes(codes, ix.quantizer, ix.distance)
    with np.errstate(all="ignore"):
        for topk in topks:
            want = s4.search(Q, topk)
            _same(ix.search(Q, topk=topk, nprobe=nlist), want, f"Scalar4Index: search topk {topk}")
        radii = _radii(want[1], 9)
        _same(ix.range_search(Q, radii, nprobe=nlist), s4.range_search(Q, radii), "Scalar4Index: range")
        for name, m in masks.items():
            _same(ix.search(Q, topk=4, nprobe=nlist, allowed=m), s4.search(Q, 4, allowed=m), f"Scalar4Index: search mask {name}")
            _same(ix.range_search(Q, radii, nprobe=nlist, allowed=m), s4.range_search(Q, radii, allowed=m), f"Scalar4Index: range mask {name}")
    ix.close()


@pytest.mark.parametrize("sq", R.QUANTIZERS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("nlist", NLISTS)
def test_identity_1_at_every_nlist_nq_and_quantizer(nlist, nq, sq):
    """the four calls against IVFScalarIndex at dim 33 (a ragged last chunk and a last word of one dimension); the metric
    goes round"""
    metric = K.METRICS[(nlist + nq + R.QUANTIZERS.index(sq)) % 5]
    n = 1201
    coarse, lists, codes, Q = _case(nlist * 1000 + nq, n, nlist, 33, nq, sq)
    ix = _index(coarse, metric, lists, codes, sq, packed=True)
    ref = _sq8(coarse, metric, lists, codes, sq)
    _hold_to(ix, ref, Q, sorted({1, min(2, nlist), nlist}), [1, 4, 1024], _masks(n, nq), "IVFScalarIndex")
    ref.close()
    ix.close()


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("dim", [1, 9, 33, 40])
def test_the_four_calls_match_the_statement(dim, metric):
    """against numpy: the radii are distances the statement reports, so the hit counts are the statement's"""
    sq = R.QUANTIZERS[(dim + metric) % 4]
    n, nlist = 400, 4
    coarse, lists, codes, Q = _case(50 * dim + metric, n, nlist, dim, 3, sq)
    ix = _index(coarse, metric, lists, codes, sq, pieces=2)
    masks = _masks(n, dim)
    with np.errstate(all="ignore"):
        for nprobe in (1, 2, 4):
            want = R.search(metric, coarse, lists, sq, codes, Q, nprobe, 400)
            assert np.array_equal(ix.probe(Q, nprobe), R.probe(metric, coarse, Q, nprobe))
            for topk in (1, 4, 400):
                _same(ix.search(Q, topk=topk, nprobe=nprobe), (want[0][:, :topk], want[1][:, :topk]), f"search {nprobe} {topk}")
            radii = _radii(want[1], 20)
            lims, ri, rd = R.range_search(metric, coarse, lists, sq, codes, Q, nprobe, radii)
            _same(ix.range_search(Q, radii, nprobe=nprobe), (lims, ri, rd), f"range {nprobe}")
            if np.isfinite(want[1][0, 20]):
                assert int(lims[1]) >= 21  # Q[0] hits at least the rows the radius was taken from
            for name, m in masks.items():
                _same(ix.search(Q, topk=7, nprobe=nprobe, allowed=m), R.search_masked(metric, coarse, lists, sq, codes, Q, nprobe, 7, m),
                      f"search {nprobe} mask {name}")
                _same(ix.range_search(Q, radii, nprobe=nprobe, allowed=m),
                      R.range_search_masked(metric, coarse, lists, sq, codes, Q, nprobe, radii, m), f"range {nprobe} mask {name}")
    ix.close()


@pytest.mark.parametrize("dim", [33, 1100])
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 127, 128, 129])
def test_every_query_probes_the_same_list(nq, dim):
    """nq queries beside one centroid: its list is probed by all nq of them -- below 16 the scan kernel computes every pair,
    from 16 on the tile kernel, in one or two tiles of 128 queries.  Filtered too (the picked forms of both kernels)."""
    sq = R.QUANTIZERS[0]
    n = 900 if dim < 1000 else 300
    coarse, lists, codes, _ = _case(100 + nq, n, 7, dim, 1, sq)
    rng = np.random.default_rng(nq)
    Q = (coarse[5] + F(1e-3) * rng.standard_normal((nq, dim)).astype(F)).astype(F)
    ix = _index(coarse, K.EUCLIDEAN, lists, codes, sq)
    ref = _sq8(coarse, K.EUCLIDEAN, lists, codes, sq)
    P = ix.probe(Q, 1)
    assert np.all(P == 5)
    m = _masks(n, nq)["random"]
    want = ref.search(Q, topk=30, nprobe=1)
    _same(ix.search(Q, topk=30, nprobe=1), want)
    _same(ix.search(Q, topk=30, nprobe=1, allowed=m), ref.search(Q, topk=30, nprobe=1, allowed=m))
    radii = _radii(want[1], 9)
    _same(ix.range_search(Q, radii, nprobe=1), ref.range_search(Q, radii, nprobe=1))
    _same(ix.range_search(Q, radii, nprobe=1, allowed=m), ref.range_search(Q, radii, nprobe=1, allowed=m))
    ref.close()
    ix.close()


@pytest.mark.parametrize("dim", [9, 40, 1100])
def test_kernel_variants_give_the_same_bits(dim):
    """the same query alone (the scan kernel) and among 39 copies of itself (the tile kernel), unfiltered and filtered"""
    sq = R.QUANTIZERS[2]
    n = 1000 if dim < 1000 else 300
    coarse, lists, codes, Q = _case(77, n, 4, dim, 3, sq)
    m = _masks(n, 3)["random"]
    for metric in K.METRICS:
        ix = _index(coarse, metric, lists, codes, sq)
        for allowed in (None, m):
            alone = ix.search(Q[1:2], topk=200, nprobe=2, allowed=allowed)
            many = ix.search(np.repeat(Q[1:2], 40, axis=0), topk=200, nprobe=2, allowed=allowed)
            for j in range(40):
                _same((many[0][j:j + 1], many[1][j:j + 1]), alone, f"metric {metric} copy {j}")
        ix.close()


@pytest.mark.parametrize("nq", [3, 40])  # the scan kernel, the tile kernel
def test_list_lengths_around_the_row_tile(nq):
    """lists of 63, 64, 65, 1, 0 and 127 rows at dim 20 (three words a row): the runs start at any word"""
    sq = R.QUANTIZERS[1]
    sizes = [63, 64, 65, 1, 0, 127]
    lists = np.repeat(np.arange(6), sizes).astype(np.uint32)
    n = len(lists)
    rng = np.random.default_rng(31)
    coarse, _, codes, _ = _case(31, n, 6, 20, 1, sq)
    perm = rng.permutation(n)
    lists, codes = lists[perm], codes[perm]
    Q = np.repeat(coarse, nq, axis=0) + F(1e-3) * rng.standard_normal((6 * nq, 20)).astype(F)
    for metric in (K.SQUARED_EUCLIDEAN, K.COSINE):
        ix = _index(coarse, metric, lists, codes, sq)
        ref = _sq8(coarse, metric, lists, codes, sq)
        assert ix.list_sizes().tolist() == sizes
        for nprobe in (1, 2, 6):
            want = R.search(metric, coarse, lists, sq, codes, Q[::nq], nprobe, 70)
            got = ix.search(Q, topk=70, nprobe=nprobe)
            _same((got[0][::nq], got[1][::nq]), want)
            _same(got, ref.search(Q, topk=70, nprobe=nprobe))
        ref.close()
        ix.close()


def test_add_rows_encodes_and_packs_as_the_quantizer():
    import vq_amd

    sqp = R.QUANTIZERS[0]
    sq = _quantizer(sqp)
    coarse, lists, _, Q = _case(41, 1500, 7, 17, 3, sqp)
    rng = np.random.default_rng(41)
    rows = rng.uniform(-1.5, 1.5, (1500, 17)).astype(F)  # past both ends of [-1, 1]
    rows[5, 3], rows[6, 0], rows[7, 1] = np.nan, np.inf, -np.inf
    ix = vq_amd.IVFScalar4Index(coarse, sq, vq_amd.Distance.manhattan())
    assert np.array_equal(ix.add_rows(lists[:500], rows[:500]), np.arange(500))
    codes = sq.quantize_batch(rows)
    words = vq_amd.ScalarQuantizer.pack4_codes(codes)
    assert np.array_equal(ix.codes(), codes[:500]) and np.array_equal(ix.packed(), words[:500])
    want = _sq8(coarse, K.MANHATTAN, lists[:500], codes[:500], sqp).search(Q, topk=10, nprobe=3)
    _same(ix.search(Q, topk=10, nprobe=3), want)
    # an add after a search rebuilds the device state
    assert np.array_equal(ix.add_rows(lists[500:], rows[500:].astype(np.float64)), np.arange(500, 1500))
    assert np.array_equal(ix.packed(), words) and np.array_equal(ix.list_ids, lists)
    want = _sq8(coarse, K.MANHATTAN, lists, codes, sqp).search(Q, topk=10, nprobe=3)
    _same(ix.search(Q, topk=10, nprobe=3), want)
    ix.close()
    assert np.array_equal(ix.packed(), words)  # the words outlive the handle
    _same(ix.search(Q, topk=10, nprobe=3), want)
    ix.close()


def test_add_assigns_the_nearest_list():
    import vq_amd
    from vq_amd.ivf import _nearest_lists

    sqp = R.QUANTIZERS[1]
    sq = _quantizer(sqp)
    coarse, _, _, Q = _case(14, 1000, 7, 21, 3, sqp)
    rows = np.random.default_rng(14).uniform(0, 15, (1000, 21)).astype(F)
    ix = vq_amd.IVFScalar4Index(coarse, sq)
    assert np.array_equal(ix.add(rows), np.arange(1000))
    assert np.array_equal(ix.list_ids, _nearest_lists(coarse, rows, K.EUCLIDEAN))
    assert np.array_equal(ix.codes(), sq.quantize_batch(rows))
    _same(ix.search(Q[:2], topk=10, nprobe=7), vq_amd.Scalar4Index(rows, sq).search(Q[:2], 10))
    ix.close()


def _every_call(ix, Q, radii, mask):
    """what identity 4 compares: every call of the index at nprobe 2 and nlist"""
    out = [ix.list_sizes(), ix.list_ids, ix.codes(), ix.packed()]
    t = min(len(ix), 20)
    for nprobe in (2, ix.nlist):
        out.append(ix.probe(Q, nprobe))
        out += list(ix.search(Q, topk=t, nprobe=nprobe))
        out += list(ix.search(Q, topk=t, nprobe=nprobe, allowed=mask))
        out += list(ix.range_search(Q, radii, nprobe=nprobe))
        out += list(ix.range_search(Q, radii, nprobe=nprobe, allowed=mask))
    return tuple(out)


@pytest.mark.parametrize("metric", [K.EUCLIDEAN, K.COSINE])
@pytest.mark.parametrize("dim", [9, 100])
def test_adds_interleaved_with_removals_equal_a_fresh_index(dim, metric):
    """identity 4: `kept` is IVFScalarIndex.remove_rows'; a current device state stays current (uploads does not move);
    removing everything leaves an index that takes rows again"""
    sq = R.QUANTIZERS[2]
    n = 1200
    coarse, lists, codes, Q = _case(500 + dim + metric, n, 7, dim, 3, sq)
    rng = np.random.default_rng(dim)
    ix = _index(coarse, metric, lists[:800], codes[:800], sq)
    twin = _sq8(coarse, metric, lists[:800], codes[:800], sq)
    cur_l, cur_c = lists[:800], codes[:800]

    def check(what, uploads):
        fresh = _index(coarse, metric, cur_l, cur_c, sq)
        mask = np.random.default_rng(len(cur_l)).random(len(cur_l)) < 0.5
        with np.errstate(all="ignore"):
            radii = _radii(twin.search(Q, topk=min(len(cur_l), 20), nprobe=2)[1], 9)
            got, want = _every_call(ix, Q, radii, mask), _every_call(fresh, Q, radii, mask)
        _same(got, want, what)
        assert ix._ix.uploads() == uploads, f"{what}: uploads {ix._ix.uploads()}, want {uploads}"
        fresh.close()

    check("as added", 1)
    for step, (frac, more) in enumerate(((0.3, None), (0.05, slice(800, 1000)), (0.6, None), (0.0, slice(1000, 1200)), (0.5, None))):
        if more is not None:  # an add: the device state is no longer current, and the removal behind it is the host's
            ix.add_codes(lists[more], codes[more])
            twin.add_codes(lists[more], codes[more])
            cur_l, cur_c = np.concatenate([cur_l, lists[more]]), np.concatenate([cur_c, codes[more]])
        gone = rng.random(len(cur_l)) < frac
        gone[0] = frac > 0
        before = ix._ix.uploads()
        kept = ix.remove_rows(gone)
        assert np.array_equal(kept, twin.remove_rows(gone)) and np.array_equal(kept, np.flatnonzero(~gone))
        assert ix._ix.uploads() == before  # a removal never uploads
        cur_l, cur_c = cur_l[kept], cur_c[kept]
        check(f"step {step}", before + (1 if more is not None else 0))
    # everything goes, on the device: the state stays current and empty
    before = ix._ix.uploads()
    assert ix.remove_rows(np.ones(len(ix), bool)).shape == (0,) and len(ix) == 0 and ix._ix.info()[0] == 0
    assert ix._ix.uploads() == before and not ix.list_sizes().any()
    lims, ri, _ = ix.range_search(Q, 1e30, nprobe=7)
    assert not lims.any() and ri.size == 0
    ix.add_packed(lists[:50], S4.pack4(codes[:50]))
    cur_l, cur_c = lists[:50], codes[:50]
    twin.remove_rows(np.ones(len(twin), bool))
    twin.add_codes(cur_l, cur_c)
    check("after removing everything", before + 1)
    twin.close()
    ix.close()


def test_device_forms_at_a_pointer_that_is_not_16_byte_aligned():
    torch = pytest.importorskip("torch")
    from vq_amd import _lib, pack_row_mask

    sq = R.QUANTIZERS[0]
    n, nq, dim = 1300, 33, 40
    coarse, lists, codes, Q = _case(15, n, 7, dim, nq, sq)
    ix = _index(coarse, K.COSINE, lists, codes, sq)
    mask = _masks(n, 15)["random"]
    buf = torch.zeros(nq * dim + 1, dtype=torch.float32, device="cuda")
    dq = buf[1:]
    dq.copy_(torch.from_numpy(Q.reshape(-1)))
    assert dq.data_ptr() % 16 == 4
    dm = torch.from_numpy(pack_row_mask(mask, n).view(np.int32)).cuda()
    for allowed, dev_allowed in ((None, None), (mask, dm.data_ptr())):
        host = ix.search(Q, topk=15, nprobe=3, allowed=allowed)
        di = torch.empty((nq, 15), dtype=torch.int32, device="cuda")
        dd = torch.empty((nq, 15), dtype=torch.float32, device="cuda")
        ix.search_device(dq.data_ptr(), nq, 15, di.data_ptr(), dd.data_ptr(), nprobe=3, dev_allowed=dev_allowed)
        torch.cuda.synchronize()
        _lib.synchronize()
        _same((di.cpu().numpy().view(np.uint32), dd.cpu().numpy()), host)
        radii = _radii(host[1], 9)
        _same(ix.range_search_device(dq.data_ptr(), nq, radii, nprobe=3, dev_allowed=dev_allowed).read(),
              ix.range_search(Q, radii, nprobe=3, allowed=allowed))
    _same(ix.search(Q, topk=15, nprobe=3), _sq8(coarse, K.COSINE, lists, codes, sq).search(Q, topk=15, nprobe=3))
    ix.close()


@pytest.mark.parametrize("kind", ["flat", "scalar4"])
def test_rerank_with_an_exact_index(kind):
    """search(rerank=) equals IVFScalarIndex's with the same reranker (identity 1), and the reranker's own rerank of the
    first stage's real hits"""
    import vq_amd

    sq = R.QUANTIZERS[0]
    n = 1500
    coarse, lists, codes, Q = _case(17, n, 7, 24, 129, sq)
    ix = _index(coarse, K.EUCLIDEAN, lists, codes, sq)
    ref = _sq8(coarse, K.EUCLIDEAN, lists, codes, sq)
    rows = ix.quantizer.dequantize_batch(codes) + F(0.01) * np.random.default_rng(17).standard_normal((n, 24)).astype(F)
    exact = vq_amd.FlatIndex(rows) if kind == "flat" else vq_amd.Scalar4Index.from_codes(codes, _quantizer((-1.0, 1.0, 12)))
    mask = _masks(n, 17)["block"]
    with np.errstate(all="ignore"):
        for nprobe, cand in ((4, 40), (1, 20)):
            got = ix.search(Q, topk=10, nprobe=nprobe, rerank=exact, candidates=cand)
            _same(got, ref.search(Q, topk=10, nprobe=nprobe, rerank=exact, candidates=cand))
            _same(ix.search(Q, topk=10, nprobe=nprobe, rerank=exact, candidates=cand, allowed=mask),
                  ref.search(Q, topk=10, nprobe=nprobe, rerank=exact, candidates=cand, allowed=mask))
            hits = ix.search(Q, topk=cand, nprobe=nprobe)[0]
            for j in (0, 1, 2, 64, 128):
                real = hits[j][hits[j] != R.PAD_ID]
                t = min(10, real.size)
                if t:
                    _same((got[0][j:j + 1, :t], got[1][j:j + 1, :t]), exact.rerank(Q[j:j + 1], real[None, :], t))
                assert np.all(got[0][j, t:] == R.PAD_ID) and np.isposinf(got[1][j, t:]).all()
    ref.close()
    ix.close()


def test_save_load_gives_the_same_search(tmp_path):
    import vq_amd

    sq = R.QUANTIZERS[3]
    coarse, lists, codes, Q = _case(19, 1400, 7, 31, 3, sq)
    ix = _index(coarse, K.COSINE_UNCLAMPED, lists, codes, sq, pieces=2)
    with np.errstate(all="ignore"):
        want = ix.search(Q, topk=12, nprobe=3)
        ix.save(tmp_path / "ix.bin")  # (with the handle open: the words come from it)
        back = vq_amd.IVFScalar4Index.load(tmp_path / "ix.bin")
        _same(back.search(Q, topk=12, nprobe=3), want)
        _same(want, R.search(K.COSINE_UNCLAMPED, coarse, lists, sq, codes, Q, 3, 12))
    ix.close()
    back.close()


def test_two_runs_give_the_same_arrays():
    sq = R.QUANTIZERS[0]
    coarse, lists, codes, Q = _case(23, 1501, 7, 40, 129, sq)
    codes[200:700] = codes[5]  # heavy ties
    ix = _index(coarse, K.COSINE, lists, codes, sq)
    m = _masks(1501, 23)["random"]
    with np.errstate(all="ignore"):
        a = ix.search(Q, topk=50, nprobe=4) + ix.search(Q, topk=50, nprobe=4, allowed=m) + ix.range_search(Q, 0.2, nprobe=4)
        b = ix.search(Q, topk=50, nprobe=4) + ix.search(Q, topk=50, nprobe=4, allowed=m) + ix.range_search(Q, 0.2, nprobe=4)
        _same(a, b)
        ix.close()
        ix2 = _index(coarse, K.COSINE, lists, codes, sq, packed=True)
        _same(ix2.search(Q, topk=50, nprobe=4) + ix2.search(Q, topk=50, nprobe=4, allowed=m) + ix2.range_search(Q, 0.2, nprobe=4), a)
    ix2.close()
