"""Randomised sweep of the eight search indexes on the MI355X against their numpy statements: FlatIndex, ScalarIndex,
BinaryIndex, PQIndex.search, IVFPQIndex (plain and residual), IVFFlatIndex, IVFScalarIndex and IVFBinaryIndex.  A case
(tests/fuzz_search_draws.py) is an index kind, a metric, data, queries and a drawn sequence of adds, searches, range
searches, close(), save / load and rerank=; after every search the result must be the statement's over the rows added so
far: indices equal, distances equal as uint32 bits, padding exactly 0xFFFFFFFF / +inf, range results equal in order and
offsets.  No tolerance, no skip: a drawn case is a valid call, so an error return is a finding.  A failure carries the
whole case in one line; `draw(family, seed)` rebuilds it.  VQ_FUZZ_SCALE=4 for a long hunt.

test_fuzz_<family>_filtered runs the same cases under `draw_filtered`'s ops: the filtered searches, range searches and
reranks and the Hamming-radius range searches, every filtered call with a mask of its own over the rows present, handed
over as bools, as words, as packed ids or as words with the bits past the rows set, some directly after close() or
save / load.  Beyond the statement, each filtered call is held to: no masked-out row returned, padding exactly behind the
allowed rows in reach, the unfiltered search of the same handle unchanged directly after, the unfiltered call under an
all-ones mask, the resident twin under the same mask at nprobe == nlist, and a range result against the filtered top-k of
its own hit count."""
import os

import numpy as np
import pytest

import fuzz_search_draws as D

pytestmark = pytest.mark.gpu
F = np.float32
SCALE = int(os.environ.get("VQ_FUZZ_SCALE", "1"))
PAD_ID = np.uint32(0xFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)


def _same(got, want):
    """(the helper of the indexes' own test files)"""
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    bad = np.argwhere(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[tuple(bad[0])]} != {wi[tuple(bad[0])]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _assert_same(got, want):
    """(the helper of tests/test_gpu_range.py and tests/test_gpu_ivf_range.py)"""
    gl, gi, gd = got
    wl, wi, wd = want
    assert gl.dtype == np.uint64 and gi.dtype == np.uint32 and gd.dtype == F
    assert gl.shape == wl.shape and np.array_equal(gl, wl), f"lims differ: {gl[:8]} != {wl[:8]}"
    assert gi.shape == wi.shape
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"first index mismatch at {bad[0]}: {gi[bad[0]]} != {wi[bad[0]]}"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def _padding(case, got, rows):
    """slots past the rows of a query's probed lists: exactly 0xFFFFFFFF / +inf, and none before"""
    idx, dist = got
    real = np.minimum(rows, idx.shape[1])
    pad = np.arange(idx.shape[1])[None, :] >= real[:, None]
    assert (idx[pad] == PAD_ID).all() and (dist.view(np.uint32)[pad] == INF_BITS).all(), "padding slots"
    assert (idx[~pad] != PAD_ID).all(), "a padding id among the real hits"


def _distance(metric):
    import vq_amd

    return vq_amd.Distance(D.NAMES[metric])


def _build(case):
    """the case's index: a resident kind over its rows, an IVF kind without rows yet"""
    import vq_amd
    from vq_amd.store import PQIndex

    c, d, dist = case.ctor, case.data, _distance(case.metric)
    fam = case.family
    if fam == "flat":
        return vq_amd.FlatIndex(d["stored"], dist)
    if fam == "scalar":
        q = vq_amd.ScalarQuantizer(*c["sq"])
        return vq_amd.ScalarIndex(d["rows"], q, dist) if c["source"] == "rows" else vq_amd.ScalarIndex.from_codes(d["codes"], q, dist)
    if fam == "binary":
        q = vq_amd.BinaryQuantizer(*c["bq"])
        if c["source"] == "rows":
            return vq_amd.BinaryIndex(d["rows"], q, dist)
        if c["source"] == "codes":
            return vq_amd.BinaryIndex.from_codes(d["bq_codes"], q, dist)
        return vq_amd.BinaryIndex.from_packed(d["words"], case.dim, q, dist)
    if fam == "pq":
        return PQIndex(d["codebooks"], d["codes"], dist)
    if fam == "ivfpq":
        return vq_amd.IVFPQIndex(d["coarse"], d["codebooks"], dist, residual=c["residual"])
    if fam == "ivfflat":
        return vq_amd.IVFFlatIndex(d["coarse"], dist, np.dtype(c["dtype"]))
    if fam == "ivfsq":
        return vq_amd.IVFScalarIndex(d["coarse"], vq_amd.ScalarQuantizer(*c["sq"]), dist)
    if fam == "ivfbin":
        return vq_amd.IVFBinaryIndex(d["coarse"], vq_amd.BinaryQuantizer(*c["bq"]), dist, _distance(case.coarse_metric))
    raise ValueError(fam)


def _twin(case, n):
    """the resident index over the first n rows of an IVF case (nprobe == nlist: the same results)"""
    import vq_amd
    from vq_amd.store import PQIndex

    c, d, dist = case.ctor, case.data, _distance(case.metric)
    if case.family == "ivfflat":
        return vq_amd.FlatIndex(d["stored"][:n], dist)
    if case.family == "ivfsq":
        return vq_amd.ScalarIndex.from_codes(d["codes"][:n], vq_amd.ScalarQuantizer(*c["sq"]), dist)
    if case.family == "ivfbin":
        return vq_amd.BinaryIndex.from_packed(d["words"][:n], case.dim, vq_amd.BinaryQuantizer(*c["bq"]), dist)
    if case.family == "ivfpq" and not c["residual"]:
        return PQIndex(d["codebooks"], d["codes"][:n], dist)
    return None


def _add(case, ix, op):
    d = case.data
    a = slice(op["lo"], op["n"])
    payload = {("ivfpq", "add_codes"): "codes", ("ivfflat", "add_rows"): "stored", ("ivfsq", "add_codes"): "codes",
               ("ivfsq", "add_rows"): "rows", ("ivfbin", "add_packed"): "words", ("ivfbin", "add_codes"): "bq_codes",
               ("ivfbin", "add_rows"): "rows"}[(case.family, op["how"])]
    ids = getattr(ix, op["how"])(d["lists"][a], d[payload][a])
    assert np.array_equal(ids, np.arange(op["lo"], op["n"], dtype=np.uint32)), "row ids of the add"


def _load(case, path):
    import vq_amd
    from vq_amd.store import PQIndex

    cls = {"scalar": vq_amd.ScalarIndex, "binary": vq_amd.BinaryIndex, "pq": PQIndex, "ivfpq": vq_amd.IVFPQIndex,
           "ivfflat": vq_amd.IVFFlatIndex, "ivfsq": vq_amd.IVFScalarIndex, "ivfbin": vq_amd.IVFBinaryIndex}[case.family]
    return cls.load(path)


def _close(ix):
    if hasattr(ix, "close"):
        ix.close()


RESIDENT = {"ivfflat": "flat", "ivfsq": "scalar", "ivfbin": "binary", "ivfpq": "pq"}  # the family of an IVF case's _twin


def _allowed_arg(op):
    """the mask of a filtered op in the form the draw chose for it"""
    import vq_amd

    mask, n = op["mask"], op["n"]
    if op["form"] == "bool":
        return mask.copy()
    if op["form"] == "ids":
        return vq_amd.pack_row_mask(op["ids"], n)
    words = vq_amd.pack_row_mask(mask, n)
    if op["form"] == "words_tail" and n % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # the bits past the rows: ignored
    assert np.array_equal(np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(np.bool_), mask)
    return words


def _filtered_search(family, index, Q, topk, allowed, kw, **rerank):
    if family in ("binary", "ivfbin"):
        return index.filtered_search(Q, allowed, topk, **kw, **rerank)
    if family == "ivfpq":
        return index.masked_search(Q, allowed, topk, **kw, **rerank)
    return index.search(Q, topk, **kw, allowed=allowed, **rerank)


def _filtered_range(index, Q, op, allowed, kw):
    if "hradius" in op:
        return index.filtered_hamming_range_search(Q, op["hradius"], allowed, **kw)
    return index.range_search(Q, op["radius"], **kw, allowed=allowed)


def _range(index, Q, op, kw):
    if "hradius" in op:
        return index.hamming_range_search(Q, op["hradius"], **kw)
    return index.range_search(Q, op["radius"], **kw)


def _only_allowed(idx, mask):
    real = idx[idx != PAD_ID].astype(np.int64)
    assert real.size == 0 or int(real.max()) < mask.shape[0], f"row id {int(real.max())} past the {mask.shape[0]} rows"
    out = real[~mask[real]]
    assert out.size == 0, f"{out.size} masked-out rows returned, the first: row {out[0]}"


def _new_op(case, ix, op, kw, want, path):
    """one op of fuzz_search_draws.NEW_OPS on the handle `ix`"""
    import vq_amd

    family, Q, name, n = case.family, case.queries, op["op"], op["n"]
    ivf = family in D.IVF
    topk = op.get("topk", min(case.topk, n))
    twin = _twin(case, n) if ivf and case.nprobe == case.nlist else None  # all lists probed: the resident index

    def unfiltered_search_is_unchanged(index):
        got = index.search(Q, topk, **kw)
        _same(got, want(n, topk))
        if ivf:
            _padding(case, got, D.probed_rows(case, n))

    if name == "hamming_range_search":
        got = ix.hamming_range_search(Q, op["hradius"], **kw)
        _assert_same(got, D.statement_hamming_range(case, n, op["hradius"]))
        if twin is not None:
            _assert_same(twin.hamming_range_search(Q, op["hradius"]), got)
        unfiltered_search_is_unchanged(ix)
        return

    mask, allowed = op["mask"], _allowed_arg(op)
    reach = D.allowed_in_reach(case, n, mask)
    index = ix
    if op.get("after_close"):
        ix.close()
    elif op.get("after_load"):
        ix.save(path)
        index = _load(case, path)
        assert len(index) == n
    try:  # (the filtered call is the first the fresh handle sees)
        if name == "filtered_search":
            got = _filtered_search(family, index, Q, topk, allowed, kw)
            _only_allowed(got[0], mask)
            _same(got, D.statement_filtered_search(case, n, topk, mask))
            _padding(case, got, reach)
            if mask.all():
                _same(got, index.search(Q, topk, **kw))
            if twin is not None:
                _same(_filtered_search(RESIDENT[family], twin, Q, topk, allowed, {}), got)
        elif name == "filtered_rerank_search":
            exact = vq_amd.FlatIndex(D.rerank_rows(case, n), _distance(op["flat_metric"]))
            rerank = {"rerank": exact, "candidates": op["candidates"]}
            got = _filtered_search(family, index, Q, topk, allowed, kw, **rerank)
            short = D.statement_filtered_search(case, n, op["candidates"], mask)  # the short list: the filtered statement ...
            first = _filtered_search(family, index, Q, op["candidates"], allowed, kw)
            _only_allowed(first[0], mask)
            _same(first, short)
            _padding(case, first, reach)
            _only_allowed(got[0], mask)
            _same(got, D.statement_rerank(case, n, short[0], topk, op["flat_metric"]))  # ... reranked exactly
            _padding(case, got, reach)
            if mask.all():
                _same(got, index.search(Q, topk, **kw, **rerank))
        else:  # filtered_range_search, filtered_hamming_range_search
            got = _filtered_range(index, Q, op, allowed, kw)
            _only_allowed(got[1], mask)
            if "hradius" in op:
                _assert_same(got, D.statement_hamming_range(case, n, op["hradius"], mask))
            else:
                _assert_same(got, D.statement_filtered_range(case, n, op["radius"], mask))
            if mask.all():
                _assert_same(got, _range(index, Q, op, kw))
            if twin is not None:
                _assert_same(_filtered_range(twin, Q, op, allowed, {}), got)
            lims = got[0].astype(np.int64)
            for j in np.flatnonzero((np.diff(lims) >= 1) & (np.diff(lims) <= 1024)):  # range and top-k agree
                a, b = lims[j], lims[j + 1]
                ti, td = _filtered_search(family, index, Q[j:j + 1], int(b - a), allowed, kw)
                assert np.array_equal(np.sort(ti[0]), got[1][a:b]), f"query {j}: the top {b - a} are not its {b - a} range hits"
                assert np.array_equal(np.sort(td[0].view(np.uint32)), np.sort(got[2][a:b].view(np.uint32))), \
                    f"query {j}: top-k and range distances differ"
        unfiltered_search_is_unchanged(index)  # a masked call leaves nothing behind
    finally:
        if index is not ix:
            _close(index)


def _run(family, seed, tmp_path, filtered=False):
    case = (D.draw_filtered if filtered else D.draw)(family, seed)
    ivf = family in D.IVF
    Q = case.queries
    kw = {"nprobe": case.nprobe} if ivf else {}
    ix = _build(case)
    wants = {}

    def want(n, topk):
        if (n, topk) not in wants:
            wants[n, topk] = D.statement_search(case, n, topk)
        return wants[n, topk]

    def checked_search(index, op):
        got = index.search(Q, op["topk"], **kw)
        _same(got, want(op["n"], op["topk"]))
        if ivf:
            _padding(case, got, D.probed_rows(case, op["n"]))
        return got

    step = -1
    try:
        for step, op in enumerate(case.ops):
            name, n = op["op"], op["n"]
            if name == "add":
                _add(case, ix, op)
                assert len(ix) == n
            elif name == "search":
                got = checked_search(ix, op)
                twin = _twin(case, n) if ivf and case.nprobe == case.nlist else None
                if twin is not None:  # all lists probed: the resident index over the same rows
                    _same(twin.search(Q, op["topk"]), got)
            elif name == "range_search":
                got = ix.range_search(Q, op["radius"], **kw)
                _assert_same(got, D.statement_range(case, n, op["radius"]))
                if ivf and case.nprobe == case.nlist:
                    _assert_same(_twin(case, n).range_search(Q, op["radius"]), got)
            elif name == "close_search":
                before = checked_search(ix, op)
                ix.close()
                _same(checked_search(ix, op), before)
            elif name == "save_load_search":
                before = checked_search(ix, op)
                path = tmp_path / f"{family}_{step}.bin"
                ix.save(path)
                back = _load(case, path)
                assert len(back) == n
                _same(checked_search(back, op), before)
                _close(back)
            elif name == "rerank_search":
                import vq_amd

                exact = vq_amd.FlatIndex(D.rerank_rows(case, n), _distance(op["flat_metric"]))
                got = ix.search(Q, op["topk"], rerank=exact, candidates=op["candidates"], **kw)
                short = want(n, op["candidates"])  # the short list is the statement's at topk = candidates ...
                _same(ix.search(Q, op["candidates"], **kw), short)
                _same(got, D.statement_rerank(case, n, short[0], op["topk"], op["flat_metric"]))  # ... reranked exactly
            elif filtered and name in D.NEW_OPS[family]:
                _new_op(case, ix, op, kw, want, tmp_path / f"{family}_{step}.bin")
            else:
                raise ValueError(name)
    except AssertionError as e:
        raise AssertionError(f"{case.describe(step)} :: {e}") from e
    finally:
        _close(ix)


@pytest.mark.parametrize("seed", D.seeds("flat", SCALE))
def test_fuzz_flat(seed, tmp_path):
    _run("flat", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("flat", SCALE))
def test_fuzz_flat_filtered(seed, tmp_path):
    _run("flat", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("scalar", SCALE))
def test_fuzz_scalar(seed, tmp_path):
    _run("scalar", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("scalar", SCALE))
def test_fuzz_scalar_filtered(seed, tmp_path):
    _run("scalar", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("binary", SCALE))
def test_fuzz_binary(seed, tmp_path):
    _run("binary", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("binary", SCALE))
def test_fuzz_binary_filtered(seed, tmp_path):
    _run("binary", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("pq", SCALE))
def test_fuzz_pq(seed, tmp_path):
    _run("pq", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("pq", SCALE))
def test_fuzz_pq_filtered(seed, tmp_path):
    _run("pq", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("ivfpq", SCALE))
def test_fuzz_ivfpq(seed, tmp_path):
    _run("ivfpq", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("ivfpq", SCALE))
def test_fuzz_ivfpq_filtered(seed, tmp_path):
    _run("ivfpq", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("ivfflat", SCALE))
def test_fuzz_ivfflat(seed, tmp_path):
    _run("ivfflat", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("ivfflat", SCALE))
def test_fuzz_ivfflat_filtered(seed, tmp_path):
    _run("ivfflat", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("ivfsq", SCALE))
def test_fuzz_ivfsq(seed, tmp_path):
    _run("ivfsq", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("ivfsq", SCALE))
def test_fuzz_ivfsq_filtered(seed, tmp_path):
    _run("ivfsq", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("ivfbin", SCALE))
def test_fuzz_ivfbin(seed, tmp_path):
    _run("ivfbin", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("ivfbin", SCALE))
def test_fuzz_ivfbin_filtered(seed, tmp_path):
    _run("ivfbin", seed, tmp_path, filtered=True)
