"""Randomised sweep of the eleven search indexes on the MI355X against their numpy statements: FlatIndex, ScalarIndex,
BinaryIndex, PQIndex.search, IVFPQIndex (plain and residual), IVFFlatIndex, IVFScalarIndex, IVFBinaryIndex,
AsymmetricBinaryIndex, Scalar4Index and IVFScalar4Index.  A case
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
its own hit count.

The three packed families are also held, one seed in four, to the identity their indexes claim: the 8-bit index over the
unpacked codes under the same quantizer (a FlatIndex over the decoded bits for AsymmetricBinaryIndex) returns the same
indices and distance bits.

test_fuzz_<family>_mutated runs the cases under `draw_mutated`'s ops, for the ten families that remove rows (every one but
pq): adds, remove_rows -- by bool mask or by shuffled ids with repeats -- and the family's query ops between them, some
removes directly before close() or save / load.  `remove_rows` must return ref_mutate.kept and len() must follow; every
query op is held to the family's statement over the rows present (`gathered`), row ids being positions among them; the
first query behind a remove is also held to a fresh index built over those rows, both searched at topk = min(n, 1024)
so that a wrong id of any row in reach shows, and with every list probed at a radius that takes every row, and
a FlatIndex reranker follows every add and remove with the same
argument."""
import os

import numpy as np
import pytest

import fuzz_search_draws as D
import ref_mutate as M

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


def _build(case, rows=None):
    """the case's index: a resident kind over its rows (its first `rows` ones), an IVF kind without rows yet"""
    import vq_amd
    from vq_amd.store import PQIndex

    c, dist = case.ctor, _distance(case.metric)
    d = case.data if rows is None else {k: (v[:rows] if k in D.PER_ROW else v) for k, v in case.data.items()}
    fam = case.family
    if fam == "flat":
        return vq_amd.FlatIndex(d["stored"], dist)
    if fam == "scalar":
        q = vq_amd.ScalarQuantizer(*c["sq"])
        return vq_amd.ScalarIndex(d["rows"], q, dist) if c["source"] == "rows" else vq_amd.ScalarIndex.from_codes(d["codes"], q, dist)
    if fam in ("binary", "abin"):
        cls = vq_amd.BinaryIndex if fam == "binary" else vq_amd.AsymmetricBinaryIndex
        q = vq_amd.BinaryQuantizer(*c["bq"])
        if c["source"] == "rows":
            return cls(d["rows"], q, dist)
        if c["source"] == "codes":
            return cls.from_codes(d["bq_codes"], q, dist)
        return cls.from_packed(d["words"], case.dim, q, dist)
    if fam == "sq4":
        q = vq_amd.ScalarQuantizer(*c["sq"])
        if c["source"] == "rows":
            return vq_amd.Scalar4Index(d["rows"], q, dist)
        if c["source"] == "codes":
            return vq_amd.Scalar4Index.from_codes(d["codes"], q, dist)
        return vq_amd.Scalar4Index.from_packed(d["words"], case.dim, q, dist)
    if fam == "ivfsq4":
        return vq_amd.IVFScalar4Index(d["coarse"], vq_amd.ScalarQuantizer(*c["sq"]), dist)
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
    if case.family == "ivfsq4":
        return vq_amd.Scalar4Index.from_packed(d["words"][:n], case.dim, vq_amd.ScalarQuantizer(*c["sq"]), dist)
    return None


def _eight_bit(case, n):
    """the index a packed family claims to equal bit for bit: the 8-bit one over the unpacked codes under the same
    quantizer; for AsymmetricBinaryIndex a FlatIndex over the decoded rows"""
    import vq_amd

    c, d, dist = case.ctor, case.data, _distance(case.metric)
    if case.family == "abin":
        return vq_amd.FlatIndex(D.decoded(case)[:n], dist)
    q = vq_amd.ScalarQuantizer(*c["sq"])
    if case.family == "sq4":
        return vq_amd.ScalarIndex.from_codes(d["codes"][:n], q, dist)
    ix = vq_amd.IVFScalarIndex(d["coarse"], q, dist)
    ix.add_codes(d["lists"][:n], d["codes"][:n])
    return ix


PAYLOAD = {("ivfpq", "add_codes"): "codes", ("ivfflat", "add_rows"): "stored", ("ivfsq", "add_codes"): "codes",
           ("ivfsq", "add_rows"): "rows", ("ivfbin", "add_packed"): "words", ("ivfbin", "add_codes"): "bq_codes",
           ("ivfbin", "add_rows"): "rows", ("ivfsq4", "add_rows"): "rows", ("ivfsq4", "add_codes"): "codes",
           ("ivfsq4", "add_packed"): "words",
           # the resident families (a mutated case):
           ("flat", "add"): "stored", ("scalar", "add"): "rows", ("scalar", "add_codes"): "codes", ("binary", "add"): "rows",
           ("binary", "add_codes"): "bq_codes", ("binary", "add_packed"): "words", ("abin", "add"): "rows",
           ("abin", "add_codes"): "bq_codes", ("abin", "add_packed"): "words", ("sq4", "add"): "rows",
           ("sq4", "add_codes"): "codes", ("sq4", "add_packed"): "words"}


def _add(case, ix, op):
    """an add op: draw's rows lo .. n - 1 keep their ids; a mutated case's rows lo .. hi - 1 arrive as ids at .. n - 1"""
    d = case.data
    a = slice(op["lo"], op.get("hi", op["n"]))
    payload = d[PAYLOAD[case.family, op["how"]]][a]
    ids = getattr(ix, op["how"])(d["lists"][a], payload) if case.family in D.IVF else getattr(ix, op["how"])(payload)
    assert np.array_equal(ids, np.arange(op.get("at", op["lo"]), op["n"], dtype=np.uint32)), "row ids of the add"


def _load(case, path):
    import vq_amd
    from vq_amd.store import PQIndex

    cls = {"scalar": vq_amd.ScalarIndex, "binary": vq_amd.BinaryIndex, "pq": PQIndex, "ivfpq": vq_amd.IVFPQIndex,
           "ivfflat": vq_amd.IVFFlatIndex, "ivfsq": vq_amd.IVFScalarIndex, "ivfbin": vq_amd.IVFBinaryIndex,
           "abin": vq_amd.AsymmetricBinaryIndex, "sq4": vq_amd.Scalar4Index, "ivfsq4": vq_amd.IVFScalar4Index}[case.family]
    return cls.load(path)


def _close(ix):
    if hasattr(ix, "close"):
        ix.close()


RESIDENT = {"ivfflat": "flat", "ivfsq": "scalar", "ivfbin": "binary", "ivfpq": "pq", "ivfsq4": "sq4"}  # an IVF case's _twin


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


def _exact(case, op, exact_of=None):
    """the FlatIndex a rerank op goes through: a fresh one over the case's rerank rows, or the one `exact_of` keeps"""
    import vq_amd

    if exact_of is not None:
        return exact_of(op)
    return vq_amd.FlatIndex(D.rerank_rows(case, op["n"]), _distance(op["flat_metric"]))


def _new_op(case, ix, op, kw, want, path, exact_of=None):
    """one op of fuzz_search_draws.NEW_OPS on the handle `ix`"""
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
            rerank = {"rerank": _exact(case, op, exact_of), "candidates": op["candidates"]}
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


def _wanted(case):
    """the search statement of `case`, each (n, topk) computed once"""
    wants = {}

    def want(n, topk):
        if (n, topk) not in wants:
            wants[n, topk] = D.statement_search(case, n, topk)
        return wants[n, topk]

    return want


def _query(case, ix, op, step, kw, want, tmp_path, filtered, exact_of=None):
    """one query op on the handle `ix`, held to `case`'s statements"""
    family, Q = case.family, case.queries
    ivf = family in D.IVF
    name, n = op["op"], op["n"]

    def checked_search(index, op):
        got = index.search(Q, op["topk"], **kw)
        _same(got, want(op["n"], op["topk"]))
        if ivf:
            _padding(case, got, D.probed_rows(case, op["n"]))
        return got

    if name == "search":
        got = checked_search(ix, op)
        twin = _twin(case, n) if ivf and case.nprobe == case.nlist else None
        if twin is not None:  # all lists probed: the resident index over the same rows
            _same(twin.search(Q, op["topk"]), got)
        if family in D.PACKED and case.seed % 4 == 0:  # the 8-bit index over the same codes: the same bits
            other = _eight_bit(case, n)
            _same(other.search(Q, op["topk"], **kw), got)
            _close(other)
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
        got = ix.search(Q, op["topk"], rerank=_exact(case, op, exact_of), candidates=op["candidates"], **kw)
        short = want(n, op["candidates"])  # the short list is the statement's at topk = candidates ...
        _same(ix.search(Q, op["candidates"], **kw), short)
        _same(got, D.statement_rerank(case, n, short[0], op["topk"], op["flat_metric"]))  # ... reranked exactly
    elif filtered and name in D.NEW_OPS[family]:
        _new_op(case, ix, op, kw, want, tmp_path / f"{family}_{step}.bin", exact_of)
    else:
        raise ValueError(name)


def _run(family, seed, tmp_path, filtered=False):
    case = (D.draw_filtered if filtered else D.draw)(family, seed)
    kw = {"nprobe": case.nprobe} if family in D.IVF else {}
    ix = _build(case)
    want = _wanted(case)
    step = -1
    try:
        for step, op in enumerate(case.ops):
            if op["op"] == "add":
                _add(case, ix, op)
                assert len(ix) == op["n"]
            else:
                _query(case, ix, op, step, kw, want, tmp_path, filtered)
    except AssertionError as e:
        raise AssertionError(f"{case.describe(step)} :: {e}") from e
    finally:
        _close(ix)


class _Reranker:
    """the FlatIndex a mutated case reranks through: it follows every add and every remove with the same argument (an
    index emptied by a removal of every row starts again at the next add)"""

    def __init__(self, case):
        ops = [o for o in case.ops if "flat_metric" in o]
        self.metric = ops[0]["flat_metric"] if ops else None  # (one flat metric a case: draw_mutated's)
        self.rows = np.ascontiguousarray(D.rerank_rows(case, case.n), F) if ops else None
        self.ix = None

    def add(self, lo, hi):
        import vq_amd

        if self.metric is None:
            return
        if self.ix is None:
            self.ix = vq_amd.FlatIndex(self.rows[lo:hi], _distance(self.metric))
        else:
            self.ix.add(self.rows[lo:hi])

    def remove(self, op):
        if self.ix is None:
            return
        if op["n"] == 0:
            self.ix = None
        else:
            kept = self.ix.remove_rows(op["arg"].copy())
            assert np.array_equal(kept, M.kept(op["n_before"], op["arg"])), "kept of the reranker's removal"

    def __call__(self, op):
        assert self.metric == op["flat_metric"] and len(self.ix) == op["n"]
        return self.ix


def _fresh(G):
    """a new index over the rows of the gathered case `G`: the family's own constructor, an IVF kind with one add"""
    ix = _build(G)
    if G.family in D.IVF:
        how = G.ctor["adds"][0]
        getattr(ix, how)(G.data["lists"], G.data[PAYLOAD[G.family, how]])
    return ix


def _every_id(G, ix, n):
    """the queries over every list at a radius that takes every row: the renumbered id of each row shows (IVFPQIndex has
    no range search: its top min(n, 1024))"""
    E = D.every_row(G)
    kw = {"nprobe": E.nprobe} if G.family in D.IVF else {}
    if "range_search" in D.QUERY_OPS[G.family]:
        radius = np.full(G.nq, np.inf, F)
        _assert_same(ix.range_search(E.queries, radius, **kw), D.statement_range(E, n, radius))
    elif G.family in ("binary", "ivfbin"):
        hradius = np.full(G.nq, G.dim + 7, np.int64)
        _assert_same(ix.hamming_range_search(E.queries, hradius, **kw), D.statement_hamming_range(E, n, hradius))
    else:
        _same(ix.search(E.queries, min(n, 1024), **kw), D.statement_search(E, n, min(n, 1024)))


def _run_mutated(family, seed, tmp_path):
    case = D.draw_mutated(family, seed)
    Q = case.queries
    ivf = family in D.IVF
    kw = {"nprobe": case.nprobe} if ivf else {}
    ix = _build(case, None if ivf else D.built_over(case))
    exact = _Reranker(case)
    if not ivf:
        exact.add(0, D.built_over(case))
    G = want = None       # the case over the rows present, and its search statement
    removed = False       # a remove since the last query op
    step = -1
    try:
        for step, op in enumerate(case.ops):
            name, n = op["op"], op["n"]
            if name == "add":
                _add(case, ix, op)
                exact.add(op["lo"], op["hi"])
                assert len(ix) == n
                G = None
                continue
            if name == "remove":
                kept = ix.remove_rows(op["arg"].copy())
                assert kept.dtype == np.uint32 and np.array_equal(kept, M.kept(op["n_before"], op["arg"])), "kept of the removal"
                assert len(ix) == n, f"len {len(ix)} behind the removal, not {n}"
                exact.remove(op)
                if op.get("then_close"):
                    ix.close()
                elif op.get("then_load"):
                    path = tmp_path / f"{family}_{step}.bin"
                    ix.save(path)
                    back = _load(case, path)
                    _close(ix)
                    ix = back
                    assert len(ix) == n
                G, removed = None, True
                continue
            if G is None:
                G = D.gathered(case, case.n, op["present"])
                want = _wanted(G)
            assert len(ix) == n == G.n
            if removed:  # a fresh index over the same rows answers the same, at a topk that shows every id it can
                topk = min(n, 1024)
                got = ix.search(Q, topk, **kw)
                _same(got, want(n, topk))
                fresh = _fresh(G)
                _same(fresh.search(Q, topk, **kw), got)
                _close(fresh)
                twin = _twin(G, n) if ivf and case.nprobe == case.nlist else None
                if twin is not None:
                    _same(twin.search(Q, topk), got)
                _every_id(G, ix, n)
                removed = False
            _query(G, ix, op, step, kw, want, tmp_path, True, exact)
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


@pytest.mark.parametrize("seed", D.seeds("abin", SCALE))
def test_fuzz_abin(seed, tmp_path):
    _run("abin", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("abin", SCALE))
def test_fuzz_abin_filtered(seed, tmp_path):
    _run("abin", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("sq4", SCALE))
def test_fuzz_sq4(seed, tmp_path):
    _run("sq4", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("sq4", SCALE))
def test_fuzz_sq4_filtered(seed, tmp_path):
    _run("sq4", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.seeds("ivfsq4", SCALE))
def test_fuzz_ivfsq4(seed, tmp_path):
    _run("ivfsq4", seed, tmp_path)


@pytest.mark.parametrize("seed", D.seeds("ivfsq4", SCALE))
def test_fuzz_ivfsq4_filtered(seed, tmp_path):
    _run("ivfsq4", seed, tmp_path, filtered=True)


@pytest.mark.parametrize("seed", D.mutated_seeds("flat", SCALE))
def test_fuzz_flat_mutated(seed, tmp_path):
    _run_mutated("flat", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("scalar", SCALE))
def test_fuzz_scalar_mutated(seed, tmp_path):
    _run_mutated("scalar", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("binary", SCALE))
def test_fuzz_binary_mutated(seed, tmp_path):
    _run_mutated("binary", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("ivfpq", SCALE))
def test_fuzz_ivfpq_mutated(seed, tmp_path):
    _run_mutated("ivfpq", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("ivfflat", SCALE))
def test_fuzz_ivfflat_mutated(seed, tmp_path):
    _run_mutated("ivfflat", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("ivfsq", SCALE))
def test_fuzz_ivfsq_mutated(seed, tmp_path):
    _run_mutated("ivfsq", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("ivfbin", SCALE))
def test_fuzz_ivfbin_mutated(seed, tmp_path):
    _run_mutated("ivfbin", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("abin", SCALE))
def test_fuzz_abin_mutated(seed, tmp_path):
    _run_mutated("abin", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("sq4", SCALE))
def test_fuzz_sq4_mutated(seed, tmp_path):
    _run_mutated("sq4", seed, tmp_path)


@pytest.mark.parametrize("seed", D.mutated_seeds("ivfsq4", SCALE))
def test_fuzz_ivfsq4_mutated(seed, tmp_path):
    _run_mutated("ivfsq4", seed, tmp_path)
