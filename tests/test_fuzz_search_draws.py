"""CPU checks of the search fuzz's draws (tests/fuzz_search_draws.py): the coverage of the sweep tests/test_gpu_fuzz_search.py
runs at VQ_FUZZ_SCALE=1, so that the fuzz cannot quietly shrink, and the numpy statements held to each other on the draws
themselves -- an inverted-file statement at nprobe == nlist equals the dense statement over the same rows.  `draw` is held
to the digests of tests/golden/fuzz_search_draws_digests.json; `draw_filtered`, the second draw over the same cases, has the
same three kinds of check for its filtered and Hamming-range ops, and so has `draw_mutated`, the third, for its adds and
removes."""
import dataclasses
import functools
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest

import fuzz_search_draws as D
import ref_abin as A
import ref_ivfsq as ISQ
import ref_knn as K
import ref_mutate as M
import ref_sq4 as S4
import ref_sqindex as SI

F = np.float32


@functools.lru_cache(maxsize=None)
def _cases(family):
    return [D.draw(family, s) for s in D.seeds(family)]


def _bytes(case):
    parts = [case.queries.tobytes()] + [case.data[k].tobytes() for k in sorted(case.data)]
    for o in case.ops:
        arrays = sorted(k for k, v in o.items() if isinstance(v, np.ndarray))  # radius; a filtered op: mask, ids, hradius
        parts.append(repr({k: v for k, v in o.items() if k not in arrays}).encode())
        parts += [o[k].tobytes() for k in arrays]
    return b"|".join(parts)


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_seed_counts():
    assert set(D.N_FAMILY) == set(D.PAIRS) == set(D.QUERY_OPS) == set(D.DENSE) | set(D.IVF)
    for family, nfam in D.N_FAMILY.items():
        assert 16 <= nfam <= 32, family


@pytest.mark.parametrize("family", D.FAMILIES)
def test_draw_is_deterministic(family):
    for s in (0, 3, D.N_FAMILY[family] - 1):
        a, b = D.draw(family, s), D.draw(family, s)
        assert a.describe() == b.describe()
        assert _bytes(a) == _bytes(b)
    assert _bytes(D.draw(family, 0)) != _bytes(D.draw(family, 1))


@pytest.mark.parametrize("family", D.FAMILIES)
def test_every_case_is_a_valid_call(family):
    for c in _cases(family):
        msg = c.describe()
        assert 1 <= c.n and 1 <= c.dim and c.queries.shape == (c.nq, c.dim), msg
        assert 1 <= c.nprobe <= min(c.nlist, 1024) and 1 <= c.topk <= min(c.n, 1024), msg
        assert 3 <= len(c.ops) <= 7, msg
        rows = 0 if family in D.IVF else c.n  # (a resident index is built over all its rows)
        for o in c.ops:
            if o["op"] == "add":
                assert o["lo"] == rows < o["n"] and o["how"] in c.ctor["adds"], msg
                rows = o["n"]
                continue
            assert o["op"] in D.QUERY_OPS[family] and o["n"] == rows >= 1, msg
            if o["op"] == "range_search":
                assert o["radius"].shape == (c.nq,) and o["radius"].dtype == F and not np.isnan(o["radius"]).any(), msg
            else:
                assert 1 <= o["topk"] <= min(rows, 1024), msg
            if o["op"] == "rerank_search":
                assert o["topk"] <= o["candidates"] <= min(rows, 1024), msg
        assert rows == c.n and c.ops[-1]["op"] != "add", msg
        if family in D.IVF:
            assert c.data["lists"].shape == (c.n,) and int(c.data["lists"].max()) < c.nlist, msg
        if family in ("pq", "ivfpq"):
            assert c.ctor["m"] * c.ctor["k"] <= 38400 and int(c.data["codes"].max()) < c.ctor["k"], msg
        if family in ("sq4", "ivfsq4"):  # codes of four bits, the words their packing, pad nibbles zero
            assert c.ctor["sq"][2] <= 16 and int(c.data["codes"].max()) <= 15, msg
            assert c.data["words"].dtype == np.uint32 and np.array_equal(c.data["words"], S4.pack4(c.data["codes"])), msg
            assert np.array_equal(S4.unpack4(c.data["words"], c.dim), c.data["codes"]), msg
        if family == "abin":  # the three forms of one set of bits, pad bits zero
            bits = A.unpack(c.data["words"], c.dim)
            assert np.array_equal(A.pack(bits), c.data["words"]), msg
            assert np.array_equal(c.data["bq_codes"] >= np.uint8(c.ctor["bq"][2]), bits), msg
            if c.ctor["source"] == "rows":
                assert np.array_equal(c.data["rows"] >= F(c.ctor["bq"][0]), bits), msg


@pytest.mark.parametrize("family", D.FAMILIES)
def test_coverage_at_scale_1(family):
    cases = _cases(family)
    pairs = Counter((c.kind, c.metric) for c in cases)
    assert set(pairs) == set(D.PAIRS[family])
    assert min(pairs.values()) >= 2, pairs
    ops = Counter(o["op"] for c in cases for o in c.ops)
    for name in D.QUERY_OPS[family] + (("add",) if family in D.IVF else ()):
        assert ops[name] >= 5, (name, ops)
    assert any(c.topk == min(c.n, 1024) for c in cases)
    if family in ("flat", "ivfflat"):
        assert {c.ctor["dtype"] for c in cases} == {"float32", "float16"}
    if family == "ivfpq":
        assert {c.ctor["residual"] for c in cases} == {False, True}
    if family in ("pq", "ivfpq"):
        assert {c.data["codes"].dtype.itemsize for c in cases} == {1, 2}
    if family in D.DENSE:
        cut = [c for c in cases if c.dense_cut]
        assert len(cut) >= 2
        for c in cut:
            stored = c.data["codes"] if family == "pq" else c.data["words"] if family in D.PACKED else c.data["rows"]
            equal = (stored.view(np.uint8).reshape(c.n, -1) == stored[:1].view(np.uint8).reshape(1, -1)).all(axis=1)
            assert c.n > 8192 and int(equal.sum()) > 8192 and not equal.all(), c.describe()
    if family in ("sq4", "ivfsq4"):
        assert any(c.dim % 8 != 0 for c in cases) and any(1 <= c.dim % 32 <= 7 for c in cases)
        assert any(int(c.data["codes"].max()) >= c.ctor["sq"][2] for c in cases), "no code at or above `levels`"
        assert {c.ctor["source"] for c in cases} == {"rows", "codes", "packed"}
        assert {c.ctor["sq"] for c in cases} == set(S4.QUANTIZERS)
    if family == "ivfsq4":
        assert {o["how"] for c in cases for o in c.ops if o["op"] == "add"} == {"add_rows", "add_codes", "add_packed"}
    if family == "abin":
        assert {c.ctor["source"] for c in cases} == {"rows", "codes", "packed"}
        assert {c.ctor["bq"][1:] for c in cases} == set(A.LOW_HIGH)
        assert any(c.dim % 32 == 0 for c in cases) and any(c.dim % 32 != 0 and c.dim > 32 for c in cases)
    if family in D.IVF:
        assert any(c.nprobe == c.nlist and c.nlist > 1 for c in cases)
        assert any(c.nprobe == 1 and c.nlist > 1 for c in cases)
        assert any(c.nq >= 17 for c in cases) and any(c.nq >= 130 for c in cases)
        assert any(c.nlist > c.n for c in cases)
        searches = [(c, o) for c in cases for o in c.ops if o["op"] != "add"]
        assert any((D.probed_rows(c, o["n"]) == 0).any() for c, o in searches), "no query whose every probed list is empty"

        def pieces_with_a_search_between(c):
            names = [o["op"] for o in c.ops]
            adds = [i for i, x in enumerate(names) if x == "add"]
            return len(adds) >= 3 and any(b - a > 1 for a, b in zip(adds, adds[1:]))

        assert any(pieces_with_a_search_between(c) for c in cases)


@pytest.mark.parametrize("family", ["ivfflat", "ivfsq", "ivfbin", "ivfsq4"])
def test_statements_agree_at_all_lists(family):
    """ref_ivfflat against ref_knn, ref_ivfsq against ref_sqindex, ref_ivfbin against ref_binary, ref_ivfsq4 against ref_sq4
    and ref_ivf_range against ref_range: at nprobe == nlist the inverted-file statement is the dense statement over the same rows -- on the drawn
    shapes themselves, after every add"""
    searched = ranged = 0
    for c in _cases(family):
        if c.nprobe != c.nlist:
            continue
        for o in c.ops:
            if o["op"] == "range_search":
                got, want = D.statement_range(c, o["n"], o["radius"]), D.dense_statement_range(c, o["n"], o["radius"])
                assert np.array_equal(got[0], want[0]), c.describe()
                _same(got[1:], want[1:])
                ranged += 1
            elif o["op"] != "add":
                _same(D.statement_search(c, o["n"], o["topk"]), D.dense_statement(c, o["n"], o["topk"]))
                searched += 1
    assert searched >= 1 and (ranged >= 1 or family == "ivfbin")


@pytest.mark.parametrize("family", D.PACKED)
def test_packed_statements_agree_with_the_8_bit_ones(family):
    """the identity the packed indexes claim, on the statements: ref_sq4 / ref_ivfsq4 over the packed words against
    ref_sqindex / ref_ivfsq over the unpacked codes under the same quantizer, ref_abin against ref_knn over its decoded
    rows -- on the drawn shapes themselves"""
    searched = 0
    for c in _cases(family):
        if c.dense_cut and searched:
            continue  # (one statement of 9000 rows is enough)
        for o in c.ops:
            if o["op"] in ("add", "range_search"):
                continue
            n, topk, d = o["n"], o["topk"], c.data
            if family == "abin":
                want = K.search(c.metric, c.queries, A.decode(d["words"][:n], c.dim, *c.ctor["bq"][1:]), topk)
            elif family == "sq4":
                want = SI.search(c.metric, c.queries, c.ctor["sq"], S4.unpack4(d["words"][:n], c.dim), topk)
            else:
                want = ISQ.search(c.metric, d["coarse"], d["lists"][:n], c.ctor["sq"], S4.unpack4(d["words"][:n], c.dim),
                                  c.queries, c.nprobe, topk)
            _same(D.statement_search(c, n, topk), want)
            searched += 1
            break
    assert searched >= 8


# -- draw() stays what it was ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", D.FAMILIES)
def test_draw_keeps_its_digests(family):
    """sha256 of _bytes(draw(family, seed)) for every seed of scale 1, recorded before draw_filtered was added (those of
    abin, sq4 and ivfsq4 with their families, before draw_mutated was): the data, the queries and the ops of every
    existing test_fuzz_<family>[seed] are byte for byte what they were"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_search_draws_digests.json")) as f:
        want = json.load(f)
    assert set(want) == set(D.FAMILIES) and len(want[family]) == D.N_FAMILY[family]
    for s, c in enumerate(_cases(family)):
        assert hashlib.sha256(_bytes(c)).hexdigest() == want[family][s], c.describe()


# -- the second draw ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _filtered_cases(family):
    return [D.draw_filtered(family, s) for s in D.seeds(family)]


@functools.lru_cache(maxsize=None)
def _filtered_ops(family):
    """(case, op, allowed rows in reach per query) of every filtered op"""
    return [(c, o, D.allowed_in_reach(c, o["n"], o["mask"])) for c in _filtered_cases(family) for o in c.ops if "mask" in o]


def _same_csr(got, want, msg):
    assert got[0].dtype == want[0].dtype == np.uint64 and np.array_equal(got[0], want[0]), msg
    assert got[1].dtype == want[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), msg
    assert got[2].dtype == want[2].dtype == F and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), msg


@pytest.mark.parametrize("family", D.FAMILIES)
def test_draw_filtered_is_deterministic(family):
    for s in (0, 3, D.N_FAMILY[family] - 1):
        a, b = D.draw_filtered(family, s), D.draw_filtered(family, s)
        assert a.describe() == b.describe()
        assert _bytes(a) == _bytes(b)
        old = D.draw(family, s)  # everything but the ops is draw()'s
        a.ops = old.ops
        assert _bytes(a) == _bytes(old) and a.describe() == old.describe()
    assert _bytes(D.draw_filtered(family, 0)) != _bytes(D.draw_filtered(family, 1))


@pytest.mark.parametrize("family", D.FAMILIES)
def test_every_filtered_case_is_a_valid_call(family):
    for c in _filtered_cases(family):
        msg = c.describe()
        assert 3 <= len(c.ops) <= 7, msg
        rows = 0 if family in D.IVF else c.n
        queries = new = 0
        for o in c.ops:
            if o["op"] == "add":
                assert o["lo"] == rows < o["n"] and o["how"] in c.ctor["adds"], msg
                rows = o["n"]
                continue
            queries += 1
            new += o["op"] in D.NEW_OPS[family]
            assert o["op"] in D.QUERY_OPS[family] + D.NEW_OPS[family] and o["n"] == rows >= 1, msg
            if "topk" in o:
                assert 1 <= o["topk"] <= min(rows, 1024), msg
            if "candidates" in o:
                assert o["topk"] <= o["candidates"] <= min(rows, 1024) and 0 <= o["flat_metric"] < 5, msg
            if "radius" in o:
                assert o["radius"].shape == (c.nq,) and o["radius"].dtype == F and not np.isnan(o["radius"]).any(), msg
            if "hradius" in o:
                assert o["hradius"].shape == (c.nq,) and o["hradius"].dtype.kind == "i" and (o["hradius"] >= 0).all(), msg
                assert o["hradius"][0] == 0 and (c.nq < 2 or o["hradius"][-1] == c.dim), msg
                assert c.nq < 17 or o["hradius"][-2] == c.dim + 7, msg
            assert ("topk" in o) + ("radius" in o) + ("hradius" in o) == 1, msg
            assert ("mask" in o) == (o["op"] in D.FILTERED), msg
            if "mask" in o:
                assert o["mask"].dtype == np.bool_ and o["mask"].shape == (rows,), msg
                assert o["mask_kind"] in D.mask_kinds(family) and o["form"] in D.FORMS, msg
                assert o["allowed"] == int(o["mask"].sum()), msg
                if o["form"] == "ids":
                    assert np.array_equal(np.sort(o["ids"]), np.flatnonzero(o["mask"])), msg
                text = D._op_text(o)  # the line a red seed replays from: op, n, topk, mask kind, form, allowed rows
                for word in (o["op"], f"n={rows}", f"mask={o['mask_kind']}", f"form={o['form']}", f"allowed={o['allowed']}"):
                    assert word in text, (word, text)
                assert "topk" not in o or f"topk={o['topk']}" in text, text
                assert "candidates" not in o or f"candidates={o['candidates']} flat_metric={o['flat_metric']}" in text, text
                assert not (o.get("after_close") and o.get("after_load")), msg
                assert not o.get("after_close") or (family in D.IVF and "after_close" in text), msg
                assert not o.get("after_load") or (family in D.HAS_SAVE and "after_load" in text), msg
        assert rows == c.n and c.ops[-1]["op"] != "add", msg
        assert 2 * new >= queries, msg  # at least half of the query ops are new ones
        assert all(D._op_text(o) in c.describe() for o in c.ops), msg


def _tied(case):
    """bool (n,): the rows of a dense-cut case that equal row 0"""
    stored = case.data["codes"] if case.family == "pq" else case.data["words"] if case.family in D.PACKED else case.data["rows"]
    b = stored.view(np.uint8).reshape(case.n, -1)
    return (b == b[:1]).all(axis=1)


@pytest.mark.parametrize("family", D.FAMILIES)
def test_filtered_coverage_at_scale_1(family):
    cases, fops = _filtered_cases(family), _filtered_ops(family)
    assert len(cases) == D.N_FAMILY[family]
    ops = Counter(o["op"] for c in cases for o in c.ops)
    for name in D.NEW_OPS[family]:
        assert ops[name] >= 5, (name, ops)
    kinds = Counter(o["mask_kind"] for _, o, _ in fops)
    for kind in D.mask_kinds(family):
        assert kinds[kind] >= 2, (kind, kinds)
    forms = Counter(o["form"] for _, o, _ in fops)
    for form in D.FORMS:
        assert forms[form] >= 3, (form, forms)
    topk_ops = [(c, o, reach) for c, o, reach in fops if "topk" in o]
    assert any((reach == 0).any() for _, _, reach in fops), "no query without an allowed row in reach"
    assert any(((reach >= 1) & (reach < o["topk"])).any() for _, o, reach in topk_ops), "no query between 1 and topk - 1"
    assert any((reach >= o["topk"]).all() for _, o, reach in topk_ops), "no op with every query full"
    if family in D.IVF:
        assert any(o["n"] < c.n for c, o, _ in fops), "no filtered op between two adds"
        assert any(o["mask_kind"] == "one_list" and (reach == 0).any() and (reach > 0).any() for _, o, reach in fops), \
            "no one_list op with a query that does not probe the list"
        assert any(o.get("after_close") for _, o, _ in fops)
    if family in D.HAS_SAVE:
        assert any(o.get("after_load") for _, o, _ in fops)
    if family in D.DENSE:
        cut = [(c, o) for c, o, _ in fops if c.dense_cut]
        assert len({c.seed for c, _ in cut}) >= 2
        assert any(int((_tied(c) & o["mask"]).sum()) > 8192 for c, o in cut), "no dense cut among the allowed rows"
        assert any(o["mask_kind"] in ("without_winners", "random") for _, o in cut)
    if family in ("binary", "ivfbin"):
        assert any("hradius" in o and c.nq >= 17 for c in cases for o in c.ops)
    if "filtered_rerank_search" in D.NEW_OPS[family]:
        assert any("candidates" in o and (reach < o["candidates"]).any() for _, o, reach in fops), \
            "no filtered rerank with fewer allowed rows in reach than candidates"


_gathered = D.gathered  # (the case over the allowed rows alone)


def _back(idx, rows):
    out = np.full(idx.shape, 0xFFFFFFFF, np.uint32)
    real = idx != 0xFFFFFFFF
    out[real] = rows[idx[real].astype(np.int64)]
    return out


@pytest.mark.parametrize("family", D.FAMILIES)
def test_filtered_statements_agree(family):
    """the filtered statements held to the others on the drawn ops themselves: under `ones` a filtered statement is the
    unfiltered one; for a resident family it is the unfiltered statement over the gathered allowed rows, ids mapped back
    and padded -- restated here; for an IVF case at nprobe == nlist it is the filtered statement of the resident index"""
    ones = gathered = dense = 0
    for c, o, _ in _filtered_ops(family):
        n, mask, msg = o["n"], o["mask"], c.describe()
        rows = np.flatnonzero(mask)
        if "hradius" in o:
            got = D.statement_hamming_range(c, n, o["hradius"], mask)
            unfiltered = lambda cc, nn: D.statement_hamming_range(cc, nn, o["hradius"])
            at_all_lists = lambda: D.statement_hamming_range(c, n, o["hradius"], mask, dense=True)
        elif "radius" in o:
            got = D.statement_filtered_range(c, n, o["radius"], mask)
            unfiltered = lambda cc, nn: D.statement_range(cc, nn, o["radius"])
            at_all_lists = lambda: D.dense_statement_filtered_range(c, n, o["radius"], mask)
        else:
            topk = o.get("candidates", o["topk"])  # (a rerank's first stage is the filtered statement at `candidates`)
            got = D.statement_filtered_search(c, n, topk, mask)
            unfiltered = lambda cc, nn: D.statement_search(cc, nn, min(topk, nn))
            at_all_lists = lambda: D.dense_statement_filtered(c, n, topk, mask)
            if "candidates" in o:  # the reranked result: each query's first hits of its short list in another order
                ri, rd = D.statement_rerank(c, n, got[0], o["topk"], o["flat_metric"])
                for j in range(c.nq):
                    real = ri[j][ri[j] != 0xFFFFFFFF]
                    assert real.size == min(o["topk"], np.count_nonzero(got[0][j] != 0xFFFFFFFF)), msg
                    assert np.isin(real, got[0][j]).all() and mask[real].all() and np.unique(real).size == real.size, msg
                    assert (rd[j, real.size:].view(np.uint32) == 0x7F800000).all(), msg
        csr = len(got) == 3
        if mask.all():
            want = unfiltered(c, n)
            _same_csr(got, want, msg) if csr else _same(got, want)
            ones += 1
        if family in D.DENSE:
            if csr:
                want = unfiltered(_gathered(c, n, rows), rows.size) if rows.size else \
                    (np.zeros(c.nq + 1, np.uint64), np.empty(0, np.uint32), np.empty(0, F))
                _same_csr(got, (want[0], _back(want[1], rows), want[2]), msg)
            else:
                idx = np.full(got[0].shape, 0xFFFFFFFF, np.uint32)
                dist = np.full(got[1].shape, np.inf, F)
                if rows.size:
                    i, d = unfiltered(_gathered(c, n, rows), rows.size)
                    idx[:, :i.shape[1]], dist[:, :i.shape[1]] = _back(i, rows), d
                _same((got[0], got[1]), (idx, dist))
            gathered += 1
        elif c.nprobe == c.nlist:
            want = at_all_lists()
            if want is not None:  # (the residual IVFPQ index has no resident form)
                _same_csr(got, want, msg) if csr else _same(got, want)
                dense += 1
    assert ones >= 1 and (gathered >= 1 if family in D.DENSE else dense >= 1)


# -- the third draw ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mutated_cases(family):
    return [D.draw_mutated(family, s) for s in D.mutated_seeds(family)]


def _removes(family):
    """(case, position, op) of every remove op"""
    return [(c, i, o) for c in _mutated_cases(family) for i, o in enumerate(c.ops) if o["op"] == "remove"]


def _adds_of(c):
    return c.ctor["adds"] if c.family in D.IVF else D.resident_adds(c)


def test_mutable_families():
    assert set(D.MUTABLE) == set(D.FAMILIES) - {"pq"} and len(D.MUTABLE) == 10


@pytest.mark.parametrize("family", D.MUTABLE)
def test_draw_mutated_is_deterministic(family):
    for s in (0, 3, D.N_MUTATED[family] - 1):
        a, b = D.draw_mutated(family, s), D.draw_mutated(family, s)
        assert a.describe() == b.describe()
        assert _bytes(a) == _bytes(b)
        old = D.draw(family, s)  # everything but the ops is draw()'s
        a.ops = old.ops
        assert _bytes(a) == _bytes(old) and a.describe() == old.describe()
    assert _bytes(D.draw_mutated(family, 0)) != _bytes(D.draw_mutated(family, 1))


@pytest.mark.parametrize("family", D.MUTABLE)
def test_every_mutated_case_is_a_valid_call(family):
    ivf = family in D.IVF
    for c in _mutated_cases(family):
        msg = c.describe()
        assert 4 <= len(c.ops) <= 9, msg
        start = 0 if ivf else D.built_over(c)
        assert 1 <= start <= c.n or ivf, msg
        present = np.arange(start, dtype=np.int64)  # the original ids of the rows in the index
        arrived = start
        counts = Counter(o["op"] for o in c.ops)
        assert 1 <= counts["remove"] <= 3 and (1 <= counts["add"] <= 3 if ivf else counts["add"] <= 2), msg
        assert len({o["flat_metric"] for o in c.ops if "flat_metric" in o}) <= 1, msg
        for i, o in enumerate(c.ops):
            text = D._op_text(o)
            assert text in c.describe() and text in c.describe(i), msg
            if o["op"] == "add":
                assert o["lo"] == arrived < o["hi"] <= c.n and o["how"] in _adds_of(c) and o["at"] == present.size, msg
                present = np.concatenate([present, np.arange(o["lo"], o["hi"])])
                arrived = o["hi"]
                assert o["n"] == present.size and np.array_equal(o["present"], present), msg
                assert f"[{o['lo']}:{o['hi']}]@{o['at']}" in text, text
                continue
            if o["op"] == "remove":
                n0, arg = present.size, o["arg"]
                assert n0 >= 1 and o["n_before"] == n0 and o["kind"] in D.remove_kinds(family) and o["form"] in D.REMOVE_FORMS, msg
                if o["form"] == "bool":
                    assert arg.dtype == np.bool_ and arg.shape == (n0,), msg
                else:
                    assert arg.dtype == np.int64 and arg.ndim == 1 and (arg.size == 0 or (0 <= arg.min() and arg.max() < n0)), msg
                gone = M.remove_mask(n0, arg)
                present = present[M.kept(n0, arg).astype(np.int64)]
                assert o["removed"] == int(gone.sum()) == n0 - present.size, msg
                assert o["n"] == present.size and np.array_equal(o["present"], present), msg
                assert present.size >= 1 or (ivf and c.ops[i + 1]["op"] == "add"), msg  # (a query op needs a row)
                where = np.flatnonzero(gone)
                if o["kind"] == "nothing":
                    assert where.size == 0, msg
                if o["kind"] == "everything":
                    assert ivf and present.size == 0, msg
                if o["kind"] == "all_but_one":
                    assert present.size == 1, msg
                if o["kind"] == "word_straddle":
                    assert where.size == 4 and where[0] % 32 == 30 and np.array_equal(where, where[0] + np.arange(4)), msg
                if o["kind"] == "block64":
                    assert where[0] % 64 == 0 and np.array_equal(where, np.arange(where[0], where[-1] + 1)), msg
                    assert where[-1] + 1 == n0 or (where[-1] + 1) % 64 == 0, msg
                if o["kind"] in ("block", "one_row"):
                    assert where.size >= 1 and np.array_equal(where, np.arange(where[0], where[-1] + 1)), msg
                if o["kind"] == "one_list" and where.size:
                    lists = c.data["lists"][c.ops[i - 1]["present"]]
                    assert np.unique(lists[where]).size == 1 and (where.size == n0 - 1 or not (lists[~gone] == lists[where[0]]).any()), msg
                for word in (f"n={n0}->{o['n']}", f"kind={o['kind']}", f"form={o['form']}", f"removed={o['removed']}"):
                    assert word in text, (word, text)
                assert not (o.get("then_close") and o.get("then_load")), msg
                assert not o.get("then_close") or (ivf and "then_close" in text and present.size), msg
                assert not o.get("then_load") or (family in D.HAS_SAVE and "then_load" in text and present.size), msg
                continue
            rows = present.size
            assert o["op"] in D.QUERY_OPS[family] + D.NEW_OPS[family] and o["n"] == rows >= 1, msg
            assert np.array_equal(o["present"], present), msg
            assert ("topk" in o) + ("radius" in o) + ("hradius" in o) == 1, msg
            if "topk" in o:
                assert 1 <= o["topk"] <= min(rows, 1024), msg
            if "candidates" in o:
                assert o["topk"] <= o["candidates"] <= min(rows, 1024) and 0 <= o["flat_metric"] < 5, msg
            if "radius" in o:
                assert o["radius"].shape == (c.nq,) and o["radius"].dtype == F and not np.isnan(o["radius"]).any(), msg
            if "hradius" in o:
                assert o["hradius"].shape == (c.nq,) and (o["hradius"] >= 0).all(), msg
            assert ("mask" in o) == (o["op"] in D.FILTERED), msg
            if "mask" in o:  # over the rows present at that op
                assert o["mask"].dtype == np.bool_ and o["mask"].shape == (rows,) and o["allowed"] == int(o["mask"].sum()), msg
                assert o["mask_kind"] in D.mask_kinds(family) and o["mask_kind"] != "higher_twins" and o["form"] in D.FORMS, msg
                if o["form"] == "ids":
                    assert np.array_equal(np.sort(o["ids"]), np.flatnonzero(o["mask"])), msg
        assert arrived == c.n and c.ops[-1]["op"] not in ("add", "remove"), msg


def _probed_lists(c):
    return np.unique(D.I.probe(c.coarse_metric, c.data["coarse"], c.queries, c.nprobe))


@pytest.mark.parametrize("family", D.MUTABLE)
def test_mutated_coverage_at_scale_1(family):
    cases, removes = _mutated_cases(family), _removes(family)
    ivf = family in D.IVF
    assert len(cases) == D.N_MUTATED[family] >= D.N_FAMILY[family]
    pairs = Counter((c.kind, c.metric) for c in cases)
    assert set(pairs) == set(D.PAIRS[family]) and min(pairs.values()) >= 2, pairs
    ops = Counter(o["op"] for c in cases for o in c.ops)
    for name in D.QUERY_OPS[family] + D.NEW_OPS[family] + ("remove", "add"):
        assert ops[name] >= 5, (name, ops)
    kinds = Counter(o["kind"] for _, _, o in removes)
    for kind in D.remove_kinds(family):
        assert kinds[kind] >= 2, (kind, kinds)
    forms = Counter(o["form"] for _, _, o in removes)
    for form in D.REMOVE_FORMS:
        assert forms[form] >= 3, (form, forms)
    assert any(o["form"] == "ids" and np.unique(o["arg"]).size < o["arg"].size for _, _, o in removes), "no id given twice"
    assert any(o["n"] == 1 for _, _, o in removes), "no remove that leaves exactly one row"

    def crosses_64(o):  # removed rows on both sides of a multiple of 64, rows behind them: survivors move across a tile edge
        where = np.flatnonzero(M.remove_mask(o["n_before"], o["arg"]))
        return where.size >= 2 and where[0] // 64 != where[-1] // 64 and o["n"] >= 1

    assert any(crosses_64(o) for _, _, o in removes), "no remove across a multiple of 64"
    assert any(np.flatnonzero(M.remove_mask(o["n_before"], o["arg"])).size and o["n_before"] % 32 != 0
               and o["n_before"] > 32 for _, _, o in removes), "no remove under a mask whose last word is partial"
    assert any(c.ops[i + 1]["op"] == "add" for c, i, _ in removes), "no add directly behind a remove"
    if ivf:
        def empties_a_probed_list(c, i, o):
            before = c.data["lists"][c.ops[i - 1]["present"]]
            after = c.data["lists"][o["present"]]
            emptied = np.setdiff1d(np.unique(before), np.unique(after))
            return o["n"] >= 1 and np.isin(emptied, _probed_lists(c)).any()

        assert any(empties_a_probed_list(c, i, o) for c, i, o in removes), "no remove that empties a probed list"
        assert any(o["kind"] == "everything" and c.ops[i + 1]["op"] == "add" for c, i, o in removes)
        assert any("add" in [x["op"] for x in c.ops[:i]] and "add" in [x["op"] for x in c.ops[i + 1:]] for c, i, _ in removes), \
            "no remove between two adds"
        assert any(o.get("then_close") for _, _, o in removes)
    else:
        assert any(D.built_over(c) < c.n for c in cases) and any(D.built_over(c) == c.n for c in cases)
        assert {o["how"] for c in cases for o in c.ops if o["op"] == "add"} >= set(D.resident_adds(cases[0])[-1:])
    if family in D.HAS_SAVE:
        assert any(o.get("then_load") for _, _, o in removes)
    behind = Counter()  # the query ops with a remove before them
    for c in cases:
        seen = False
        for o in c.ops:
            seen = seen or o["op"] == "remove" and o["removed"] > 0
            if seen and o["op"] not in ("add", "remove"):
                behind["filtered" if "mask" in o else "range" if ("radius" in o or "hradius" in o) else "search"] += 1
    has_range = any("range" in name for name in D.QUERY_OPS[family] + D.NEW_OPS[family])  # (IVFPQIndex has no range search)
    assert behind["search"] >= 1 and (behind["range"] >= 1 or not has_range) and behind["filtered"] >= 1, behind
    if family in D.DENSE:
        assert any(c.dense_cut and any(o["op"] == "remove" and o["removed"] for o in c.ops) for c in cases)


def _statement(case, o):
    """the statement of one query op (a rerank's: its first stage), every result as a tuple of arrays"""
    n = o["n"]
    if "hradius" in o:
        return D.statement_hamming_range(case, n, o["hradius"], o.get("mask"))
    if "radius" in o:
        return D.statement_filtered_range(case, n, o["radius"], o["mask"]) if "mask" in o else D.statement_range(case, n, o["radius"])
    topk = o.get("candidates", o["topk"])
    return D.statement_filtered_search(case, n, topk, o["mask"]) if "mask" in o else D.statement_search(case, n, topk)


@pytest.mark.parametrize("family", D.MUTABLE)
def test_mutated_statements_agree(family):
    """the statement over `gathered(case, n, present)` a mutated query op is held to, against ref_mutate.apply -- every
    per-row array put through the case's adds and removes -- followed by the plain statement over what it leaves: on the
    first query op behind each remove"""
    checked = 0
    for c in _mutated_cases(family):
        start = 0 if family in D.IVF else D.built_over(c)
        per_row = {k: (v if v.ndim == 2 else v[:, None]) for k, v in c.data.items() if k in D.PER_ROW}
        rows = {k: v[:start] for k, v in per_row.items()}
        due = False
        for o in c.ops:
            if o["op"] == "add":
                piece = {k: v[o["lo"]:o["hi"]] for k, v in per_row.items()}
                rows = {k: M.apply(rows[k], [("add", piece[k])]) if rows[k].shape[0] else piece[k] for k in per_row}
            elif o["op"] == "remove":
                if o["n"] == 0:  # (ref_mutate.apply keeps a row: an emptied IVF index starts again)
                    rows = {k: v[:0] for k, v in per_row.items()}
                else:
                    rows = {k: M.apply(rows[k], [("remove", o["arg"])]) for k in per_row}
                due = o["removed"] > 0
            elif due:
                data = dict(c.data)
                data.update({k: (v if c.data[k].ndim == 2 else v[:, 0]) for k, v in rows.items()})
                plain = dataclasses.replace(c, n=o["n"], data=data, gathered=True, cache={})
                got = _statement(D.gathered(c, c.n, o["present"]), o)
                want = _statement(plain, o)
                assert len(got) == len(want) and plain.data[next(iter(rows))].shape[0] == o["n"], c.describe()
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if g.dtype == F else g,
                                                                 w.view(np.uint32) if w.dtype == F else w), c.describe()
                checked += 1
                due = False
    assert checked >= 8
