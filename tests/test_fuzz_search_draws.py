"""CPU checks of the search fuzz's draws (tests/fuzz_search_draws.py): the coverage of the sweep tests/test_gpu_fuzz_search.py
runs at VQ_FUZZ_SCALE=1, so that the fuzz cannot quietly shrink, and the numpy statements held to each other on the draws
themselves -- an inverted-file statement at nprobe == nlist equals the dense statement over the same rows.  `draw` is held
to the digests of tests/golden/fuzz_search_draws_digests.json; `draw_filtered`, the second draw over the same cases, has the
same three kinds of check for its filtered and Hamming-range ops."""
import dataclasses
import functools
import hashlib
import json
import os
from collections import Counter

import numpy as np
import pytest

import fuzz_search_draws as D

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
            stored = c.data["codes"] if family == "pq" else c.data["rows"]
            equal = (stored.view(np.uint8).reshape(c.n, -1) == stored[:1].view(np.uint8).reshape(1, -1)).all(axis=1)
            assert c.n > 8192 and int(equal.sum()) > 8192 and not equal.all(), c.describe()
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


@pytest.mark.parametrize("family", ["ivfflat", "ivfsq", "ivfbin"])
def test_statements_agree_at_all_lists(family):
    """ref_ivfflat against ref_knn, ref_ivfsq against ref_sqindex, ref_ivfbin against ref_binary and ref_ivf_range against
    ref_range: at nprobe == nlist the inverted-file statement is the dense statement over the same rows -- on the drawn
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


# -- draw() stays what it was ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", D.FAMILIES)
def test_draw_keeps_its_digests(family):
    """sha256 of _bytes(draw(family, seed)) for every seed of scale 1, recorded before draw_filtered was added: the data, the
    queries and the ops of every existing test_fuzz_<family>[seed] are byte for byte what they were"""
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
    stored = case.data["codes"] if case.family == "pq" else case.data["rows"]
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


def _gathered(case, n, rows):
    """the case over the allowed rows alone: every per-row array gathered, the rest as it is"""
    per_row = ("rows", "stored", "codes", "words", "bq_codes", "rerank_rows")
    data = {k: (v[:n][rows] if k in per_row else v) for k, v in case.data.items()}
    return dataclasses.replace(case, n=int(rows.size), data=data)


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
