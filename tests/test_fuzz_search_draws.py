"""CPU checks of the search fuzz's draws (tests/fuzz_search_draws.py): the coverage of the sweep tests/test_gpu_fuzz_search.py
runs at VQ_FUZZ_SCALE=1, so that the fuzz cannot quietly shrink, and the numpy statements held to each other on the draws
themselves -- an inverted-file statement at nprobe == nlist equals the dense statement over the same rows."""
import functools
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
        parts.append(repr({k: v for k, v in o.items() if k != "radius"}).encode())
        if "radius" in o:
            parts.append(o["radius"].tobytes())
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
