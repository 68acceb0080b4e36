"""The expected-answer helpers of tests/test_gpu_big_offsets.py (tests/big_offsets.py) against brute force, with the
32-bit boundaries scaled down to 2^12 / 2^13 so every row can be checked."""
import numpy as np
import pytest

import big_offsets as BO

LO, HI = 1 << 12, 1 << 13


@pytest.mark.parametrize("n,row_elems,elem_bytes", [(9000, 4, 4), (LO + 7, 1, 2), (3000, 2, 4), (HI + 3, 1, 1), (100, 8, 4)])
def test_boundary_rows_hold_the_boundary(n, row_elems, elem_bytes):
    got = BO.boundary_rows(n, row_elems, elem_bytes, LO, HI)
    for name, r in got.items():
        kind, val = name.split()
        b = int(val, 16)
        if kind == "byte":
            assert r * row_elems * elem_bytes <= b < (r + 1) * row_elems * elem_bytes
        elif kind == "element":
            assert r * row_elems <= b < (r + 1) * row_elems
        else:
            assert r == b
        assert r < n
    # every boundary that falls inside the array is named
    want = {b // elem_bytes // row_elems for b in (LO, HI)} | {b // row_elems for b in (LO, HI)} | {LO}
    assert set(got.values()) == {r for r in want if r < n}


@pytest.mark.parametrize("n,rows,half", [(LO + 4099, [LO // 4, LO // 2, LO], 64), (300, [5, 290], 64), (100, [50], 64),
                                         (10_000, [4000, 4001, 9999], 16)])
def test_windows_match_brute_force(n, rows, half):
    spans = BO.windows(n, rows, half)
    want = np.zeros(n, bool)
    want[:half] = True
    want[max(0, n - half):] = True
    for r in rows:
        want[max(0, r - half):min(n, r + half)] = True
    got = np.zeros(n, bool)
    got[BO.window_index(spans)] = True
    assert np.array_equal(got, want)
    assert all(a < b for a, b in spans) and all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1))
    assert np.array_equal(BO.window_index(spans), np.nonzero(want)[0])


def test_sample_rows_distinct_sorted_seeded():
    s = BO.sample_rows(1 << 20, 5000, seed=3)
    assert s.size == 5000 and np.all(np.diff(s) > 0) and s[-1] < (1 << 20)
    assert np.array_equal(s, BO.sample_rows(1 << 20, 5000, seed=3))
    assert np.array_equal(BO.sample_rows(10, 50, seed=1), np.arange(10))


@pytest.mark.parametrize("m,k,topk", [(8, 256, 10), (2, 256, 300), (4, 300, 10), (2, 40, 7)])
def test_adc_planted_rows_are_the_brute_force_topk(m, k, topk):
    """the planted rows' expectation of the ADC tests: with every other row's codes in [1, k), the brute-force top-k over
    all rows starts with the planted rows in the order given"""
    n = HI + 4099
    rng = np.random.default_rng(m * k)
    rows = BO.boundary_rows(n, m, 1 if k <= 256 else 2, LO, HI)
    planted = BO.adc_planted_rows(n, rows.values())
    assert planted[0] == n - 1 and len(set(planted)) == len(planted)
    codes = rng.integers(1, k, size=(n, m))
    codes[planted] = BO.adc_planted_codes(m, len(planted))
    cb = BO.adc_codebooks(m, k, 2)
    table = BO.adc_table(cb)
    # the table against the definition: sum over the sub-vector of (0 - c)^2, f64 (exact here)
    assert np.array_equal(table.astype(np.float64), (cb.astype(np.float64) ** 2).sum(-1))
    dist = BO.adc_distances(table, codes)
    ref = np.array([sum(float(table[s][codes[i, s]]) for s in range(m)) for i in range(n)])
    assert np.array_equal(dist.astype(np.float64), ref)  # exact: the sums need few bits
    order = np.lexsort((np.arange(n), dist))[:topk]
    lead = min(topk, len(planted))
    assert list(order[:lead]) == planted[:lead]
    # beats(): nothing beats the brute-force k-th; a row moved ahead of it is found
    kth = order[-1]
    assert BO.beats(dist, np.arange(n), dist[kth], kth, order).size == 0
    d2 = dist.copy()
    other = np.setdiff1d(np.arange(n), order)[123]
    d2[other] = np.float32(0.5)
    assert list(BO.beats(d2, np.arange(n), dist[kth], kth, order)) == [other]


def test_centroid_statements_match_brute_force():
    """f64_sums and sequential_f32_means against a plain loop over the rows, on values that are multiples of 2^-24 in
    [0, 1) (the synthetic matrix) with clusters large enough that the f32 chains round"""
    rng = np.random.default_rng(8)
    n, k, sd = 20000, 7, 3
    cols = (rng.integers(0, 1 << 24, size=(n, sd)) * 2.0 ** -24).astype(np.float32)
    assign = rng.integers(0, k - 1, size=n)  # cluster k-1 stays empty
    c, S = BO.f64_sums(assign, cols, k)
    got = BO.sequential_f32_means(assign, cols, k)
    cnt = np.zeros(k, np.int64)
    s64 = np.zeros((k, sd))
    s32 = np.zeros((k, sd), np.float32)
    for i in range(n):
        j = assign[i]
        cnt[j] += 1
        s64[j] += cols[i].astype(np.float64)
        s32[j] = (s32[j] + cols[i]).astype(np.float32)
    assert np.array_equal(c, cnt) and np.array_equal(S, s64)
    want = np.zeros((k, sd), np.float32)
    ne = cnt > 0
    want[ne] = s32[ne] / cnt[ne, None].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(want[ne], (s64[ne] / cnt[ne, None]).astype(np.float32))  # the f32 chains did round
