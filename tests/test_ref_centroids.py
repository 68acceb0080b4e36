"""The f64 centroid bound of tests/ref_centroids.py, held against the C oracle and numpy (no GPU): the reference's own
sequential mean and an f64 mean rounded once pass it; a lost member, flushed subnormals and an f32 division after a
long f32 sum fail it."""
import numpy as np
import pytest

import ref_centroids as RC

F = np.float32


def _rows(kind, n, d, rng):
    if kind == "uniform":
        return rng.random((n, d), dtype=F)
    if kind == "tiny":
        return (rng.standard_normal((n, d)) * 1e-20).astype(F)
    if kind == "subnormal":
        x = rng.standard_normal((n, d)) * np.where(rng.random((n, d)) < 0.5, 1e-40, 1e-38)
        return x.astype(F)
    if kind == "offset":
        return (F(4096) + F(0.5) * rng.random((n, d), dtype=F)).astype(F)
    if kind == "cancel":
        s = np.where(rng.random((n, d)) < 0.5, -1e4, 1e4)
        return (s + rng.standard_normal((n, d))).astype(F)
    raise ValueError(kind)


def _sequential_mean(x):
    """vector.rs:368-384: f32 adds in row order, f32 divide"""
    acc = np.zeros(x.shape[1], F)
    for row in x:
        acc = (acc + row).astype(F)
    return (acc / F(len(x))).astype(F)


@pytest.mark.parametrize("kind", ["uniform", "tiny", "subnormal", "offset", "cancel"])
def test_oracle_step_passes_with_l_equal_c(oracle, kind):
    rng = np.random.default_rng(7)
    n, sd, k = 3000, 4, 8
    X = _rows(kind, n, sd, rng)
    c0 = X[rng.choice(n, k, replace=False)]
    c1, assign, counts, _ = oracle.lloyd_step(X, c0)
    c, _, _ = RC.exact_means(X, assign, k)
    np.testing.assert_array_equal(c, counts)
    RC.assert_centroids(X, assign, c1, k, R=None, what=kind)


@pytest.mark.parametrize("kind", ["uniform", "tiny", "subnormal", "offset", "cancel"])
def test_f64_mean_rounded_once_passes_with_l_equal_1(kind):
    rng = np.random.default_rng(8)
    n, sd, k = 5000, 3, 5
    X = _rows(kind, n, sd, rng)
    assign = rng.integers(0, k, n)
    got = np.stack([X[assign == j].astype(np.float64).sum(0) / (assign == j).sum() for j in range(k)]).astype(F)
    RC.assert_centroids(X, assign, got, k, R=1, what=kind)


def test_sequential_chain_passes_with_its_chunk_length():
    """chunks of 256 rows summed in f32, partials combined in f64: passes with R = 256"""
    rng = np.random.default_rng(9)
    X = _rows("offset", 4096, 2, rng)
    assign = np.zeros(4096, np.int64)
    parts = [_sequential_mean(X[i:i + 256]).astype(np.float64) * 256 for i in range(0, 4096, 256)]
    got = (np.sum(parts, axis=0) / 4096).astype(F)[None, :]
    RC.assert_centroids(X, assign, got, 1, R=256, what="chunks of 256")


# ---- teeth --------------------------------------------------------------------------------------------------------

def test_bound_rejects_a_dropped_member():
    """offset data, a cluster of a few hundred members, one member's sum left out (count kept)"""
    rng = np.random.default_rng(10)
    X = _rows("offset", 300, 4, rng)
    assign = np.zeros(300, np.int64)
    got = ((X.astype(np.float64).sum(0) - X[137]) / 300).astype(F)[None, :]
    bad, worst = RC.centroid_violations(X, assign, got, 1, R=None)
    assert len(bad) == 4 and worst > 1
    with pytest.raises(AssertionError):
        RC.assert_centroids(X, assign, got, 1, R=None)


def test_bound_rejects_flushed_subnormals():
    rng = np.random.default_rng(11)
    X = _rows("subnormal", 2000, 4, rng)
    assign = rng.integers(0, 4, 2000)
    flushed = np.where(np.abs(X) < np.finfo(F).tiny, F(0), X)
    got = np.stack([flushed[assign == j].astype(np.float64).sum(0) / (assign == j).sum() for j in range(4)]).astype(F)
    with pytest.raises(AssertionError):
        RC.assert_centroids(X, assign, got, 4, R=None)


def test_bound_rejects_f32_division_after_a_long_f32_sum():
    """4096 rows at 4096 + 0.5 U summed in f32 and divided in f32 (the reference's own arithmetic) is NOT a path whose
    partials are f64 sums rounded once: checked with L = 1 it must fail"""
    rng = np.random.default_rng(12)
    X = _rows("offset", 4096, 4, rng)
    assign = np.zeros(4096, np.int64)
    got = _sequential_mean(X)[None, :]
    with pytest.raises(AssertionError):
        RC.assert_centroids(X, assign, got, 1, R=1)
    RC.assert_centroids(X, assign, got, 1, R=None)  # and with L = c it is within the bound


def test_changed_helper_flags_the_threshold_band():
    X = np.array([[0.0], [2e-6]], F)
    assign = np.array([0, 0])
    old = np.array([[0.0]], F)
    mean = np.array([[1e-6]], F)  # |new - old| lands on the threshold itself
    _, amb = RC.changed_expected(X, assign, mean, old, 1, True)
    assert amb
    old2 = np.array([[0.5]], F)
    exp, amb2 = RC.changed_expected(X, assign, mean, old2, 1, True)
    assert exp and not amb2
