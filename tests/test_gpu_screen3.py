"""The three-product form of the pipelined encode screen (k_assign_screen_bf16_x32p with NPR = 3: sub_dim 16 or 13..15
padded onto it, k in 225..256, squared-L2 / Euclidean): every code bit for bit against the oracle on rows built to sit
on the margin -- twin centroids 1 ulp apart, rows on centroids and on midpoints of two centroids, a subspace with a common
offset of 1000 (the centring), rows of norm 1e18 and 1e-30, NaN / inf rows and the last row of a partial step.  The
export vqhip_last_screen_products names the form that ran: 3 here, 6 for the training step and the cosine encode."""
import functools

import numpy as np
import pytest

import oracle as O
from vq_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32

SHAPES = [(40_007, 8, 256, 16),   # ragged row count
          (33_000, 3, 250, 16),   # odd m, partial last tile
          (40_001, 1, 225, 16),   # smallest k of the variant
          (40_000, 8, 256, 13)]   # padded onto the 16 kernel


@functools.lru_cache(maxsize=None)
def _data(shape):
    n, m, k, sd = shape
    rng = np.random.default_rng(n + 7 * sd)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    for s in range(m):
        for j in range(0, k - 1, 8):  # every eighth centroid has a twin 1 ulp away in one coordinate
            cb[s, j + 1] = cb[s, j]
            t = (j // 8) % sd
            cb[s, j + 1, t] = np.nextafter(cb[s, j, t], F(9.0))
    X = rng.standard_normal((n, m * sd)).astype(F)
    for i in rng.integers(0, n, n // 50):      # rows on top of a centroid
        for s in range(m):
            X[i, s * sd:(s + 1) * sd] = cb[s, rng.integers(0, k)] + (1e-4 * rng.standard_normal(sd)).astype(F)
    for i in rng.integers(0, n, n // 50):      # rows on the midpoint of two centroids (exactly, or one rounding off it)
        for s in range(m):
            j1, j2 = rng.integers(0, k, 2)
            X[i, s * sd:(s + 1) * sd] = (cb[s, j1] + cb[s, j2]) * F(0.5)
    cb[0] += F(1000.0)                         # subspace 0: rows and centroids share an offset of 1000
    X[:, :sd] += F(1000.0)
    X[11, :] = (rng.standard_normal(m * sd) * 1e18 / np.sqrt(sd)).astype(F)   # sub-vector norms ~1e18
    X[12, :] = (rng.standard_normal(m * sd) * 1e-30 / np.sqrt(sd)).astype(F)  # ... and ~1e-30
    X[5, 3] = np.nan
    X[n // 3, :] = np.nan
    X[n - 2, 7] = -np.inf
    X[n - 1, :] = np.inf                       # the last row (of a partial step when n % 32 != 0)
    X.setflags(write=False)
    cb.setflags(write=False)
    return X, cb


@functools.lru_cache(maxsize=None)
def _reference(shape, metric):
    X, cb = _data(shape)
    codes, _ = O.get().pq_encode(metric, X, cb, threads=0)
    codes.setflags(write=False)
    return codes


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("metric", [O.SQUARED_EUCLIDEAN, O.EUCLIDEAN])
def test_three_product_encode_bit_exact(shape, metric):
    n, m, k, sd = shape
    X, cb = _data(shape)
    enc = _lib.PQEncoder(cb, metric)
    codes, _ = enc.encode(X, want_f16=False)
    rechecked, engine = _lib.last_assign_stats()
    products = _lib.last_screen_products()
    print(f"shape {shape} metric {metric}: products {products} rechecked {rechecked} of {n * m} ({100.0 * rechecked / (n * m):.2f} %)")
    assert engine == _lib.ENGINE_MFMA_BF16
    assert products == 3
    assert rechecked > 0
    np.testing.assert_array_equal(codes.astype(np.uint32), _reference(shape, metric))
    enc.close()
    # the other forms at the same shape stay on six products: cosine encode, training step
    enc = _lib.PQEncoder(cb, O.COSINE)
    enc.encode(X, want_f16=False)
    assert _lib.last_assign_stats()[1] == _lib.ENGINE_MFMA_BF16 and _lib.last_screen_products() == 6
    enc.close()
    ds = _lib.Dataset.from_host(np.nan_to_num(X, nan=0.0, posinf=0.0, neginf=0.0))
    km = _lib.KMeans(ds, m, k)
    km.set_centroids(cb)
    km.step()
    assert _lib.last_assign_stats()[1] == _lib.ENGINE_MFMA_BF16 and _lib.last_screen_products() == 6
    km.close()
    ds.close()


def test_three_product_recheck_share_on_normal_rows():
    """Plain N(0,1) rows and codebooks: the re-checked share stays under 5 % of n m (the cap of tests/test_gpu_fullsize.py),
    so a margin accidentally too wide cannot hide behind the exact re-check; the six-product form re-checks 0.3 % here."""
    n, m, k, sd = 40_000, 8, 256, 16
    rng = np.random.default_rng(3)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    X = rng.standard_normal((n, m * sd)).astype(F)
    enc = _lib.PQEncoder(cb, O.SQUARED_EUCLIDEAN)
    codes, _ = enc.encode(X, want_f16=False)
    rechecked, engine = _lib.last_assign_stats()
    print(f"N(0,1): rechecked {rechecked} of {n * m} ({100.0 * rechecked / (n * m):.3f} %)")
    assert engine == _lib.ENGINE_MFMA_BF16 and _lib.last_screen_products() == 3
    assert rechecked < 0.05 * n * m
    want, _ = O.get().pq_encode(O.SQUARED_EUCLIDEAN, X, cb, threads=0)
    np.testing.assert_array_equal(codes.astype(np.uint32), want)
    enc.close()
