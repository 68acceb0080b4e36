"""The grid reduce of the pipelined screen (k_assign_screen_bf16_x32p: column and row minima on untagged values, tags on
the 24 minima only) on the GPU, every code bit for bit against the oracle: the winner at each of the 256 index
decodings, twin centroids in every relation of the grid (same row class, same column class, other lane half, other
tile), the row counts at the pipeline's edges, and the cap on the re-checked share.  tests/test_grid_reduce.py has the
numpy statement of the reduce itself."""
import functools

import numpy as np
import pytest

import oracle as O
from vq_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
K_PIPE_MIN_STEPS = 8   # kPipeMinSteps: shortest row chunk, in 32-row steps, of the pipelined kernel
WAVES_PER_BLOCK = 4    # kWavesPerBlock


def _encode_device(cb, X, metric=O.SQUARED_EUCLIDEAN):
    """One launch over exactly X's rows (a host call may split them): codes, re-checked entries, products of the screen."""
    import torch

    enc = _lib.PQEncoder(cb, metric)
    enc.set_engine(_lib.ENGINE_MFMA_BF16)   # by name: left to itself the library gives small work to the exact scan
    dx = torch.from_numpy(np.array(X, dtype=F, order="C", copy=True)).cuda()
    dc = torch.empty((X.shape[0], cb.shape[0]), dtype=torch.uint8, device="cuda")
    enc.encode_device(dx.data_ptr(), X.shape[0], dc.data_ptr(), None)
    _lib.synchronize()
    rechecked, engine = _lib.last_assign_stats()
    products = _lib.last_screen_products()
    codes = dc.cpu().numpy()
    enc.close()
    assert engine == _lib.ENGINE_MFMA_BF16
    return codes, rechecked, products


def _oracle(cb, X, metric=O.SQUARED_EUCLIDEAN):
    want, _ = O.get().pq_encode(metric, X, cb, threads=0)
    return want


def _sd8_chunks(m):
    """Row chunks the launcher cuts an encode at sub_dim 8 into (two waves per SIMD, one centroid group); the pipelined
    kernel runs when ceil(steps / chunks) >= K_PIPE_MIN_STEPS."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, (cus * WAVES_PER_BLOCK * 2) // m)


# ---- the winner at every cell -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _winner_case(sd, k):
    m = 8 if sd != 8 else 64
    rng = np.random.default_rng(100 * sd + k)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    if sd == 8:   # enough rows for chunks of K_PIPE_MIN_STEPS + 1 steps, every centroid at least four times
        n = max(4 * k, 32 * (K_PIPE_MIN_STEPS + 1) * _sd8_chunks(m))
    else:
        n = 4 * k
    want = (np.arange(n)[:, None] + 37 * np.arange(m)[None, :]) % k           # row i of subspace s sits on this centroid
    X = cb[np.arange(m)[None, :], want] + (1e-3 * rng.standard_normal((n, m, sd))).astype(F)
    return cb, np.ascontiguousarray(X.reshape(n, m * sd)), want


@pytest.mark.parametrize("k", [256, 225])
@pytest.mark.parametrize("sd", [16, 8, 13])
def test_winner_at_every_cell(sd, k):
    """Row i's nearest centroid is (i + 37 s) mod k by a margin far above T (the next centroid of an N(0,1) codebook is
    more than 0.1 away, the row 1e-3): every index decoding of the two chains' tags occurs in every subspace."""
    cb, X, want = _winner_case(sd, k)
    codes, rechecked, products = _encode_device(cb, X)
    print(f"sd {sd} k {k} n {X.shape[0]}: products {products} rechecked {rechecked}")
    assert products == (6 if sd == 8 else 3)
    for s in range(cb.shape[0]):
        assert set(np.unique(want[:, s]).tolist()) == set(range(k))
    np.testing.assert_array_equal(_oracle(cb, X), want)
    np.testing.assert_array_equal(codes.astype(np.uint32), want)


def test_training_step_sub_dim_8_at_every_cell():
    """The fused-update form at sub_dim 8 runs the four-column grid: assignments of one Lloyd step against the oracle."""
    cb, X, want = _winner_case(8, 256)
    n, m = want.shape
    ds = _lib.Dataset.from_host(X)
    km = _lib.KMeans(ds, m, 256)
    km.set_centroids(cb)
    km.step()
    assert _lib.last_assign_stats()[1] == _lib.ENGINE_MFMA_BF16 and _lib.last_screen_products() == 6
    assign = km.get_assignments()
    km.close()
    ds.close()
    np.testing.assert_array_equal(assign.astype(np.uint32), want)


# ---- the runner-up in every relation to the winner -----------------------------------------------------------------

DISTANCES = [1, 2, 4, 8, 16, 32, 64, 128, 4 + 8, 8 + 32]
RELATIONS = ["same", "up", "down"]   # the later twin: identical, or 1 ulp above / below the earlier one in one coordinate


N_TWIN_SUBSPACES = len(DISTANCES) * len(RELATIONS)


@functools.lru_cache(maxsize=None)
def _twins(sd, n):
    k, m = 256, N_TWIN_SUBSPACES
    rng = np.random.default_rng(17 + sd)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    X = np.empty((n, m, sd), F)
    for s in range(m):
        dist, rel = DISTANCES[s // len(RELATIONS)], RELATIONS[s % len(RELATIONS)]
        used, later = set(), []
        for j in range(k - dist):            # disjoint pairs (j, j + dist)
            if j in used or j + dist in used:
                continue
            used.update((j, j + dist))
            cb[s, j + dist] = cb[s, j]
            t = j % sd
            if rel != "same":
                cb[s, j + dist, t] = np.nextafter(cb[s, j, t], F(9.0) if rel == "up" else F(-9.0))
            later.append(j + dist)
        later = np.array(later)
        X[:, s, :] = cb[s, later[(np.arange(n) + s) % len(later)]]    # every row sits ON a later twin
    return cb, np.ascontiguousarray(X.reshape(n, m * sd))


@pytest.mark.parametrize("sd", [16, 8])
def test_twin_centroids_in_every_relation(sd):
    """Every (row, subspace) is a planted tie: the twin is identical (the oracle takes the earlier one) or 1 ulp away
    in one coordinate (the row's own, later twin is at distance 0), at index distances that put the two in one row
    class (1, 2), one column class (16, 32, 64, 128), the other lane half (4, 4 + 8) or across both (8, 8 + 32).  The screen
    cannot tell twins apart, so every entry must reach the exact re-check -- a reduce that lost the second minimum of its
    row chain or of its column chain proves such rows and fails both assertions."""
    # sub_dim 16: any 1024 rows take the pipelined form; sub_dim 8: chunks of exactly K_PIPE_MIN_STEPS steps
    n = 1024 if sd == 16 else 32 * K_PIPE_MIN_STEPS * _sd8_chunks(N_TWIN_SUBSPACES)
    cb, X = _twins(sd, n)
    m = cb.shape[0]
    codes, rechecked, products = _encode_device(cb, X)
    print(f"twins sd {sd}: products {products} rechecked {rechecked} of {n * m} planted ties")
    assert products == (6 if sd == 8 else 3)
    assert rechecked >= n * m
    np.testing.assert_array_equal(codes.astype(np.uint32), _oracle(cb, X))


# ---- row counts at the pipeline's edges ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ragged(m, k, sd, n):
    """n rows of N(0,1) with a twin per eight centroids; the shorter cases take its first rows."""
    rng = np.random.default_rng(5 + sd)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    for j in range(0, k - 1, 8):
        cb[:, j + 1] = cb[:, j]
        cb[:, j + 1, j % sd] = np.nextafter(cb[:, j, j % sd], F(9.0))
    X = rng.standard_normal((n, m * sd)).astype(F)
    X[::7, :sd] = cb[0, 8 * (np.arange(0, n, 7) % (k // 8)) + 1]     # rows on twins in subspace 0
    cb.setflags(write=False)
    X.setflags(write=False)
    return cb, X, _oracle(cb, X)


@pytest.mark.parametrize("n", [224, 225, 256, 257, 287, 40_013])
def test_row_counts_three_products(n):
    """225 and 256 rows are one chunk of exactly K_PIPE_MIN_STEPS steps, the shortest input of the three-product form (224
    rows, seven steps, stay on six products); 257 and 287 rows end in a partial step and make an odd step count (the
    dummy step); 40 013 rows run many chunks, both step parities and a ragged last step."""
    cb, X, want = _ragged(8, 256, 16, 40_013)
    codes, rechecked, products = _encode_device(cb, X[:n])
    print(f"n {n}: products {products} rechecked {rechecked}")
    assert products == (3 if (n + 31) // 32 >= K_PIPE_MIN_STEPS else 6)
    assert rechecked > 0
    np.testing.assert_array_equal(codes.astype(np.uint32), want[:n])


@pytest.mark.parametrize("edge", ["first", "eight", "eight+1", "eight+31"])
def test_row_counts_sub_dim_8(edge):
    """sub_dim 8, m = 64: the launcher cuts C = _sd8_chunks(m) row chunks and takes the pipelined kernel from
    ceil(steps / C) >= 8 on, i.e. from 7 C + 1 steps (chunks of 8 steps, the last ones short or empty); then exactly 8
    steps in every chunk, one row more (chunks of 9 steps: the dummy step) and a ragged last step."""
    m = 64
    C = _sd8_chunks(m)
    n = {"first": 32 * (7 * C) + 1, "eight": 32 * 8 * C, "eight+1": 32 * 8 * C + 1, "eight+31": 32 * 8 * C + 31}[edge]
    cb, X, want = _ragged(m, 256, 8, 32 * 8 * C + 31)
    codes, rechecked, products = _encode_device(cb, X[:n])
    print(f"sub_dim 8 {edge}: n {n} chunks {C} products {products} rechecked {rechecked}")
    assert products == 6
    np.testing.assert_array_equal(codes.astype(np.uint32), want[:n])


# ---- the re-checked share ---------------------------------------------------------------------------------------------

def test_recheck_share_on_normal_rows():
    """The N(0,1) shape of tests/test_gpu_screen3.py: under the suite's cap of 5 % of n m.  The two tagged chains
    re-checked 1191 entries here (0.372 %) and so does the grid reduce; the two can differ only by rows within the tags'
    perturbation of T."""
    n, m, k, sd = 40_000, 8, 256, 16
    rng = np.random.default_rng(3)
    cb = rng.standard_normal((m, k, sd)).astype(F)
    X = rng.standard_normal((n, m * sd)).astype(F)
    codes, rechecked, products = _encode_device(cb, X)
    print(f"N(0,1): rechecked {rechecked} of {n * m} ({100.0 * rechecked / (n * m):.3f} %)")
    assert products == 3
    assert rechecked < 0.05 * n * m
    np.testing.assert_array_equal(codes.astype(np.uint32), _oracle(cb, X))
