"""ALL-ROWS oracle parity at BASELINE.json's full sizes.

Every row of every configuration is compared with the CPU oracle (the restatement of
src/pq.rs:177-196 and src/tsvq.rs:117-132), not a sample and not the library's own exact
engine: the GPU box has 128 host threads, on which the OpenMP oracle encodes C2 in about a
second.  Rows travel in chunks so host memory stays bounded (the C5 shard is 6.4 GB).

  * C2  1M x 128,  m=8,  k=256, squared L2: codes + f16 reconstruction, and one full Lloyd
        step (assignments, counts exact; centroids within the stated tolerance);
  * C3  1M x 768,  m=96, k=256, cosine: codes;
  * C5  one GPU's shard of the 8-GPU job, 12.5M x 128, m=16, k=256, squared L2: codes;
  * C4  TSVQ depth 8 on 1M x 128: every leaf id and f16 reconstruction (tree equality is
        held by tests/test_gpu_tsvq.py::test_config4_fullsize_depth8).

Round 3 ("parity soft spots"):
  * C2 on CLUSTERED rows (bench.py's mixture of 256 tight Gaussians: > 2 % of the (row, subspace) pairs go through the
    exact re-check and the list-driven update): all codes and one Lloyd step;
  * vqhip_kmeans_run -- the device-gated loop bench.py and fit_codebooks use -- for 10 iterations at C2 against the
    oracle's loop from the same initial rows;
  * a 2.5M-row chunk of the C5 shard under Distance::Euclidean with the f16 reconstruction.
"""
import numpy as np
import pytest

import oracle as O
import ref_centroids as RC
from vq_amd import _lib

pytestmark = pytest.mark.gpu


def _trained_codebooks(ds, m, k, iters=2):
    n = ds.n
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    for _ in range(iters):
        km.step()
    cb = km.get_centroids()
    km.close()
    return cb


def _encode_all_rows_vs_oracle(oracle, n, d, m, k, metric, chunk, want_f16):
    import torch

    ds = _lib.Dataset.synthetic(n, d, seed=66)
    cb = _trained_codebooks(ds, m, k)
    enc = _lib.PQEncoder(cb, metric)
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    f16 = torch.empty((n, d), dtype=torch.float16, device="cuda") if want_f16 else None
    enc.encode_device(ds.device_ptr, n, codes.data_ptr(), f16.data_ptr() if want_f16 else None)
    _lib.synchronize()
    torch.cuda.synchronize()
    rechecked, engine = _lib.last_assign_stats()
    if metric != _lib.MANHATTAN:
        assert engine == _lib.ENGINE_MFMA_BF16  # the path under test is the screened one
    bad = 0
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        X = ds.read(r0, r1 - r0)
        want, want16 = oracle.pq_encode(metric, X, cb, want_f16=want_f16, threads=0)
        got = codes[r0:r1].cpu().numpy().astype(np.uint32)
        bad += int((got != want).sum())
        if want_f16:
            got16 = f16[r0:r1].cpu().numpy().view(np.uint16)
            bad += int((got16 != want16).sum())
        del X, want, want16, got
    enc.close()
    ds.close()
    assert bad == 0, f"{bad} codes / f16 values differ from the oracle over all {n} rows"
    return rechecked


def test_c2_all_rows_codes_and_f16(oracle):
    """BASELINE configs[1]: every one of the 8M codes and 128M f16 values."""
    r = _encode_all_rows_vs_oracle(oracle, 1_000_000, 128, 8, 256, _lib.SQUARED_EUCLIDEAN, 1_000_000, True)
    assert r < 0.05 * 8_000_000


def test_c2_all_rows_euclidean(oracle):
    """the sqrt metric (Distance::Euclidean, the pyvq default) over all rows"""
    _encode_all_rows_vs_oracle(oracle, 1_000_000, 128, 8, 256, _lib.EUCLIDEAN, 1_000_000, False)


def test_c3_all_rows_cosine(oracle):
    """BASELINE configs[2] at its full 1M x 768 (96M cosine codes)."""
    _encode_all_rows_vs_oracle(oracle, 1_000_000, 768, 96, 256, _lib.COSINE, 250_000, False)


def test_c5_shard_all_rows(oracle):
    """BASELINE configs[4], the rows one of the 8 GPUs holds: 12.5M x 128, m=16 (200M codes)."""
    _encode_all_rows_vs_oracle(oracle, 12_500_000, 128, 16, 256, _lib.SQUARED_EUCLIDEAN, 2_500_000, False)


def test_c2_lloyd_step_all_rows(oracle):
    """One full-size Lloyd iteration: all 8M training assignments and all counts equal the
    oracle's (vector.rs:417-447); centroids within |d| <= 1e-5 max(1,|c|)."""
    n, d, m, k = 1_000_000, 128, 8, 256
    sd = d // m
    ds = _lib.Dataset.synthetic(n, d, seed=66)
    X = ds.read()
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    km.step()                      # move off the init rows so the second step is a generic one
    c_in = km.get_centroids()
    counts, changed = km.step()
    assign = km.get_assignments()
    c_out = km.get_centroids()
    km.close()
    ds.close()
    for s in range(m):
        c1, a_ref, n_ref, ch_ref = oracle.lloyd_step(X[:, s * sd:(s + 1) * sd], c_in[s], threads=0)
        assert int((assign[:, s].astype(np.uint32) != a_ref).sum()) == 0
        np.testing.assert_array_equal(counts[s], n_ref)
        assert bool(changed[s]) == ch_ref
        err = np.max(np.abs(c_out[s] - c1) / np.maximum(1.0, np.abs(c1)))
        assert err <= 1e-5, f"subspace {s}: centroid deviation {err:g}"
        RC.assert_centroids(X[:, s * sd:(s + 1) * sd], a_ref, c_out[s], c1.shape[0], what=f"subspace {s}")  # f64 mean, L = c


def test_c4_every_leaf(oracle):
    """BASELINE configs[3]: every one of the 1M rows descends to the oracle's leaf and gets the
    oracle's f16 reconstruction, for squared L2 and Euclidean (the screened descent) and
    for cosine / Manhattan."""
    from vq_amd import Distance, TSVQ

    from vq_amd.tsvq import build_tree

    n, d, depth = 1_000_000, 128, 8
    ds = _lib.Dataset.synthetic(n, d, seed=66)
    X = ds.read()
    cent, left, right = build_tree(ds, depth)
    ds.close()
    tree = dict(centroids=cent, left=left, right=right)
    for name, metric, f16 in (("squared_euclidean", O.SQUARED_EUCLIDEAN, True), ("euclidean", O.EUCLIDEAN, False),
                              ("cosine", O.COSINE, False), ("manhattan", O.MANHATTAN, False)):
        tq = TSVQ.from_tree(cent, left, right, Distance(name))
        want_leaf, want16 = oracle.tsvq_encode(metric, X, tree, want_f16=f16, threads=0)
        got = tq.leaf_ids(X)
        assert int((got != want_leaf).sum()) == 0, name
        if f16:
            got16 = tq.quantize_batch(X).view(np.uint16)
            assert int((got16 != want16).sum()) == 0


def test_c4_zero_mean_rows_build_and_every_leaf(oracle):
    """BASELINE configs[3]'s shape on ZERO-MEAN rows (N(0,1)): the column sums of the mean passes are random walks that
    change binade all the time -- the hard case of the build's exact emulation (no sampled guesses for
    such columns, 10-29 % of the mean passes' 64-row segments re-added) and, with cosines of either sign, of the cosine
    descent's clamp rules.  The whole tree and every leaf against the oracle."""
    from vq_amd import Distance, TSVQ

    from vq_amd.tsvq import build_tree

    n, d, depth = 1_000_000, 128, 8
    X = np.random.default_rng(77).standard_normal((n, d), dtype=np.float32)
    ds = _lib.Dataset.from_host(X)
    cent, left, right = build_tree(ds, depth)
    ds.close()
    want = oracle.tsvq_build(X, depth)
    np.testing.assert_array_equal(left, want["left"])
    np.testing.assert_array_equal(right, want["right"])
    assert cent.tobytes() == want["centroids"].tobytes()
    for name, metric in (("squared_euclidean", O.SQUARED_EUCLIDEAN), ("cosine", O.COSINE), ("manhattan", O.MANHATTAN)):
        tq = TSVQ.from_tree(cent, left, right, Distance(name))
        want_leaf, _ = oracle.tsvq_encode(metric, X, want, want_f16=False, threads=0)
        got = tq.leaf_ids(X)
        assert int((got != want_leaf).sum()) == 0, name
        assert tq.last_encode_stats()[0]


def _clustered_rows(n, d, k, seed=66):
    """bench.py's clustered data: k centres in [0,1)^d, rows = centre + 0.02 N(0,1) (near-tied centroids inside a blob)"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = torch.rand((k, d), device="cuda", generator=g)
    which = torch.randint(0, k, (n,), device="cuda", generator=g)
    X = (centers[which] + 0.02 * torch.randn((n, d), device="cuda", generator=g)).contiguous()
    torch.cuda.synchronize()
    return X


def test_c2_clustered_rows_codes_and_lloyd_step(oracle):
    """The recheck-heavy regime at full size against the ORACLE (round 2 checked it library-vs-library only): every code of
    an encode pass, and every assignment / count / centroid of a Lloyd step whose update runs through the fused
    accumulation PLUS k_accumulate_listed for the re-checked rows."""
    import torch

    n, d, m, k = 1_000_000, 128, 8, 256
    sd = d // m
    Xd = _clustered_rows(n, d, k)
    ds = _lib.Dataset.from_device(Xd.data_ptr(), n, d)
    X = Xd.cpu().numpy()
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    for _ in range(3):
        km.step()
    c_in = km.get_centroids()
    counts, changed = km.step()
    rechecked, engine = _lib.last_assign_stats()
    assert engine == _lib.ENGINE_MFMA_BF16 and rechecked >= 0.02 * n * m, rechecked  # the regime this test is about
    assign = km.get_assignments()
    c_out = km.get_centroids()
    km.close()
    for s in range(m):
        c1, a_ref, n_ref, ch_ref = oracle.lloyd_step(X[:, s * sd:(s + 1) * sd], c_in[s], threads=0)
        assert int((assign[:, s].astype(np.uint32) != a_ref).sum()) == 0
        np.testing.assert_array_equal(counts[s], n_ref)
        assert bool(changed[s]) == ch_ref
        err = np.max(np.abs(c_out[s] - c1) / np.maximum(1.0, np.abs(c1)))
        assert err <= 1e-5, f"subspace {s}: centroid deviation {err:g}"
        RC.assert_centroids(X[:, s * sd:(s + 1) * sd], a_ref, c_out[s], c1.shape[0], what=f"subspace {s}")  # f64 mean, L = c
    enc = _lib.PQEncoder(c_out, _lib.SQUARED_EUCLIDEAN)
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    enc.encode_device(Xd.data_ptr(), n, codes.data_ptr(), None)
    _lib.synchronize()
    assert _lib.last_assign_stats()[0] >= 0.02 * n * m
    want, _ = oracle.pq_encode(O.SQUARED_EUCLIDEAN, X, c_out, want_f16=False, threads=0)
    assert int((codes.cpu().numpy().astype(np.uint32) != want).sum()) == 0
    enc.close()
    ds.close()


def test_c2_normal_rows_codes_and_lloyd_step(oracle):
    """Zero-mean rows (N(0,1), what real embeddings look like; the other all-rows PQ checks are Uniform[0,1) or a clustered
    mixture): every assignment / count / centroid of a Lloyd step and every code of an encode pass, squared L2 and cosine
    (cosine on zero-mean rows is the case where the best cosine of many rows is barely positive)."""
    import torch

    n, d, m, k = 1_000_000, 128, 8, 256
    sd = d // m
    g = torch.Generator(device="cuda")
    g.manual_seed(4242)
    Xd = torch.randn((n, d), device="cuda", generator=g, dtype=torch.float32)
    ds = _lib.Dataset.from_device(Xd.data_ptr(), n, d)
    X = Xd.cpu().numpy()
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    for _ in range(2):
        km.step()
    c_in = km.get_centroids()
    counts, changed = km.step()
    assert _lib.last_assign_stats()[1] == _lib.ENGINE_MFMA_BF16
    assign = km.get_assignments()
    c_out = km.get_centroids()
    km.close()
    for s in range(m):
        c1, a_ref, n_ref, ch_ref = oracle.lloyd_step(X[:, s * sd:(s + 1) * sd], c_in[s], threads=0)
        assert int((assign[:, s].astype(np.uint32) != a_ref).sum()) == 0
        np.testing.assert_array_equal(counts[s], n_ref)
        assert bool(changed[s]) == ch_ref
        err = np.max(np.abs(c_out[s] - c1) / np.maximum(1.0, np.abs(c1)))
        assert err <= 1e-5, f"subspace {s}: centroid deviation {err:g}"
        RC.assert_centroids(X[:, s * sd:(s + 1) * sd], a_ref, c_out[s], c1.shape[0], what=f"subspace {s}")  # f64 mean, L = c
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    for lib_metric, o_metric in ((_lib.SQUARED_EUCLIDEAN, O.SQUARED_EUCLIDEAN), (_lib.COSINE, O.COSINE)):
        enc = _lib.PQEncoder(c_out, lib_metric)
        enc.encode_device(Xd.data_ptr(), n, codes.data_ptr(), None)
        _lib.synchronize()
        want, _ = oracle.pq_encode(o_metric, X, c_out, want_f16=False, threads=0)
        assert int((codes.cpu().numpy().astype(np.uint32) != want).sum()) == 0, lib_metric
        enc.close()
    ds.close()


def test_c2_kmeans_run_10_iterations(oracle):
    """vqhip_kmeans_run (iterations queued back to back, decisions on the device) at C2 for 10 iterations from the
    bench's strided initial rows, against the oracle's Lloyd loop from the same rows (vector.rs:415-458): iteration
    counts equal, final inertia within 0.1 % (trajectories may part at boundary rows: the centroid tolerance), and
    every assignment of the LAST iteration equal to the oracle's given the run's own centroids going into it."""
    n, d, m, k, iters = 1_000_000, 128, 8, 256, 10
    sd = d // m
    ds = _lib.Dataset.synthetic(n, d, seed=66)
    X = ds.read()
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    it, _, _, paused = km.run(iters - 1)
    assert not paused and it.tolist() == [iters - 1] * m
    c_before = km.get_centroids()
    it, counts, changed, paused = km.run(1)
    assert not paused and it.tolist() == [1] * m
    assign = km.get_assignments()
    c_gpu = km.get_centroids()
    km.close()
    ds.close()

    def inertia(xs, cs, a):
        diff = xs - cs[a]
        return float(np.einsum("ij,ij->", diff, diff, dtype=np.float64))

    for s in range(m):
        xs = X[:, s * sd:(s + 1) * sd]
        # the last iteration, from the run's own centroids: exact assignments and counts, centroids within tolerance
        c1, a_ref, n_ref, ch_ref = oracle.lloyd_step(xs, c_before[s], threads=0)
        assert int((assign[:, s].astype(np.uint32) != a_ref).sum()) == 0
        np.testing.assert_array_equal(counts[s], n_ref)
        assert bool(changed[s]) == ch_ref
        assert np.max(np.abs(c_gpu[s] - c1) / np.maximum(1.0, np.abs(c1))) <= 1e-5
        RC.assert_centroids(xs, a_ref, c_gpu[s], c1.shape[0], what=f"subspace {s}")  # f64 mean, L = c
        # the whole trajectory: the oracle's loop from the same initial rows
        c_ref, it_ref, _ = oracle.lloyd(xs, k, iters, init[s], threads=0)
        assert it_ref == iters
        i_gpu = inertia(xs, c_gpu[s], a_ref)
        _, a_end, _, _ = oracle.lloyd_step(xs, c_ref, threads=0)
        i_ref = inertia(xs, c_ref, a_end)
        assert abs(i_gpu - i_ref) <= 1e-3 * i_ref, (s, i_gpu, i_ref)


def test_c5_chunk_euclidean_with_f16(oracle):
    """BASELINE configs[4]'s shape (d = 128, m = 16: sub_dim 8, two waves per SIMD) under Distance::Euclidean -- the sqrt
    collapses near-ties onto the earlier index -- with the f16 reconstruction, on 2.5M rows of the shard."""
    _encode_all_rows_vs_oracle(oracle, 2_500_000, 128, 16, 256, _lib.EUCLIDEAN, 1_250_000, True)


def test_c1_at_its_ten_thousand_rows(oracle):
    """BASELINE configs[0] at its own size (PQ m=4 k=16 Euclidean on 10k x 64; VERDICT r3 "C1 runs at n = 3000 / 4096"):
    the whole fit from injected draws -- vqhip_kmeans_run's trajectory, iteration counts included -- and the encode of
    every row with f16, against the oracle's loop (src/pq.rs:83-141, 167-199)."""
    import vq_amd as pyvq

    n, d, m, k, iters = 10_000, 64, 4, 16, 10
    X = _lib.synth_uniform_host(n, d, seed=66)
    rng = np.random.default_rng(5)
    init = np.stack([rng.choice(n, k, replace=False) for _ in range(m)]).astype(np.uint64)
    reseed = rng.integers(0, n, (m, 64)).astype(np.uint64)
    want_cb, want_iters = oracle.pq_fit(X, m, k, iters, init, reseed, threads=0)
    for exact in (True, False):
        pq = pyvq.ProductQuantizer(X, m, k, iters, pyvq.Distance.euclidean(), 42, init_rows=init, reseed_rows=reseed,
                                   exact_update=exact)
        if exact:  # sums in the reference's row order: the trajectory is the oracle's bit for bit
            np.testing.assert_array_equal(pq.codebooks, want_cb)
            np.testing.assert_array_equal(pq.fit_stats["iters"], want_iters)
        # (default blocked sums: each step is within 1e-5 of the oracle's from the same centroids, tests/test_gpu_parity.py;
        # ten steps on may part ways at a tie, so only the encode below is held to the oracle for that fit)
        codes = pq.encode(X)
        f16 = pq.quantize_batch(X)
        want_c, want_f = oracle.pq_encode(O.EUCLIDEAN, X, pq.codebooks, threads=0)
        np.testing.assert_array_equal(codes.astype(np.uint32), want_c)
        np.testing.assert_array_equal(f16.view(np.uint16), want_f)


def _lloyd_step_all_rows_vs_oracle(oracle, n, d, m, k, chunk, run_iters=0):
    """One generic full-size Lloyd iteration (after a warm-up step off the initial rows) with every assignment, count and
    `changed` flag equal to the oracle's (vector.rs:417-447); with `run_iters`, additionally vqhip_kmeans_run for that
    many iterations whose LAST iteration is checked the same way from the run's own centroids going into it; finally the
    same step with `exact_update` (the reference's sum order): centroids BIT-equal to the oracle's.

    Centroids of the default (blocked f32 + f64) update: |gpu - oracle| <= 1e-5 max(1,|c|) up to clusters of ~30k
    members; the reference's own sequential f32 sum carries an error of ~sqrt(members) 2^-24 relative (1.3e-5 at the
    C5 shard's 49k members per cluster), so beyond that the bound is the triangle inequality through the f64 mean of the
    oracle's own assignment: |gpu - mean64| <= 2e-6 max(1,|c|) (the GPU is the closer of the two) and
    |gpu - oracle| <= 1e-5 max(1,|c|) + |oracle - mean64|.  The rows come to the host in chunks."""
    sd = d // m
    ds = _lib.Dataset.synthetic(n, d, seed=66)
    km = _lib.KMeans(ds, m, k)
    init = np.array([[(j * (n // k) + s) % n for j in range(k)] for s in range(m)], np.uint64)
    km.init_from_rows(init)
    km.step()
    stages = []
    c_in = km.get_centroids()
    counts, changed = km.step()
    assert _lib.last_assign_stats()[1] == _lib.ENGINE_MFMA_BF16
    stages.append((c_in, counts.copy(), np.array(changed).copy(), km.get_assignments(), km.get_centroids(), False))
    if run_iters:
        it, _, _, paused = km.run(run_iters - 1)
        assert not paused and it.tolist() == [run_iters - 1] * m
        c_in2 = km.get_centroids()
        it, counts, changed, paused = km.run(1)
        assert not paused and it.tolist() == [1] * m
        stages.append((c_in2, counts.copy(), np.array(changed).copy(), km.get_assignments(), km.get_centroids(), False))
    # the same generic step in the reference's summation order
    km.set_centroids(c_in)
    km.set_active(np.ones(m, np.uint8))
    km.set_exact_update(True)
    counts, changed = km.step()
    stages.append((c_in, counts.copy(), np.array(changed).copy(), km.get_assignments(), km.get_centroids(), True))
    km.close()
    X = np.empty((n, d), np.float32)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        X[r0:r1] = ds.read(r0, r1 - r0)
    ds.close()
    worst = 0.0
    for s in range(m):
        xs = np.ascontiguousarray(X[:, s * sd:(s + 1) * sd])
        memo = {}
        for c_in, counts, changed, assign, c_out, exact in stages:
            key = c_in[s].tobytes()
            if key not in memo:
                memo[key] = oracle.lloyd_step(xs, c_in[s], threads=0)
            c1, a_ref, n_ref, ch_ref = memo[key]
            assert int((assign[:, s].astype(np.uint32) != a_ref).sum()) == 0, s
            np.testing.assert_array_equal(counts[s], n_ref)
            assert bool(changed[s]) == ch_ref
            if exact:
                assert c_out[s].tobytes() == c1.tobytes(), f"subspace {s}: exact_update centroids differ from the oracle's bits"
                continue
            err = float(np.max(np.abs(c_out[s] - c1) / np.maximum(1.0, np.abs(c1))))
            worst = max(worst, err)
            if err <= 1e-5:
                continue
            mean64 = np.stack([np.bincount(a_ref, weights=xs[:, t].astype(np.float64), minlength=k) for t in range(sd)], axis=1)
            mean64 /= np.maximum(1, n_ref)[:, None]
            live = n_ref > 0
            scale = np.maximum(1.0, np.abs(mean64[live]))
            e_gpu = float(np.max(np.abs(c_out[s][live] - mean64[live]) / scale))
            e_orc = float(np.max(np.abs(c1[live] - mean64[live]) / scale))
            assert e_gpu <= 2e-6, f"subspace {s}: GPU centroids {e_gpu:g} from the f64 mean"
            assert err <= 1e-5 + e_orc, f"subspace {s}: centroid deviation {err:g} (oracle's own {e_orc:g})"
    return worst


def test_c3_lloyd_step_all_rows(oracle):
    """BASELINE configs[2]'s training half at its full 1M x 768, m = 96 (sub_dim 8: the two-waves-per-SIMD fused-update
    screen with the subspace-major code scratch; VERDICT r4 "What's weak 2"): a generic step, then vqhip_kmeans_run for
    3 iterations with the last one checked -- 96M assignments each."""
    _lloyd_step_all_rows_vs_oracle(oracle, 1_000_000, 768, 96, 256, 250_000, run_iters=3)


def test_c5_shard_lloyd_step_all_rows(oracle):
    """BASELINE configs[4]'s training half on the rows one of the 8 GPUs holds: 12.5M x 128, m = 16 (200M assignments)."""
    _lloyd_step_all_rows_vs_oracle(oracle, 12_500_000, 128, 16, 256, 2_500_000)
