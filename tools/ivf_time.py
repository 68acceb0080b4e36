"""Inverted-file PQ search rates (vq_amd.IVFPQIndex, vq_amd/csrc/k_ivf.hip) on one MI355X; prints one JSON line per shape.

The set: 1M x 128 f32 rows around 4096 seeded Gaussian centres (a clustered set, so that recall means something); the
index: IVFPQIndex.train on 256K of its rows (nlist = 1024 coarse centroids, m = 8, k = 256), then add of every row.  Per
(nprobe, nq, topk): the device form (queries and results on the device, HIP-event ms per call, median of --reps), the
probe alone (the flat search over the centroids, same events), the positions the call scans (sum over queries of
|S(q)|) and the LDS bound of the scan -- m four-byte table reads per position at 256 CUs x 128 B/clk x 2.4 GHz =
78.6 TB/s, the model of DESIGN.md 8.7 --, recall@10 against an exact FlatIndex search of the rows (beside that of the
full ADC scan of the same codes and of the IVF hits reranked exactly), and at nq = 1024 the
host form against PQIndex.search of the same queries (wall ms, median of --reps).  The split of a call into tables,
scan and selection comes from a kernel trace of --quick (rocprofv3 --kernel-trace --stats).  Last: 10M x 128 at
nprobe = 32 (lists drawn with k-means-like unevenness, random codes: the timing does not depend on them).

--residual: the same set, shapes and figures for a residual index (IVFPQIndex.train(..., residual=True): codebooks fit
on the rows' residuals to their lists, rows stored as the codes of x - C[list]); the full ADC scan row is left out (its
codes are residuals), and the non-residual index trained on the same rows is timed beside it at nq = 1024, nprobe 32,
alternating the two.

    python tools/ivf_time.py [--reps 5] [--quick] [--residual] [--out profiles/ivf/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402
from vq_amd.store import PQIndex  # noqa: E402

LDS_BYTES_PER_S = 256 * 128 * 2.4e9


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def clustered(n, d, centres, seed):
    rng = np.random.default_rng(seed)
    C = (rng.standard_normal((centres, d)) * 2.0).astype(np.float32)
    X = np.empty((n, d), np.float32)
    for r0 in range(0, n, 1 << 18):
        r1 = min(n, r0 + (1 << 18))
        X[r0:r1] = C[rng.integers(0, centres, r1 - r0)] + rng.standard_normal((r1 - r0, d)).astype(np.float32)
    Q = C[rng.integers(0, centres, 1024)] + rng.standard_normal((1024, d)).astype(np.float32)
    return X, Q.astype(np.float32)


def shape(ix, flat_coarse, Q, nprobe, nq, topk, reps, sizes, exact=None, label="1M x 128"):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    ms = event_ms(lambda: ix.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), reps)
    pi = torch.empty((nq, nprobe), dtype=torch.int32, device="cuda")
    pd = torch.empty((nq, nprobe), dtype=torch.float32, device="cuda")
    probe_ms = event_ms(lambda: flat_coarse.search_device(q.data_ptr(), nq, nprobe, pi.data_ptr(), pd.data_ptr()), reps)
    P = pi.cpu().numpy().view(np.uint32)
    positions = int(sizes[P].sum())
    bound_ms = positions * ix.m * 4 / LDS_BYTES_PER_S * 1e3
    r = {"shape": label, "n": len(ix), "nlist": ix.nlist, "m": ix.m, "k": ix.k, "nprobe": nprobe, "nq": nq, "topk": topk,
         "ms": round(ms, 4), "queries_per_s": round(nq / ms * 1e3, 1), "probe_ms": round(probe_ms, 4),
         "positions": positions, "scan_lds_bound_ms": round(bound_ms, 4)}
    if exact is not None and topk >= 10:
        got = idx.cpu().numpy().view(np.uint32)[:, :10]
        r["recall_at_10"] = round(float(np.mean([len(set(got[j]) & set(exact[j])) / 10 for j in range(nq)])), 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="nq = 1024, nprobe = 32, topk = 10 only (for a kernel trace)")
    ap.add_argument("--residual", action="store_true", help="a residual index (IVFADC)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()  # the library's launches on the stream the events time
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    X, Q = clustered(1 << 20, 128, 4096, 7)
    t0 = time.perf_counter()
    ix = vq_amd.IVFPQIndex.train(X[::4], 1024, 8, 256, max_iters=10, residual=a.residual)
    train_s = time.perf_counter() - t0
    ix.add(X)
    sizes = ix.list_sizes().astype(np.int64)
    flat_coarse = vq_amd.FlatIndex(ix.coarse_centroids)
    if a.quick:
        emit(shape(ix, flat_coarse, Q, 32, 1024, 10, a.reps, sizes))
        return
    emit({"shape": "index", "residual": ix.residual, "n": len(ix), "nlist": ix.nlist, "train_s": round(train_s, 2),
          "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()), "list_size_mean": round(float(sizes.mean()), 1)})
    flat_rows = vq_amd.FlatIndex(X)
    exact = flat_rows.search(Q, 10)[0]

    def recall(got):
        return round(float(np.mean([len(set(got[j, :10]) & set(exact[j])) / 10 for j in range(got.shape[0])])), 4)

    # what limits recall on this set: the full ADC scan over the same codes, and the IVF hits reranked exactly
    pq = None if ix.residual else PQIndex(ix.codebooks, ix.codes, ix.distance)
    r = {"shape": "recall@10 of 1024 queries against an exact FlatIndex search", "residual": ix.residual}
    if pq is not None:
        r["full_adc_scan"] = recall(pq.search(Q, 10)[0])
    for nprobe in (8, 32):
        r[f"ivf_nprobe_{nprobe}"] = recall(ix.search(Q, topk=10, nprobe=nprobe)[0])
        r[f"ivf_nprobe_{nprobe}_rerank_100"] = recall(ix.search(Q, topk=10, nprobe=nprobe, rerank=flat_rows, candidates=100)[0])
    emit(r)
    del flat_rows
    if ix.residual:  # the non-residual index of the same rows, timed alternately with the residual one
        plain = vq_amd.IVFPQIndex.train(X[::4], 1024, 8, 256, max_iters=10)
        plain.add(X)
        t = {"residual": [], "non_residual": []}
        for _ in range(3):
            t["residual"].append(shape(ix, flat_coarse, Q, 32, 1024, 10, a.reps, sizes)["ms"])
            t["non_residual"].append(shape(plain, flat_coarse, Q, 32, 1024, 10, a.reps, plain.list_sizes().astype(np.int64))["ms"])
        emit({"shape": "device form, 1024 queries, nprobe 32, topk 10: residual against non-residual (3 alternations)",
              "residual_ms": t["residual"], "non_residual_ms": t["non_residual"],
              "ratio": round(float(np.median(t["residual"]) / np.median(t["non_residual"])), 3)})
        plain.close()
        del plain
    for nprobe in (1, 8, 32, 128):
        for nq in (1, 64, 1024):
            for topk in (10, 100):
                emit(shape(ix, flat_coarse, Q, nprobe, nq, topk, a.reps, sizes, exact[:nq]))
    # the host forms at nq = 1024 against a full ADC scan of the same codes
    for topk in ((10, 100) if pq is not None else ()):
        pq_ms = wall_ms(lambda: pq.search(Q, topk), a.reps)
        for nprobe in (8, 32):
            ivf_ms = wall_ms(lambda: ix.search(Q, topk=topk, nprobe=nprobe), a.reps)
            emit({"shape": "host form, 1024 queries: IVF against PQIndex.search", "nprobe": nprobe, "topk": topk,
                  "ivf_ms": round(ivf_ms, 3), "pq_index_ms": round(pq_ms, 3), "speedup": round(pq_ms / ivf_ms, 2)})
    del pq, exact, X
    ix.close()
    # 10M x 128 at nprobe = 32
    rng = np.random.default_rng(10)
    n = 10 * (1 << 20)
    w = rng.gamma(2.0, 1.0, 1024)
    big = vq_amd.IVFPQIndex(ix.coarse_centroids, ix.codebooks, residual=ix.residual)
    big.add_codes(rng.choice(1024, n, p=w / w.sum()).astype(np.uint32), rng.integers(0, 256, (n, 8), dtype=np.uint8))
    bsizes = big.list_sizes().astype(np.int64)
    for nq in (1, 64, 1024):
        emit(shape(big, flat_coarse, Q, 32, nq, 10, a.reps, bsizes, label="10M x 128 (random codes)"))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
