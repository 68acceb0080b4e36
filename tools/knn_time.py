"""Exact k-NN search rates (vq_amd.FlatIndex, vq_amd/csrc/k_knn.hip) on one MI355X; prints one JSON line per shape.

Each shape: a warmed index, the device form (queries and results on the device, HIP-event ms per call, median of
--reps), queries/s, and the fraction of the VALU bound.  The bound counts the distance arithmetic alone -- 3 operations
per (query, row, dimension) for squared L2 / Euclidean, 2 for L1 (sub, add of |.|) and cosine (mul, add) -- at the
packed-f32 rate, 2 x 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 7.86e13 lane-operations/s (the compiler emits
v_pk_add_f32 / v_pk_mul_f32 for squared L2 and cosine).  Rerank: 1024 queries x 1024 candidates.  The CPU line:
the numpy statement of the semantics (tests/ref_knn.py), single core, on a few queries.

    python tools/knn_time.py [--reps 5] [--quick] [--out profiles/knn/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402

PACKED_LANE_OPS = 2 * 256 * 4 * 16 * 2.4e9
OPS = {"squared_euclidean": 3, "euclidean": 3, "manhattan": 2, "cosine": 2, "cosine_unclamped": 2}


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


def search_shape(X, metric, nq, topk, reps, label=None):
    n, d = X.shape
    ix = vq_amd.FlatIndex(X, vq_amd.Distance(metric))
    q = torch.rand((nq, d), device="cuda")
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    ms = event_ms(lambda: ix.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr()), reps)
    bound_ms = nq * n * d * OPS[metric] / PACKED_LANE_OPS * 1e3
    return {"shape": label or "search", "n": n, "d": d, "dtype": str(X.dtype), "metric": metric, "nq": nq, "topk": topk,
            "ms": round(ms, 3), "queries_per_s": round(nq / ms * 1e3, 1), "valu_bound_ms": round(bound_ms, 3),
            "fraction_of_valu_bound": round(bound_ms / ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the 1M x 128 Euclidean shape only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()  # the library's launches on the stream the events time
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    n = 1 << 20
    X128 = _lib.synth_uniform_host(n, 128, 1, 0)
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    if a.quick:
        emit(search_shape(X128, "euclidean", 1024, 10, a.reps))
        return
    for metric in OPS:
        for topk in (10, 100):
            emit(search_shape(X128, metric, 1024, topk, a.reps))
    emit(search_shape(X128.astype(np.float16), "euclidean", 1024, 10, a.reps, "search f16 rows"))
    # rerank: 1024 queries x 1024 candidate ids
    ix = vq_amd.FlatIndex(X128)
    rng = np.random.default_rng(0)
    Q = rng.random((1024, 128), dtype=np.float32)
    cand = np.stack([rng.permutation(n)[:1024] for _ in range(1024)]).astype(np.uint32)
    ix.rerank(Q[:1], cand[:1], 10)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ix.rerank(Q, cand, 10)
        t.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(t))
    bound_ms = 1024 * 1024 * 128 * 3 / PACKED_LANE_OPS * 1e3
    emit({"shape": "rerank (host form: queries and ids in, results out)", "n": n, "d": 128, "metric": "euclidean",
          "nq": 1024, "candidates": 1024, "topk": 10, "ms": round(ms, 3), "queries_per_s": round(1024 / ms * 1e3, 1),
          "valu_bound_ms": round(bound_ms, 4), "fraction_of_valu_bound": round(bound_ms / ms, 4)})
    del ix
    for d in (384, 768):
        Xd = _lib.synth_uniform_host(n, d, 2, 0)
        emit(search_shape(Xd, "euclidean", 256, 10, a.reps))
        del Xd
    import ref_knn as K

    t0 = time.perf_counter()
    K.search(K.EUCLIDEAN, Q[:2], X128, 10)
    cpu_ms = (time.perf_counter() - t0) * 1e3 / 2
    emit({"shape": "cpu numpy statement, one core", "n": n, "d": 128, "metric": "euclidean", "topk": 10,
          "ms_per_query": round(cpu_ms, 1), "queries_per_s": round(1e3 / cpu_ms, 2)})
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
