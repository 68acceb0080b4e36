"""Scalar index search rates (vq_amd.ScalarIndex, vq_amd/csrc/k_sqindex.hip) on one MI355X beside FlatIndex over the
dequantized f32 rows, measured alternately in one process; prints one JSON line per shape.

Each shape: both indexes warmed, then --reps rounds of (scalar call, flat call), each call between two HIP events on
the stream the library launches on; the medians, the spread (max - min) / median of each side's repeats, and the ratio
scalar / flat.  The target shape -- 1024 queries over 1M x 128 under Euclidean -- also carries `within_margin`: the
scalar median is at most the flat median times (1 + margin), the margin being the flat spread of that run and at least
5 %.  Search uses the device form (queries and results on the device); rerank (1024 x 1024 candidates) the host form,
timed by the wall clock.  The VALU bound is tools/knn_time.py's: 3 unfused operations per (query, row, dimension) for
Euclidean at 7.86e13 packed lane-operations/s.

    python tools/sqindex_time.py [--reps 7] [--quick] [--out profiles/sqindex/time.json]
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

PACKED_LANE_OPS = 2 * 256 * 4 * 16 * 2.4e9


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream())
    fn()
    b.record(torch.cuda.current_stream())
    b.synchronize()
    return a.elapsed_time(b)


def _wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(scalar_fn, flat_fn, reps, clock):
    """warm both, then reps rounds of (scalar, flat); per side: median ms, spread = (max - min) / median"""
    scalar_fn()
    flat_fn()
    torch.cuda.synchronize()
    s, f = [], []
    for _ in range(reps):
        s.append(clock(scalar_fn))
        f.append(clock(flat_fn))
    out = {}
    for name, t in (("scalar", s), ("flat", f)):
        med = float(np.median(t))
        out[name + "_ms"] = round(med, 3)
        out[name + "_spread"] = round((max(t) - min(t)) / med, 4)
        out[name + "_all_ms"] = [round(v, 3) for v in t]
    out["scalar_over_flat"] = round(out["scalar_ms"] / out["flat_ms"], 4)
    return out


def make(n, d, seed):
    rng = np.random.default_rng(seed)
    q = vq_amd.ScalarQuantizer(-1.0, 1.0, 256)
    codes = rng.integers(0, 256, (n, d), dtype=np.uint8)
    dist = vq_amd.Distance.euclidean()
    six = vq_amd.ScalarIndex.from_codes(codes, q, dist)
    flat = vq_amd.FlatIndex(q.dequantize_batch(codes), dist)
    return six, flat


def search_shape(six, flat, nq, topk, reps):
    n, d = len(six), six.dim
    q = torch.rand((nq, d), device="cuda") * 2 - 1
    bufs = [(torch.empty((nq, topk), dtype=torch.int32, device="cuda"), torch.empty((nq, topk), dtype=torch.float32, device="cuda"))
            for _ in range(2)]
    r = alternate(lambda: six.search_device(q.data_ptr(), nq, topk, bufs[0][0].data_ptr(), bufs[0][1].data_ptr()),
                  lambda: flat.search_device(q.data_ptr(), nq, topk, bufs[1][0].data_ptr(), bufs[1][1].data_ptr()), reps, _event_ms)
    torch.cuda.synchronize()
    same = bool(torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1].view(torch.int32), bufs[1][1].view(torch.int32)))
    bound_ms = nq * n * d * 3 / PACKED_LANE_OPS * 1e3
    return {"shape": "search", "n": n, "d": d, "metric": "euclidean", "nq": nq, "topk": topk, **r,
            "results_equal": same, "valu_bound_ms": round(bound_ms, 3),
            "scalar_fraction_of_valu_bound": round(bound_ms / r["scalar_ms"], 3),
            "index_bytes": {"scalar": n * d, "flat": 4 * n * d}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the 1M x 128, 1024-query shape only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()  # the library's launches on the stream the events time
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    n = 1 << 20
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    six, flat = make(n, 128, 1)
    r = search_shape(six, flat, 1024, 10, a.reps)
    margin = max(r["flat_spread"], 0.05)
    r["target"] = {"margin": round(margin, 4), "within_margin": bool(r["scalar_ms"] <= r["flat_ms"] * (1 + margin))}
    emit(r)
    if not a.quick:
        for nq in (1, 64):
            emit(search_shape(six, flat, nq, 10, a.reps))
        rng = np.random.default_rng(0)
        Q = (rng.random((1024, 128), dtype=np.float32) * 2 - 1).astype(np.float32)
        cand = np.stack([rng.permutation(n)[:1024] for _ in range(1024)]).astype(np.uint32)
        rr = alternate(lambda: six.rerank(Q, cand, 10), lambda: flat.rerank(Q, cand, 10), a.reps, _wall_ms)
        gs, gf = six.rerank(Q, cand, 10), flat.rerank(Q, cand, 10)
        emit({"shape": "rerank (host form: queries and ids in, results out)", "n": n, "d": 128, "metric": "euclidean",
              "nq": 1024, "candidates": 1024, "topk": 10, **rr,
              "results_equal": bool(np.array_equal(gs[0], gf[0]) and np.array_equal(gs[1].view(np.uint32), gf[1].view(np.uint32)))})
        del six, flat
        torch.cuda.empty_cache()
        six, flat = make(n, 768, 2)
        emit(search_shape(six, flat, 256, 10, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
