"""Inverted-file scalar search rates (vq_amd.IVFScalarIndex, vq_amd/csrc/k_ivfsq.hip) on one MI355X beside the f32 inverted-
file flat search over the dequantized rows in the same lists; prints one JSON line per shape.

The set is tools/ivfflat_time.py's: 1M x 128 f32 rows around 4096 seeded Gaussian centres; IVFScalarIndex.train on 256K of
its rows (nlist = 1024 coarse centroids, Euclidean), ScalarQuantizer(min(X), max(X), 256), then add of every row.  The
IVFFlatIndex holds quantizer.dequantize_batch(codes) in the same lists, so both searches return the same bits.  Per
(nprobe, nq): the two device forms (queries and results on the device, HIP-event ms per call) alternated in one process,
five calls each -- the median with the extremes --, the positions the call scans, and within_margin: the scalar
search's median is no more than the flat search's times 1 + margin, the margin being the larger of 5 % and the two
searches' own spreads ((max - min) / median).  recall@10 of both against the exact search over the original rows.  The
split of a call into its kernels comes from a kernel trace of --quick (rocprofv3 --kernel-trace --stats, a run of its own
with no counters).

    python tools/ivfsq_time.py [--reps 5] [--quick] [--out profiles/ivfsq/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from ivf_time import clustered  # noqa: E402
from vq_amd import _lib  # noqa: E402


def event_runs(fn, reps):
    """HIP-event ms of reps calls after one warm-up call"""
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
    return times


def stats(runs):
    return {"median": round(float(np.median(runs)), 4), "min": round(float(min(runs)), 4), "max": round(float(max(runs)), 4)}


def shape(ix, flat, Q, nprobe, nq, topk, reps, sizes, exact):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    fidx, fdist = torch.empty_like(idx), torch.empty_like(dist)
    sq_runs, flat_runs = [], []
    for _ in range(reps):  # alternated call by call
        sq_runs += event_runs(lambda: ix.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), 1)
        flat_runs += event_runs(lambda: flat.search_device(q.data_ptr(), nq, topk, fidx.data_ptr(), fdist.data_ptr(), nprobe=nprobe), 1)
    torch.cuda.synchronize()
    sq, fl = stats(sq_runs), stats(flat_runs)
    spread = max((sq["max"] - sq["min"]) / sq["median"], (fl["max"] - fl["min"]) / fl["median"])
    margin = max(0.05, spread)
    got = idx.cpu().numpy().view(np.uint32)
    same = bool(np.array_equal(got, fidx.cpu().numpy().view(np.uint32)) and torch.equal(dist.view(torch.int32), fdist.view(torch.int32)))
    positions = int(sizes[ix.probe(Q[:nq], nprobe)].sum())
    return {"n": len(ix), "dim": ix.dim, "nlist": ix.nlist, "nprobe": nprobe, "nq": nq, "topk": topk, "ivfsq_ms": sq, "ivfflat_ms": fl,
            "ratio": round(sq["median"] / fl["median"], 3), "margin": round(margin, 3),
            "within_margin": bool(sq["median"] <= fl["median"] * (1 + margin)), "same_bits": same, "positions": positions,
            "recall_at_10": round(float(np.mean([len(set(got[j, :10]) & set(exact[j])) / 10 for j in range(nq)])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="nq = 1024, nprobe = 32 only (for a kernel trace)")
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
    sq = vq_amd.ScalarQuantizer(float(X.min()), float(X.max()), 256)
    t0 = time.perf_counter()
    ix = vq_amd.IVFScalarIndex.train(X[::4], 1024, sq, max_iters=10)
    train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.add(X)
    add_s = time.perf_counter() - t0
    sizes = ix.list_sizes().astype(np.int64)
    flat = vq_amd.IVFFlatIndex(ix.coarse_centroids, ix.distance)
    flat.add_rows(ix.list_ids, sq.dequantize_batch(ix.codes))
    exact = vq_amd.FlatIndex(X).search(Q, 10)[0]
    if a.quick:
        emit(shape(ix, flat, Q, 32, 1024, 10, a.reps, sizes, exact))
        return
    emit({"shape": "index", "n": len(ix), "nlist": ix.nlist, "quantizer": repr(sq), "train_s": round(train_s, 2), "add_s": round(add_s, 2),
          "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()), "list_size_mean": round(float(sizes.mean()), 1)})
    for nprobe in (1, 8, 32, 128):
        for nq in (1, 64, 1024):
            emit(shape(ix, flat, Q, nprobe, nq, 10, a.reps, sizes, exact))
    ix.close()
    flat.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "command": "python tools/ivfsq_time.py " + " ".join(sys.argv[1:]),
                       "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
