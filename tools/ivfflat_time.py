"""Inverted-file flat search rates (vq_amd.IVFFlatIndex, vq_amd/csrc/k_ivfflat.hip) on one MI355X; prints one JSON line per
shape.

The set is tools/ivf_time.py's: 1M x 128 f32 rows around 4096 seeded Gaussian centres; the index: IVFFlatIndex.train on
256K of its rows (nlist = 1024 coarse centroids, Euclidean), then add of every row, once with f32 and once with f16 rows.
Per (nprobe, nq, topk): the device form (queries and results on the device, HIP-event ms per call, median of --reps)
alternated in the same process with FlatIndex.search_device over the same rows (three alternations, the median of their
medians), the probe alone, the positions the call scans (sum over queries of |S(q)|), the distance pass's packed-f32
VALU bound -- 3 unfused operations per (position, dimension) at 256 CUs x 4 SIMDs x 16 lanes x 2 (packed) x 2.4 GHz --
and recall@10 against the exact search.  The split of a call into its kernels comes from a kernel trace of --quick
(rocprofv3 --kernel-trace --stats, a run of its own with no counters).

    python tools/ivfflat_time.py [--reps 5] [--quick] [--dtype float32|float16|both] [--out profiles/ivfflat/time.json]
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
from ivf_time import clustered, event_ms  # noqa: E402
from vq_amd import _lib  # noqa: E402

VALU_OPS_PER_S = 256 * 4 * 16 * 2 * 2.4e9


def shape(ix, flat_rows, flat_coarse, Q, nprobe, nq, topk, reps, sizes, exact, alternations=3):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    fidx, fdist = torch.empty_like(idx), torch.empty_like(dist)
    ivf, flat = [], []
    for _ in range(alternations):
        ivf.append(event_ms(lambda: ix.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), reps))
        flat.append(event_ms(lambda: flat_rows.search_device(q.data_ptr(), nq, topk, fidx.data_ptr(), fdist.data_ptr()), reps))
    ms, flat_ms = float(np.median(ivf)), float(np.median(flat))
    pi = torch.empty((nq, nprobe), dtype=torch.int32, device="cuda")
    pd = torch.empty((nq, nprobe), dtype=torch.float32, device="cuda")
    probe_ms = event_ms(lambda: flat_coarse.search_device(q.data_ptr(), nq, nprobe, pi.data_ptr(), pd.data_ptr()), reps)
    positions = int(sizes[pi.cpu().numpy().view(np.uint32)].sum())
    got = idx.cpu().numpy().view(np.uint32)[:, :10]
    return {"n": len(ix), "dim": ix.dim, "dtype": ix.dtype.name, "nlist": ix.nlist, "nprobe": nprobe, "nq": nq, "topk": topk,
            "ms": round(ms, 4), "flat_ms": round(flat_ms, 4), "speedup": round(flat_ms / ms, 2), "ms_runs": [round(v, 4) for v in ivf],
            "flat_ms_runs": [round(v, 4) for v in flat], "probe_ms": round(probe_ms, 4), "positions": positions,
            "pair_share": round(positions / (nq * len(ix)), 4),
            "valu_bound_ms": round(positions * ix.dim * 3 / VALU_OPS_PER_S * 1e3, 4),
            "recall_at_10": round(float(np.mean([len(set(got[j]) & set(exact[j])) / 10 for j in range(nq)])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="nq = 1024, nprobe = 32, topk = 10, f32 only (for a kernel trace)")
    ap.add_argument("--dtype", default="both", choices=["float32", "float16", "both"])
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
    trained = vq_amd.IVFFlatIndex.train(X[::4], 1024, max_iters=10)
    train_s = time.perf_counter() - t0
    lists = None
    for dtype in (["float32"] if a.quick else ["float32", "float16"] if a.dtype == "both" else [a.dtype]):
        ix = vq_amd.IVFFlatIndex(trained.coarse_centroids, trained.distance, np.dtype(dtype))
        if lists is None:
            ix.add(X)
            lists = ix.list_ids
        else:
            ix.add_rows(lists, X)
        sizes = ix.list_sizes().astype(np.int64)
        flat_coarse = vq_amd.FlatIndex(ix.coarse_centroids)
        flat_rows = vq_amd.FlatIndex(ix.rows)
        exact = flat_rows.search(Q, 10)[0]
        if a.quick:
            emit(shape(ix, flat_rows, flat_coarse, Q, 32, 1024, 10, a.reps, sizes, exact, alternations=1))
            return
        emit({"shape": "index", "dtype": dtype, "n": len(ix), "nlist": ix.nlist, "train_s": round(train_s, 2),
              "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()), "list_size_mean": round(float(sizes.mean()), 1)})
        all_lists = ix.search(Q, topk=10, nprobe=1024)
        emit({"shape": "nprobe = nlist against FlatIndex.search", "dtype": dtype,
              "identical": bool(np.array_equal(all_lists[0], exact)), "recall_at_10": 1.0 if np.array_equal(all_lists[0], exact) else None})
        for nprobe in (1, 8, 32, 128):
            for nq in (1, 64, 1024):
                for topk in (10, 100):
                    emit(shape(ix, flat_rows, flat_coarse, Q, nprobe, nq, topk, a.reps, sizes, exact))
        ix.close()
        del flat_rows, ix
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
