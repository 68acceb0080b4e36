"""Inverted-file range search against the same index's top-k search (vq_amd.IVFFlatIndex, vq_amd.IVFScalarIndex;
vq_amd/csrc/ivf_range.hpp) on one MI355X; prints one JSON line per measurement.

The set is tools/ivfflat_time.py's: 1M x 128 f32 rows around 4096 seeded Gaussian centres, IVFFlatIndex.train on 256K of
its rows (nlist = 1024, Euclidean), then add of every row; IVFScalarIndex holds the same rows in the same lists as SQ
codes.  Per index, nprobe (8, 32), nq (1, 1024) and radius: range_search_device and search_device(topk = 10) in their
device forms, timed by HIP events on the stream the library launches on, ALTERNATED in one process -- range, top-k,
range, ... -- and the median of --reps each, with the extremes as the run-to-run spread.  The range call waits on the
host once per batch of queries (it reads the batch's total); those waits lie between the two events and are part of its
time.  The radii come from the data: the median over the queries of the 10th-neighbour distance of the exact search
(tens of hits per query where the neighbours' lists are probed), then of the 1000th.  The yardstick is the top-k search:
its code does not change with the range stage.  The split of a call into its kernels comes from a kernel trace of --quick
(rocprofv3 --kernel-trace --stats, a run of its own with no counters).

    python tools/ivf_range_time.py [--reps 5] [--quick] [--out profiles/ivf_range/time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from ivf_time import clustered  # noqa: E402
from range_time import alternate, stats  # noqa: E402
from vq_amd import _lib  # noqa: E402


def measure(ix, label, Q, nq, nprobe, radius, reps, about):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    tr, tk, res = alternate(lambda: ix.range_search_device(q.data_ptr(), nq, radius, nprobe=nprobe),
                            lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), reps)
    per = np.diff(res.lims.astype(np.int64))
    r, k = stats(tr), stats(tk)
    return {"index": label, "n": len(ix), "d": ix.dim, "nlist": ix.nlist, "metric": "euclidean", "nprobe": nprobe, "nq": nq,
            "radius": float(radius), "radius_from": f"median {about}th-neighbour distance of the queries (exact search)",
            "hits_total": int(res.total),
            "hits_per_query": {"mean": round(float(per.mean()), 1), "min": int(per.min()), "max": int(per.max())},
            "range_search": r, "search_topk10": k, "range_over_topk": round(r["ms"] / k["ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="IVFFlatIndex, nprobe 32, nq 1024, both radii (for a kernel trace)")
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
    ix = vq_amd.IVFFlatIndex.train(X[::4], 1024, max_iters=10)
    ix.add(X)
    lists = ix.list_ids
    exact = vq_amd.FlatIndex(X)
    _, d1000 = exact.search(Q, 1000)
    del exact
    radii = [(np.float32(np.median(d1000[:, 9])), 10), (np.float32(np.median(d1000[:, 999])), 1000)]
    if a.quick:
        for radius, about in radii:
            emit(measure(ix, "IVFFlatIndex", Q, 1024, 32, radius, a.reps, about))
    else:
        lo, hi = float(X.min()), float(X.max())
        sx = vq_amd.IVFScalarIndex(ix.coarse_centroids, vq_amd.ScalarQuantizer(lo, hi, 256), ix.distance)
        sx.add_rows(lists, X)
        for index, label in ((ix, "IVFFlatIndex"), (sx, "IVFScalarIndex")):
            for nprobe in (8, 32):
                for nq in (1, 1024):
                    for radius, about in radii:
                        emit(measure(index, label, Q, nq, nprobe, radius, a.reps, about))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
