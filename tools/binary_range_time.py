"""Hamming-radius range search against the same index's top-k search (vq_amd.BinaryIndex, vq_amd.IVFBinaryIndex;
k_bin_range in vq_amd/csrc/k_binary.hip, the range stage of ivf_range.hpp behind k_ivfbin.hip) on one MI355X; prints one
JSON line per measurement.

The sets are tools/ivfbin_time.py's: 1M x 256 and 1M x 1024 f32 rows around 4096 seeded Gaussian centres, binarised by
BinaryQuantizer(0.0) under Manhattan (the reported distance is the Hamming count); IVFBinaryIndex.train on 256K of the
rows (nlist = 1024, Euclidean) and add of every row, the BinaryIndex over the same words.  Per index and radius:
hamming_range_search_device and search_device(topk = 10) in their device forms, 1024 queries, timed by HIP events on the
stream the library launches on, ALTERNATED in one process -- range, top-k, range, ... -- and the median of --reps each,
with the extremes as the run-to-run spread.  The range call waits on the host once per batch of queries (it reads the
batch's total); those waits lie between the two events and are part of its time.  The radii come from the data: the
median over the queries of the 10th-neighbour H of the dense search, then of the 1000th.  The inverted-file index runs
at nprobe 1, 8 and 32.  The yardstick is the top-k search of the same index: its code does not change with the range
search.  within_margin: the range median is no more than the top-k median x (1 + margin), the margin the larger of 5 %
and the two runs' spreads.  The split of a call into its kernels comes from a kernel trace of --quick (rocprofv3
--kernel-trace --stats, a run of its own with no counters).

    python tools/binary_range_time.py [--reps 5] [--quick] [--dims 256,1024] [--out profiles/binary_range/time.json]
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


def spread(s):
    return (s["max_ms"] - s["min_ms"]) / s["ms"]


def measure(ix, label, q, nq, radius, reps, about, nprobe=None):
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    kw = {} if nprobe is None else {"nprobe": nprobe}
    tr, tk, res = alternate(lambda: ix.hamming_range_search_device(q.data_ptr(), nq, radius, **kw),
                            lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), **kw), reps)
    per = np.diff(res.lims.astype(np.int64))
    r, k = stats(tr), stats(tk)
    margin = max(0.05, spread(r), spread(k))
    out = {"index": label, "n": len(ix), "d": ix.dim, "metric": "manhattan", "nq": nq, "radius_bits": int(radius),
           "radius_from": f"median {about}th-neighbour H of the queries (dense search)", "hits_total": int(res.total),
           "hits_per_query": {"mean": round(float(per.mean()), 1), "min": int(per.min()), "max": int(per.max())},
           "range_search": r, "search_topk10": k, "range_over_topk": round(r["ms"] / k["ms"], 3), "margin": round(margin, 3),
           "within_margin": bool(r["ms"] <= k["ms"] * (1.0 + margin))}
    if nprobe is not None:
        out["nlist"], out["nprobe"] = ix.nlist, nprobe
    return out


def one_set(dim, a, emit):
    X, Q = clustered(1 << 20, dim, 4096, 7)
    nq = 1024
    ix = vq_amd.IVFBinaryIndex.train(X[::4], 1024, max_iters=10)
    ix.add(X)
    del X
    bx = vq_amd.BinaryIndex.from_packed(ix.packed(), dim, ix.quantizer, ix.distance)
    _, h1000 = bx.search(Q[:nq], 1000)  # Manhattan over bits 0 / 1: the distance is H
    radii = [(int(np.median(h1000[:, 9])), 10), (int(np.median(h1000[:, 999])), 1000)]
    q = torch.from_numpy(np.ascontiguousarray(Q[:nq])).cuda()
    if a.quick:
        emit(measure(bx, "BinaryIndex", q, nq, radii[0][0], a.reps, radii[0][1]))
        emit(measure(ix, "IVFBinaryIndex", q, nq, radii[0][0], a.reps, radii[0][1], nprobe=32))
    else:
        for radius, about in radii:
            emit(measure(bx, "BinaryIndex", q, nq, radius, a.reps, about))
        for nprobe in (1, 8, 32):
            for radius, about in radii:
                emit(measure(ix, "IVFBinaryIndex", q, nq, radius, a.reps, about, nprobe=nprobe))
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1M x 256, the first radius, BinaryIndex and IVFBinaryIndex at nprobe 32 (for a kernel trace)")
    ap.add_argument("--dims", default="256,1024")
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

    for dim in ([256] if a.quick else [int(v) for v in a.dims.split(",")]):
        one_set(dim, a, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        cmd = "python tools/binary_range_time.py" + (" --quick" if a.quick else "") + f" --reps {a.reps} --out {a.out}"
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "command": cmd, "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
