"""Filtered against unfiltered inverted-file search (``allowed=`` of vq_amd.IVFFlatIndex / IVFScalarIndex; the view of
vq_amd/csrc/ivf_view.hpp and the picked row sources of ivf_tile.hpp) on one MI355X; prints one JSON line per measurement.

The set is tools/ivf_time.py's: 1M x 128 f32 rows around 4096 seeded Gaussian centres, IVFFlatIndex.train on 256K of its
rows (nlist = 1024, Euclidean), then add of every row; IVFScalarIndex holds the same rows in the same lists as SQ codes.
Everything in the device forms (queries, mask and top-k results on the device; a range result stays there), timed by HIP
events on the stream the library launches on.  For one (mask, nprobe, nq) the calls are ALTERNATED in one process --
unmasked, masked, unmasked again, ... -- and each reports the median of --reps with its extremes.  The unmasked call is
therefore timed twice in the same alternation: the difference of its two medians is the run's spread, which a masked
time has to beat before it counts as faster or slower.  The masks: all ones; random 50 %, 1 % and 0.1 %; the contiguous
first 10 % and 1 % of the row ids.  The grid: nprobe 1 and 32, nq 1 and 1024, for search (topk 10) and range_search (the
median 10th-neighbour distance of the queries) on IVFFlatIndex and for search on IVFScalarIndex.
  view      per mask, the build of the view alone: the masked call at nprobe 1, nq 1 less the unmasked one, alternated the
            same way (the call behind the view is the smallest there is; the view does not depend on nprobe or nq).  The
            kernels' own times are in the kernel trace of --quick.
  crossover the masked FlatIndex.search_device over the same rows under the same mask, 1024 queries: the exact tier a
            filter can fall back to
The split of a call into its kernels comes from a kernel trace of --quick (rocprofv3 --kernel-trace --stats, a run of its
own with no counters): IVFFlatIndex.search under the random 1 % mask at nprobe 32, nq 1024.

    python tools/ivf_filter_time.py [--reps 5] [--quick] [--out profiles/ivf_filter/time.json]
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
from filter_time import alternate, masks, stats  # noqa: E402
from ivf_time import clustered  # noqa: E402
from vq_amd import _lib  # noqa: E402


def measure(ix, label, call, q, nq, nprobe, name, w, allowed, reps, radius=None):
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    if call == "search":
        plain = lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe)
        masked = lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe, dev_allowed=w.data_ptr())
    else:
        plain = lambda: ix.range_search_device(q.data_ptr(), nq, radius, nprobe=nprobe)
        masked = lambda: ix.range_search_device(q.data_ptr(), nq, radius, nprobe=nprobe, dev_allowed=w.data_ptr())
    ta, tm, tb, res = alternate(plain, masked, reps)
    a, k, b = stats(ta), stats(tm), stats(tb)
    plain_ms = (a["ms"] + b["ms"]) / 2
    out = {"index": label, "call": call, "n": len(ix), "d": ix.dim, "nlist": ix.nlist, "metric": "euclidean", "nprobe": nprobe,
           "nq": nq, "mask": name, "allowed": allowed, "unmasked_first": a, "masked": k, "unmasked_second": b,
           "spread_ms": round(abs(a["ms"] - b["ms"]), 3), "masked_over_unmasked": round(k["ms"] / plain_ms, 3),
           "masked_less_unmasked_ms": round(k["ms"] - plain_ms, 3)}
    if call == "range_search":
        out["radius"] = float(radius)
        out["hits_total"] = int(res.total)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="IVFFlatIndex search, random 1 %, nprobe 32, nq 1024 (for a kernel trace)")
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
    n = X.shape[0]
    ix = vq_amd.IVFFlatIndex.train(X[::4], 1024, max_iters=10)
    ix.add(X)
    q = torch.from_numpy(Q).to("cuda")
    rng = np.random.default_rng(0)
    ms = [(name, m, torch.from_numpy(vq_amd.pack_row_mask(m, n).view(np.int32)).to("cuda")) for name, m in masks(n, rng)]
    if a.quick:
        name, m, w = ms[2]
        emit(measure(ix, "IVFFlatIndex", "search", q, 1024, 32, name, w, int(m.sum()), a.reps))
        return
    exact = vq_amd.FlatIndex(X)
    _, d10 = exact.search(Q, 10)
    r10 = np.float32(np.median(d10[:, 9]))
    idx = torch.empty((1024, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((1024, 10), dtype=torch.float32, device="cuda")
    for name, m, w in ms:
        r = measure(ix, "IVFFlatIndex", "search", q, 1, 1, name, w, int(m.sum()), a.reps)
        emit({"shape": "view", "mask": name, "allowed": r["allowed"], "view_ms": r["masked_less_unmasked_ms"],
              "spread_ms": r["spread_ms"], "from": r})
        ta, tm, tb, _ = alternate(lambda: exact.search_device(q.data_ptr(), 1024, 10, idx.data_ptr(), dist.data_ptr()),
                                  lambda: exact.search_device(q.data_ptr(), 1024, 10, idx.data_ptr(), dist.data_ptr(), dev_allowed=w.data_ptr()),
                                  a.reps)
        emit({"shape": "crossover", "index": "FlatIndex", "call": "search", "nq": 1024, "mask": name, "allowed": int(m.sum()),
              "unmasked_first": stats(ta), "masked": stats(tm), "unmasked_second": stats(tb)})
    del exact
    for call, radius in (("search", None), ("range_search", r10)):
        for nprobe in (1, 32):
            for nq in (1, 1024):
                for name, m, w in ms:
                    emit(measure(ix, "IVFFlatIndex", call, q, nq, nprobe, name, w, int(m.sum()), a.reps, radius))
    lists = ix.list_ids
    sx = vq_amd.IVFScalarIndex(ix.coarse_centroids, vq_amd.ScalarQuantizer(float(X.min()), float(X.max()), 256), ix.distance)
    ix.close()
    del ix
    sx.add_rows(lists, X)
    for nprobe in (1, 32):
        for nq in (1, 1024):
            for name, m, w in ms:
                emit(measure(sx, "IVFScalarIndex", "search", q, nq, nprobe, name, w, int(m.sum()), a.reps))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
