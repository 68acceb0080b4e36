"""Range search against top-k search (vq_amd.FlatIndex, vq_amd/csrc/range.hpp and k_knn.hip) on one MI355X: 1M x 128
uniform rows, 1024 queries, Euclidean; prints one JSON line per measurement.

Both searches in their device forms (queries on the device; the top-k results and the range result stay there), timed by
HIP events on the stream the library launches on, ALTERNATED in one process -- range, top-k, range, ... -- and the
median of --reps each, with the extremes as the run-to-run spread.  The range call waits on the host once per batch of
queries (it reads the batch's total); those waits lie between the two events and are part of its time.  The radius comes
from the data: the median over the queries of the 10th-neighbour distance (about 10 hits per query), then of the 1000th
(about 1000).  ScalarIndex (the same rows as SQ codes) is measured the same way at the first radius.

    python tools/range_time.py [--reps 5] [--quick] [--out profiles/range/time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream())
    out = fn()
    b.record(torch.cuda.current_stream())
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(range_fn, topk_fn, reps):
    """warm both, then range / top-k in turn; (range ms list, top-k ms list, the last range result)"""
    range_fn()
    topk_fn()
    torch.cuda.synchronize()
    tr, tk, res = [], [], None
    for _ in range(reps):
        ms, res = timed(range_fn)
        tr.append(ms)
        ms, _ = timed(topk_fn)
        tk.append(ms)
    return tr, tk, res


def stats(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(ix, label, q, nq, radius, reps, about):
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    tr, tk, res = alternate(lambda: ix.range_search_device(q.data_ptr(), nq, radius),
                            lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr()), reps)
    per = np.diff(res.lims.astype(np.int64))
    r, k = stats(tr), stats(tk)
    return {"index": label, "n": len(ix), "d": ix.dim, "metric": "euclidean", "nq": nq, "radius": float(radius),
            "radius_from": f"median {about}th-neighbour distance of the queries", "hits_total": int(res.total),
            "hits_per_query": {"mean": round(float(per.mean()), 1), "min": int(per.min()), "max": int(per.max())},
            "range_search": r, "search_topk10": k, "range_over_topk": round(r["ms"] / k["ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the flat index at the first radius only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()  # the library's launches on the stream the events time
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    n, d, nq = 1 << 20, 128, 1024
    X = _lib.synth_uniform_host(n, d, 1, 0)
    rng = np.random.default_rng(0)
    Q = rng.random((nq, d), dtype=np.float32)
    q = torch.from_numpy(Q).to("cuda")
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    ix = vq_amd.FlatIndex(X, vq_amd.Distance.euclidean())
    _, d1000 = ix.search(Q, 1000)
    r10, r1000 = np.float32(np.median(d1000[:, 9])), np.float32(np.median(d1000[:, 999]))
    emit(measure(ix, "FlatIndex", q, nq, r10, a.reps, 10))
    if not a.quick:
        emit(measure(ix, "FlatIndex", q, nq, r1000, a.reps, 1000))
        del ix
        sq = vq_amd.ScalarQuantizer(0.0, 1.0, 256)
        sx = vq_amd.ScalarIndex(X, sq, vq_amd.Distance.euclidean())
        _, s10 = sx.search(Q, 10)
        emit(measure(sx, "ScalarIndex", q, nq, np.float32(np.median(s10[:, 9])), a.reps, 10))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
