"""Inverted-file 4-bit scalar search rates (vq_amd.IVFScalar4Index, vq_amd/csrc/k_ivfsq4.hip) on one MI355X beside
IVFScalarIndex over the same codes, one byte each, in the same lists; prints one JSON line per shape.

The set is tools/ivfsq_time.py's at each --dims (default 128 and 1024, where the rows' bytes show): 1M f32 rows around
4096 seeded Gaussian centres; IVFScalar4Index.train on 256K of its rows (nlist = 1024 coarse centroids, Euclidean),
ScalarQuantizer(mean - 2.5 std, mean + 2.5 std, 16) of all elements (tools/sq4index_time.py's "sigma" rule), then add of
every row.  The IVFScalarIndex holds the unpacked codes in the same lists, so both searches return the same bits
(same_bits, checked at every shape).  Per (nprobe, nq): the two device forms (queries and results on the device, HIP-event
ms per call) alternated call by call in one process, five calls each -- the median with the extremes --, the positions
the call scans, and within_margin: the 4-bit search's median is no more than the 8-bit search's times 1 + margin, the
margin being the larger of 5 % and the two searches' own spreads ((max - min) / median): the pair arithmetic is identical
and only the fill differs.  recall@10 against the exact search over the original rows.

    python tools/ivfsq4_time.py [--reps 5] [--dims 128 1024] [--quick] [--out profiles/ivfsq4/time.json]
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
from ivfsq_time import event_runs, stats  # noqa: E402
from vq_amd import _lib  # noqa: E402


def shape(ix4, ix8, Q, nprobe, nq, topk, reps, sizes, exact):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    ridx, rdist = torch.empty_like(idx), torch.empty_like(dist)
    runs4, runs8 = [], []
    for _ in range(reps):  # alternated call by call
        runs4 += event_runs(lambda: ix4.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), 1)
        runs8 += event_runs(lambda: ix8.search_device(q.data_ptr(), nq, topk, ridx.data_ptr(), rdist.data_ptr(), nprobe=nprobe), 1)
    torch.cuda.synchronize()
    s4, s8 = stats(runs4), stats(runs8)
    spread = max((s4["max"] - s4["min"]) / s4["median"], (s8["max"] - s8["min"]) / s8["median"])
    margin = max(0.05, spread)
    got = idx.cpu().numpy().view(np.uint32)
    same = bool(np.array_equal(got, ridx.cpu().numpy().view(np.uint32)) and torch.equal(dist.view(torch.int32), rdist.view(torch.int32)))
    positions = int(sizes[ix4.probe(Q[:nq], nprobe)].sum())
    return {"n": len(ix4), "dim": ix4.dim, "nlist": ix4.nlist, "nprobe": nprobe, "nq": nq, "topk": topk, "ivfsq4_ms": s4, "ivfsq_ms": s8,
            "ratio": round(s4["median"] / s8["median"], 3), "margin": round(margin, 3),
            "within_margin": bool(s4["median"] <= s8["median"] * (1 + margin)), "same_bits": same, "positions": positions,
            "row_bytes": {"ivfsq4": 4 * ix4.words, "ivfsq": ix4.dim},
            "recall_at_10": round(float(np.mean([len(set(got[j, :10]) & set(exact[j])) / 10 for j in range(nq)])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 1024])
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

    for d in a.dims:
        X, Q = clustered(a.n, d, 4096, 7)
        mean, std = float(X.mean(dtype=np.float64)), float(X.std(dtype=np.float64))
        sq = vq_amd.ScalarQuantizer(mean - 2.5 * std, mean + 2.5 * std, 16)
        t0 = time.perf_counter()
        ix4 = vq_amd.IVFScalar4Index.train(X[::4], 1024, sq, max_iters=10)
        train_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ix4.add(X)
        add_s = time.perf_counter() - t0
        sizes = ix4.list_sizes().astype(np.int64)
        ix8 = vq_amd.IVFScalarIndex(ix4.coarse_centroids, sq, ix4.distance)
        ix8.add_codes(ix4.list_ids, ix4.codes())
        exact = vq_amd.FlatIndex(X).search(Q, 10)[0]
        del X
        if a.quick:
            emit(shape(ix4, ix8, Q, 32, 1024, 10, a.reps, sizes, exact))
        else:
            emit({"shape": "index", "n": len(ix4), "dim": d, "nlist": ix4.nlist, "quantizer": repr(sq), "train_s": round(train_s, 2),
                  "add_s": round(add_s, 2), "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
                  "list_size_mean": round(float(sizes.mean()), 1)})
            for nprobe in (1, 8, 32, 128):
                for nq in (1, 64, 1024):
                    emit(shape(ix4, ix8, Q, nprobe, nq, 10, a.reps, sizes, exact))
        ix4.close()
        ix8.close()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "command": "python tools/ivfsq4_time.py " + " ".join(sys.argv[1:]),
                       "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
