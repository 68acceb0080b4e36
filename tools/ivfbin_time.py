"""Inverted-file binary search rates (vq_amd.IVFBinaryIndex, vq_amd/csrc/k_ivfbin.hip) on one MI355X beside BinaryIndex over
the same rows; prints one JSON line per shape.

The sets are 1M x 1024 and 1M x 256 f32 rows around 4096 seeded Gaussian centres (tools/ivf_time.py's `clustered`);
IVFBinaryIndex.train on 256K of the rows (nlist = 1024 coarse centroids, Euclidean), BinaryQuantizer(0.0), then add of
every row; the BinaryIndex holds the same words.  Per (nprobe, nq): the two device forms (queries and results on the
device, HIP-event ms per call) alternated call by call in one process, five calls each -- the median with the extremes --,
the positions the call scans, the fraction of the VALU bound the whole call reaches (positions x W x 2 lane-operations at
7.86e13/s: DESIGN.md section 12's bound) and within_margin: the inverted search's median is no more than BinaryIndex's
times 1 + margin, the margin being the larger of 5 % and the two searches' own spreads ((max - min) / median).
recall@10 against the exact search over the original rows, as returned and with rerank=FlatIndex at 40 and 100
candidates, for both indexes.  At nprobe = nlist, same_bits: both searches return the same arrays.

    python tools/ivfbin_time.py [--reps 5] [--quick] [--dims 1024,256] [--out profiles/ivfbin/time.json]
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

VALU_RATE = 7.86e13  # lane-operations per second


def recall(got, exact):
    return round(float(np.mean([len(set(got[j, :10]) & set(exact[j])) / 10 for j in range(got.shape[0])])), 4)


def shape(ix, bx, Q, nprobe, nq, topk, reps, sizes, exact):
    q = torch.from_numpy(Q[:nq]).cuda()
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    bidx, bdist = torch.empty_like(idx), torch.empty_like(dist)
    ivf_runs, bin_runs = [], []
    for _ in range(reps):  # alternated call by call
        ivf_runs += event_runs(lambda: ix.search_device(q.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr(), nprobe=nprobe), 1)
        bin_runs += event_runs(lambda: bx.search_device(q.data_ptr(), nq, topk, bidx.data_ptr(), bdist.data_ptr()), 1)
    torch.cuda.synchronize()
    iv, bn = stats(ivf_runs), stats(bin_runs)
    spread = max((iv["max"] - iv["min"]) / iv["median"], (bn["max"] - bn["min"]) / bn["median"])
    margin = max(0.05, spread)
    got = idx.cpu().numpy().view(np.uint32)
    positions = int(sizes[ix.probe(Q[:nq], nprobe)].sum())
    words = (ix.dim + 31) // 32
    r = {"n": len(ix), "dim": ix.dim, "nlist": ix.nlist, "nprobe": nprobe, "nq": nq, "topk": topk, "ivfbin_ms": iv, "binary_ms": bn,
         "ratio": round(iv["median"] / bn["median"], 3), "margin": round(margin, 3),
         "within_margin": bool(iv["median"] <= bn["median"] * (1 + margin)), "positions": positions,
         "valu_bound_fraction": round(positions * words * 2 / VALU_RATE / (iv["median"] * 1e-3), 4),
         "recall_at_10": recall(got, exact[:nq])}
    if nprobe == ix.nlist:
        r["same_bits"] = bool(np.array_equal(got, bidx.cpu().numpy().view(np.uint32)) and torch.equal(dist.view(torch.int32), bdist.view(torch.int32)))
    return r


def one_set(dim, a, emit):
    X, Q = clustered(1 << 20, dim, 4096, 7)
    t0 = time.perf_counter()
    ix = vq_amd.IVFBinaryIndex.train(X[::4], 1024, max_iters=10)
    train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.add(X)
    add_s = time.perf_counter() - t0
    sizes = ix.list_sizes().astype(np.int64)
    bx = vq_amd.BinaryIndex.from_packed(ix.packed(), dim, ix.quantizer, ix.distance)
    flat = vq_amd.FlatIndex(X)
    exact = flat.search(Q, 10)[0]
    if a.quick:
        emit(shape(ix, bx, Q, 32, 1024, 10, a.reps, sizes, exact))
        return
    emit({"shape": "index", "n": len(ix), "dim": dim, "nlist": ix.nlist, "quantizer": repr(ix.quantizer), "train_s": round(train_s, 2),
          "add_s": round(add_s, 2), "list_size_min": int(sizes.min()), "list_size_max": int(sizes.max()),
          "list_size_mean": round(float(sizes.mean()), 1)})
    for nprobe in (1, 8, 32, 128):
        for nq in (1, 64, 1024):
            emit(shape(ix, bx, Q, nprobe, nq, 10, a.reps, sizes, exact))
    emit(shape(ix, bx, Q, ix.nlist, 1024, 10, a.reps, sizes, exact))
    rr = {"shape": "rerank", "dim": dim, "nq": 1024, "binary": {}, "ivfbin_nprobe_32": {}}
    for c in (40, 100):  # the binarisation loss (BinaryIndex) beside the probing loss on top of it
        rr["binary"][f"candidates_{c}"] = recall(bx.search(Q[:1024], 10, rerank=flat, candidates=c)[0], exact[:1024])
        rr["ivfbin_nprobe_32"][f"candidates_{c}"] = recall(ix.search(Q[:1024], 10, nprobe=32, rerank=flat, candidates=c)[0], exact[:1024])
    emit(rr)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="nq = 1024, nprobe = 32 only (for a kernel trace)")
    ap.add_argument("--dims", default="1024,256")
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
        if a.out:  # (kept current: a long run leaves what it has)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"gpu": torch.cuda.get_device_name(0), "command": "python tools/ivfbin_time.py " + " ".join(sys.argv[1:]),
                           "results": res}, f, indent=1)

    for dim in (int(d) for d in a.dims.split(",")):
        one_set(dim, a, emit)


if __name__ == "__main__":
    main()
