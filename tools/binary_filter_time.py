"""Filtered against unfiltered search on the two binary indexes (``filtered_search_device`` /
``filtered_hamming_range_search_device`` of vq_amd.BinaryIndex and vq_amd.IVFBinaryIndex; the masked scans of
vq_amd/csrc/k_binary.hip, the view and the picked kernels of k_ivfbin.hip) on one MI355X; prints one JSON line per
measurement.

The set is tools/binary_range_time.py's: 1M rows of 256 and of 1024 dimensions around 4096 seeded Gaussian centres,
IVFBinaryIndex.train on 256K of them (nlist = 1024), add of every row, and a BinaryIndex over the same words.  Everything
in the device forms (queries, mask and top-k results on the device; a range result stays there), timed by HIP events on
the stream the library launches on.  For one line the calls are ALTERNATED in one process -- unmasked, masked, unmasked
again, ... -- and each reports the median of --reps with its extremes.  The unmasked call is therefore timed twice in the
same alternation: the difference of its two medians is the run's spread, which a masked time has to beat before it counts
as faster or slower.  The masks: all ones; random 50 %, 1 % and 0.1 %; the contiguous first 10 % and 1 % of the row ids.
The grid: 1024 queries and 1 query, topk 10, for BinaryIndex search and hamming_range_search (the median 10th-neighbour H
of the queries) and for IVFBinaryIndex search and hamming_range_search at nprobe 1 and 32.
  groups   per line of BinaryIndex, the share of 64-row groups with an allowed row: what a masked scan still computes
The split of a call into its kernels comes from a kernel trace of --quick (rocprofv3 --kernel-trace --stats, a run of its
own with no counters): the contiguous 1 % line of every call at 1M x 1024, 1024 queries.

    python tools/binary_filter_time.py [--reps 5] [--quick] [--dims 256,1024] [--out profiles/binary_filter/time.json]
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


def measure(ix, label, call, q, nq, name, m, w, reps, radius=None, nprobe=None):
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    kw = {} if nprobe is None else {"nprobe": nprobe}
    if call == "search":
        plain = lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), **kw)
        masked = lambda: ix.filtered_search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), w.data_ptr(), **kw)
    else:
        plain = lambda: ix.hamming_range_search_device(q.data_ptr(), nq, radius, **kw)
        masked = lambda: ix.filtered_hamming_range_search_device(q.data_ptr(), nq, radius, w.data_ptr(), **kw)
    ta, tm, tb, res = alternate(plain, masked, reps)
    a, k, b = stats(ta), stats(tm), stats(tb)
    n = len(ix)
    plain_ms = (a["ms"] + b["ms"]) / 2
    out = {"index": label, "call": call, "n": n, "d": ix.dim, "metric": "manhattan", "nq": nq, "mask": name, "allowed": int(m.sum()),
           "unmasked_first": a, "masked": k, "unmasked_second": b, "spread_ms": round(abs(a["ms"] - b["ms"]), 3),
           "masked_over_unmasked": round(k["ms"] / plain_ms, 3), "masked_less_unmasked_ms": round(k["ms"] - plain_ms, 3)}
    if nprobe is None:
        groups = np.zeros((n + 63) // 64 * 64, bool)
        groups[:n] = m
        out["groups_with_an_allowed_row"] = round(float(groups.reshape(-1, 64).any(axis=1).mean()), 4)
    else:
        out["nlist"], out["nprobe"] = ix.nlist, nprobe
    if call != "search":
        out["radius_bits"] = int(radius)
        out["hits_total"] = int(res.total)
    return out


def one_set(dim, a, emit):
    X, Q = clustered(1 << 20, dim, 4096, 7)
    n = X.shape[0]
    ix = vq_amd.IVFBinaryIndex.train(X[::4], 1024, max_iters=10)
    ix.add(X)
    del X
    bx = vq_amd.BinaryIndex.from_packed(ix.packed(), dim, ix.quantizer, ix.distance)
    _, h10 = bx.search(Q[:1024], 10)  # Manhattan over bits 0 / 1: the distance is H
    radius = int(np.median(h10[:, 9]))
    q = torch.from_numpy(np.ascontiguousarray(Q[:1024])).cuda()
    rng = np.random.default_rng(0)
    ms = [(name, m, torch.from_numpy(vq_amd.pack_row_mask(m, n).view(np.int32)).to("cuda")) for name, m in masks(n, rng)]
    if a.quick:
        ms, nqs = ms[5:], (1024,)
    else:
        nqs = (1024, 1)
    for call, r in (("search", None), ("hamming_range_search", radius)):
        for nq in nqs:
            for name, m, w in ms:
                emit(measure(bx, "BinaryIndex", call, q, nq, name, m, w, a.reps, r))
            for nprobe in (1, 32):
                for name, m, w in ms:
                    emit(measure(ix, "IVFBinaryIndex", call, q, nq, name, m, w, a.reps, r, nprobe=nprobe))
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1M x 1024, 1024 queries, the contiguous 1 % mask only (for a kernel trace)")
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

    for dim in ([1024] if a.quick else [int(v) for v in a.dims.split(",")]):
        one_set(dim, a, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        cmd = "python tools/binary_filter_time.py" + (" --quick" if a.quick else "") + f" --reps {a.reps} --out {a.out}"
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "command": cmd, "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
