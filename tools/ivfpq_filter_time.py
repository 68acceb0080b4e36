"""Filtered against unfiltered PQ search (``IVFPQIndex.masked_search_device``, plain and residual lists, and
``PQIndex.search(allowed=)``; the picked scans of vq_amd/csrc/k_ivf.hip and k_adc_scan_masked of k_adc.hip) on one MI355X;
prints one JSON line per measurement.  Needs a GPU: there is no fallback.

The set is tools/ivf_time.py's: 1M x 128 f32 rows around 4096 seeded Gaussian centres; IVFPQIndex.train on 256K of its rows
(nlist = 1024, m = 8, k = 256, Euclidean), plain and residual, then add of every row; PQIndex holds the plain index's codes.
IVFPQIndex runs in the device forms (queries, mask and results on the device), PQIndex in its host form (the only one it
has); both are timed by HIP events on the stream the library launches on.  For one (mask, nq) the calls are ALTERNATED in
one process -- unfiltered, filtered, unfiltered again, ... -- after a warm-up, and each reports the median of --reps with
its extremes.  The unfiltered call is therefore timed twice in the same alternation: the difference of its two medians is
the run's spread.  The masks: all ones; random 50 %, 1 % and 0.1 %; the contiguous first 10 % and 1 % of the row ids.  The
grid: 1024 queries and one query at nprobe 32 (PQIndex: 1024 queries and one), topk 10.  Per mask the JSON also holds the
allowed rows of the probed lists (mean over the queries) and, for PQIndex, the share of 64-row groups with an allowed row.

  --quick  the random 1 % line of each index only, 1024 queries: for a kernel trace (rocprofv3 --kernel-trace --stats,
           a run of its own with no counters)
  --ab     the unfiltered calls only, through nothing this tool's own tree adds: run it from two trees (--tree) in turn to
           compare two builds of the library

    python tools/ivfpq_filter_time.py [--reps 5] [--quick | --ab] [--tree DIR] [--out profiles/ivfpq_filter/time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree():
    for j, a in enumerate(sys.argv):
        if a == "--tree" and j + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[j + 1])
    return ROOT


sys.path.insert(0, _tree())  # the tree whose vq_amd (and libvqhip.so) is measured
sys.path.insert(1, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from filter_time import alternate, masks, stats, timed  # noqa: E402
from ivf_time import clustered  # noqa: E402
from vq_amd import _lib  # noqa: E402
from vq_amd.store import PQIndex  # noqa: E402

NPROBE, TOPK = 32, 10


def line(label, nq, name, allowed, ta, tm, tb, extra):
    a, k, b = stats(ta), stats(tm), stats(tb)
    plain_ms = (a["ms"] + b["ms"]) / 2
    out = {"index": label, "call": "search", "nq": nq, "topk": TOPK, "mask": name, "allowed": allowed, "unfiltered_first": a,
           "filtered": k, "unfiltered_second": b, "spread_ms": round(abs(a["ms"] - b["ms"]), 3),
           "filtered_over_unfiltered": round(k["ms"] / plain_ms, 3), "filtered_less_unfiltered_ms": round(k["ms"] - plain_ms, 3)}
    out.update(extra)
    return out


def ivf_calls(ix, q, nq, w):
    idx = torch.empty((nq, TOPK), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, TOPK), dtype=torch.float32, device="cuda")
    plain = lambda: ix.search_device(q.data_ptr(), nq, TOPK, idx.data_ptr(), dist.data_ptr(), nprobe=NPROBE)
    if w is None:
        return plain, None
    return plain, lambda: ix.masked_search_device(q.data_ptr(), nq, TOPK, idx.data_ptr(), dist.data_ptr(), w.data_ptr(), nprobe=NPROBE)


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    return stats([timed(fn)[0] for _ in range(reps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the random 1 %% line of each index, 1024 queries (for a kernel trace)")
    ap.add_argument("--ab", action="store_true", help="the unfiltered calls only (to compare two builds, one --tree each)")
    ap.add_argument("--tree", default=None, help="the tree whose vq_amd is imported (default: this one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivfpq_filter_time.py needs a GPU")
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
    q = torch.from_numpy(Q).to("cuda")
    rng = np.random.default_rng(0)
    ms = masks(n, rng)
    if a.quick:
        ms = ms[2:3]
    indexes = []
    for residual in (False, True):
        ix = vq_amd.IVFPQIndex.train(X[::4], 1024, 8, 256, max_iters=10, residual=residual)
        ix.add(X)
        indexes.append(("IVFPQIndex residual" if residual else "IVFPQIndex", ix))
    px = PQIndex(indexes[0][1].codebooks, indexes[0][1].codes, indexes[0][1].distance)
    if a.ab:
        for label, ix in indexes:
            for nq in (1024, 1):
                emit({"index": label, "call": "search", "nq": nq, "nprobe": NPROBE, "tree": _tree(), "lib": _lib.LIB_PATH,
                      "unfiltered": median_ms(ivf_calls(ix, q, nq, None)[0], a.reps)})
        for nq in (1024, 64, 1):
            emit({"index": "PQIndex", "call": "search", "nq": nq, "tree": _tree(), "lib": _lib.LIB_PATH,
                  "unfiltered": median_ms(lambda: px.search(Q[:nq], TOPK), a.reps)})
        emit({"index": "PQIndex", "call": "search", "nq": 64, "topk": 257, "schedule": "full pass", "tree": _tree(), "lib": _lib.LIB_PATH,
              "unfiltered": median_ms(lambda: px.search(Q[:64], 257), a.reps)})
    else:
        lists = indexes[0][1].list_ids
        probed = indexes[0][1].probe(Q, NPROBE)  # (the residual index probes the same centroids)
        in_probed = np.zeros((Q.shape[0], 1024), bool)
        in_probed[np.arange(Q.shape[0])[:, None], probed] = True
        for name, m in ms:
            w = torch.from_numpy(vq_amd.pack_row_mask(m, n).view(np.int32)).to("cuda")
            per_list = np.bincount(lists[m], minlength=1024)
            extra = {"n": n, "nlist": 1024, "m": 8, "k": 256, "nprobe": NPROBE,
                     "allowed_in_probed_lists_mean": round(float((in_probed * per_list[None, :]).sum(axis=1).mean()), 1),
                     "rows_in_probed_lists_mean": round(float((in_probed * np.bincount(lists, minlength=1024)[None, :]).sum(axis=1).mean()), 1)}
            for label, ix in indexes:
                for nq in ((1024,) if a.quick else (1024, 1)):
                    plain, filtered = ivf_calls(ix, q, nq, w)
                    ta, tm, tb, _ = alternate(plain, filtered, a.reps)
                    emit(line(label, nq, name, int(m.sum()), ta, tm, tb, extra))
            groups = float(m[:n // 64 * 64].reshape(-1, 64).any(axis=1).mean())
            for nq in ((1024,) if a.quick else (1024, 1)):
                ta, tm, tb, _ = alternate(lambda: px.search(Q[:nq], TOPK), lambda: px.search(Q[:nq], TOPK, allowed=m), a.reps)
                emit(line("PQIndex", nq, name, int(m.sum()), ta, tm, tb,
                          {"n": n, "m": 8, "k": 256, "groups_with_an_allowed_row": round(groups, 4),
                           "unfiltered_schedule": "one scan", "filtered_schedule": "full pass"}))
            if not a.quick:  # the same schedule on both sides: the unfiltered full pass (topk 257 > 256 is not one-scan eligible)
                ta, tm, tb, _ = alternate(lambda: px.search(Q[:64], 257), lambda: px.search(Q[:64], 257, allowed=m), a.reps)
                r = line("PQIndex", 64, name, int(m.sum()), ta, tm, tb, {"n": n, "groups_with_an_allowed_row": round(groups, 4),
                                                                       "unfiltered_schedule": "full pass", "filtered_schedule": "full pass"})
                r["topk"] = 257
                emit(r)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
