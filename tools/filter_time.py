"""Filtered against unfiltered search (``allowed=`` of vq_amd.FlatIndex / ScalarIndex; k_knn_dist_masked in
vq_amd/csrc/knn_tile.hpp) on one MI355X: 1M x 128 uniform rows, 1024 queries, Euclidean, topk 10; prints one JSON line
per measurement.

Everything in the device forms (queries, mask and top-k results on the device; a range result stays there), timed by HIP
events on the stream the library launches on.  For one mask the three calls are ALTERNATED in one process -- unmasked,
masked, unmasked again, ... -- and each reports the median of --reps with its extremes.  The unmasked call is therefore
timed twice in the same alternation: the difference of its two medians is the run's spread, which a masked time has to
beat before it counts as faster or slower.  The masks: all ones; random 50 %, 1 % and 0.1 %; the contiguous first 10 %
and 1 % of the rows.  `empty_tiles` is the share of 64-row tiles without an allowed row, the tiles k_knn_dist_masked
leaves after two mask words.  The same list runs for range_search at the median 20th-neighbour distance of the queries
(about 20 hits per query unmasked), and one line (contiguous 1 %) for ScalarIndex over the same rows as SQ codes.

    python tools/filter_time.py [--reps 5] [--quick] [--out profiles/filter/time.json]
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


def alternate(plain_fn, masked_fn, reps):
    """warm both, then unmasked / masked / unmasked in turn; (first unmasked ms list, masked ms list, second unmasked ms
    list, the last masked result)"""
    plain_fn()
    masked_fn()
    torch.cuda.synchronize()
    ta, tm, tb, res = [], [], [], None
    for _ in range(reps):
        ta.append(timed(plain_fn)[0])
        ms, res = timed(masked_fn)
        tm.append(ms)
        tb.append(timed(plain_fn)[0])
    return ta, tm, tb, res


def stats(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def masks(n, rng):
    def block(share):
        m = np.zeros(n, bool)
        m[:int(n * share)] = True
        return m

    return [("all ones", np.ones(n, bool)), ("random 50 %", rng.random(n) < 0.5), ("random 1 %", rng.random(n) < 0.01),
            ("random 0.1 %", rng.random(n) < 0.001), ("contiguous 10 %", block(0.10)), ("contiguous 1 %", block(0.01))]


def measure(ix, label, call, q, nq, name, m, reps, radius=None):
    n = len(ix)
    w = torch.from_numpy(vq_amd.pack_row_mask(m, n).view(np.int32)).to("cuda")
    idx = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
    if call == "search":
        plain = lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr())
        masked = lambda: ix.search_device(q.data_ptr(), nq, 10, idx.data_ptr(), dist.data_ptr(), dev_allowed=w.data_ptr())
    else:
        plain = lambda: ix.range_search_device(q.data_ptr(), nq, radius)
        masked = lambda: ix.range_search_device(q.data_ptr(), nq, radius, dev_allowed=w.data_ptr())
    ta, tm, tb, res = alternate(plain, masked, reps)
    a, k, b = stats(ta), stats(tm), stats(tb)
    tiles = np.zeros((n + 63) // 64 * 64, bool)
    tiles[:n] = m
    plain_ms = (a["ms"] + b["ms"]) / 2
    out = {"index": label, "call": call, "n": n, "d": ix.dim, "metric": "euclidean", "nq": nq, "mask": name,
           "allowed": int(m.sum()), "empty_tiles": round(float(1.0 - tiles.reshape(-1, 64).any(axis=1).mean()), 4),
           "unmasked_first": a, "masked": k, "unmasked_second": b, "spread_ms": round(abs(a["ms"] - b["ms"]), 3),
           "masked_over_unmasked": round(k["ms"] / plain_ms, 3)}
    if call == "range_search":
        out["radius"] = float(radius)
        out["hits_total"] = int(res.total)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="FlatIndex search under the contiguous 1 % mask only (for a kernel trace)")
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
    ms = masks(n, rng)
    if a.quick:
        emit(measure(ix, "FlatIndex", "search", q, nq, *ms[-1], a.reps))
    else:
        for name, m in ms:
            emit(measure(ix, "FlatIndex", "search", q, nq, name, m, a.reps))
        _, d20 = ix.search(Q, 20)
        r20 = np.float32(np.median(d20[:, 19]))
        for name, m in ms:
            emit(measure(ix, "FlatIndex", "range_search", q, nq, name, m, a.reps, r20))
        del ix
        sx = vq_amd.ScalarIndex(X, vq_amd.ScalarQuantizer(0.0, 1.0, 256), vq_amd.Distance.euclidean())
        emit(measure(sx, "ScalarIndex", "search", q, nq, *ms[-1], a.reps))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "reps": a.reps, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
