"""Binary index rates (vq_amd.BinaryIndex, vq_amd/csrc/k_binary.hip) on one MI355X; prints one JSON line per result.

  pack     BinaryQuantizer rows -> packed words on the device (vqhip_bq_pack_device), 1M x {256, 1024} f32: HIP-event ms
           (median of --reps) and TB/s of bytes read + written.
  search   1024 queries over 1M x {256, 1024} bits, topk 10 / 100, device form: ms per call and the fraction of the VALU
           bound of ONE Hamming scan -- 2 operations (v_xor, v_bcnt) per 32 dimensions per (query, row) pair at
           2 x 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 7.86e13 lane-operations/s.  The search runs the scan twice
           (histogram, then collection); the kernel split comes from a `rocprofv3 --kernel-trace --stats` run of --quick.
  recall   recall@10 against FlatIndex (Euclidean, f32 rows) on clustered rows: BQ alone, and BQ + exact rerank of 4x and
           10x topk candidates through FlatIndex.

    python tools/binary_time.py [--reps 5] [--quick] [--out profiles/binary/time.json]
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

LANE_OPS = 2 * 256 * 4 * 16 * 2.4e9


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def clustered(n, d, seed, centers=None):
    """rows around 4096 Gaussian centres (the centres are returned for queries from the same distribution)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if centers is None:
        centers = torch.randn((4096, d), device="cuda", generator=g)
    lab = torch.randint(0, centers.shape[0], (n,), device="cuda", generator=g)
    X = centers[lab] + 0.7 * torch.randn((n, d), device="cuda", generator=g)
    return X.contiguous(), centers


def pack_shape(X, reps):
    n, d = X.shape
    w = (d + 31) // 32
    out = torch.empty((n, w), dtype=torch.int32, device="cuda")
    fn = lambda: _lib.check(_lib.load().vqhip_bq_pack_device(0.0, X.data_ptr(), n, d, out.data_ptr()))  # noqa: E731
    ms = event_ms(fn, reps)
    nbytes = n * d * 4 + n * w * 4
    return {"shape": "pack", "n": n, "d": d, "ms": round(ms, 3), "tb_per_s": round(nbytes / ms / 1e9, 2)}


def search_shape(ix, n, d, nq, topk, reps, Qd):
    idx = torch.empty((nq, topk), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, topk), dtype=torch.float32, device="cuda")
    ms = event_ms(lambda: ix.search_device(Qd.data_ptr(), nq, topk, idx.data_ptr(), dist.data_ptr()), reps)
    w = (d + 31) // 32
    scan_ms = 2 * nq * n * w / LANE_OPS * 1e3
    return {"shape": "search", "n": n, "d": d, "nq": nq, "topk": topk, "ms": round(ms, 3),
            "queries_per_s": round(nq / ms * 1e3, 1), "valu_bound_one_scan_ms": round(scan_ms, 3),
            "fraction_of_valu_bound": round(scan_ms / ms, 3)}


def recall(got, truth):
    k = truth.shape[1]
    return float(np.mean([len(np.intersect1d(g[:k], t)) / k for g, t in zip(got, truth)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1M x 1024, topk 10 search only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    _lib.set_device(0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()  # the library's launches on the stream the events time
    torch.cuda.set_stream(stream)
    _lib.set_stream(stream.cuda_stream)
    n, nq = 1 << 20, 1024
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    for d in ((1024,) if a.quick else (256, 1024)):
        Xd, centers = clustered(n, d, 1)
        Qd, _ = clustered(nq, d, 2, centers)
        if not a.quick:
            emit(pack_shape(Xd, a.reps))
        bq = vq_amd.BinaryQuantizer(0.0)
        words = torch.empty((n, (d + 31) // 32), dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().vqhip_bq_pack_device(0.0, Xd.data_ptr(), n, d, words.data_ptr()))
        torch.cuda.synchronize()
        ix = vq_amd.BinaryIndex.from_packed(words.cpu().numpy().view(np.uint32), d, bq)
        for topk in ((10,) if a.quick else (10, 100)):
            emit(search_shape(ix, n, d, nq, topk, a.reps, Qd))
        if a.quick:
            continue
        X, Q = Xd.cpu().numpy(), Qd.cpu().numpy()
        del Xd
        flat = vq_amd.FlatIndex(X)
        truth, _ = flat.search(Q, 10)
        r = {"shape": "recall@10 vs FlatIndex euclidean", "n": n, "d": d, "nq": nq,
             "bq_only": round(recall(ix.search(Q, 10)[0], truth), 4)}
        for c in (40, 100):
            r[f"bq_rerank_{c}"] = round(recall(ix.search(Q, 10, rerank=flat, candidates=c)[0], truth), 4)
        emit(r)
        del flat, X
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
