"""4-bit scalar index figures (vq_amd.Scalar4Index, vq_amd/csrc/k_sq4index.hip) on one MI355X; prints one JSON line per
result.

  full     (i) 1024 queries over 1M x {256, 1024} rows, Euclidean and cosine, topk 10, device form, HIP events.  Four
           indexes are alternated in one process, in three rounds: Scalar4Index over the packed 4-bit codes, ScalarIndex
           over the same codes as bytes, FlatIndex over the dequantized f32 rows (the three compute the same distances and
           are compared, indices and distance bits, at the size that is timed) and AsymmetricBinaryIndex over the BQ bits
           of the same rows (threshold 0; other distances, timed only).  Per index: the median of --reps calls in each
           round.
  twostage (ii) BinaryIndex.search(Q, 10, rerank=., candidates=c), c in {40, 100, 400, 1024}, and the reranker's own
           exhaustive search, on rows around 4096 Gaussian centres (noise 0.7, threshold 0): recall@10 against FlatIndex
           (Euclidean) over the original f32 rows and host-form wall time (median of --reps, queries up, results down).
           Rerankers: FlatIndex over the f32 rows, Scalar4Index (levels 16), ScalarIndex (levels 256),
           AsymmetricBinaryIndex.  The quantizer's range comes from the data by one of two rules, both measured:
           "sigma"  min / max = mean -+ k std of all elements, k = 2.5 for 16 levels (the outermost levels of the uniform
                    16-level quantizer that is optimal for a Gaussian sit at 2.51 sigma) and k = 4 for 256 levels;
           "minmax" min / max = the least and the greatest element.
           The full search uses the "sigma" rule.

    python tools/sq4index_time.py [--reps 5] [--dims 256 1024] [--out profiles/sq4/time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_amd  # noqa: E402
from vq_amd import _lib  # noqa: E402

METRICS = (("euclidean", _lib.EUCLIDEAN), ("cosine", _lib.COSINE))
SIGMAS = {16: 2.5, 256: 4.0}


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


def wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times))


def clustered(n, d, seed, centers=None):
    """rows around 4096 Gaussian centres (the centres are returned for queries from the same distribution)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if centers is None:
        centers = torch.randn((4096, d), device="cuda", generator=g)
    lab = torch.randint(0, centers.shape[0], (n,), device="cuda", generator=g)
    X = centers[lab] + 0.7 * torch.randn((n, d), device="cuda", generator=g)
    return X.contiguous(), centers


def recall(got, truth):
    k = truth.shape[1]
    return float(np.mean([len(np.intersect1d(g[:k], t)) / k for g, t in zip(got, truth)]))


def data_range(Xd, rule, levels):
    """(min, max) of the quantizer from the rows, by the rule named in the module's docstring"""
    if rule == "minmax":
        return float(Xd.min()), float(Xd.max())
    mean, std = float(Xd.mean()), float(Xd.std())
    return mean - SIGMAS[levels] * std, mean + SIGMAS[levels] * std


def full_search(Xd, Qd, reps, emit):
    n, d = Xd.shape
    nq, topk = Qd.shape[0], 10
    mn, mx = data_range(Xd, "sigma", 16)
    sqz = vq_amd.ScalarQuantizer(mn, mx, 16)
    codes = torch.empty((n, d), dtype=torch.uint8, device="cuda")
    V = torch.empty((n, d), dtype=torch.float32, device="cuda")
    bits = torch.empty((n, (d + 31) // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sqz.quantize_device(Xd.data_ptr(), n * d, codes.data_ptr())
    sqz.dequantize_device(codes.data_ptr(), n * d, V.data_ptr())
    _lib.check(_lib.load().vqhip_bq_pack_device(0.0, Xd.data_ptr(), n, d, bits.data_ptr()))
    _lib.synchronize()
    torch.cuda.synchronize()
    q = (float(sqz._min), float(sqz._max), 16)
    for name, metric in METRICS:
        made = {"sq4": _lib.SQ4Index(None, _lib.SQ4_U8, n, d, *q, metric, dev_src=codes.data_ptr()),
                "scalar": _lib.SQIndex(None, False, n, d, *q, metric, dev_src=codes.data_ptr()),
                "abin": _lib.ABin(None, _lib.BINARY_PACKED, n, d, 0.0, 0, 1, metric, dev_src=bits.data_ptr()),
                "flat": _lib.Flat(np.empty(0, np.float32), metric, dev_rows=V.data_ptr(), shape=(n, d))}
        out = {k: (torch.empty((nq, topk), dtype=torch.int32, device="cuda"), torch.empty((nq, topk), dtype=torch.float32, device="cuda"))
               for k in made}
        rounds = {k: [] for k in made}
        for _ in range(3):
            for k, h in made.items():
                i, dd = out[k]
                rounds[k].append(round(event_ms(lambda: h.search_device(Qd.data_ptr(), nq, topk, i.data_ptr(), dd.data_ptr()), reps), 3))
        torch.cuda.synchronize()
        same = all(torch.equal(out["sq4"][0], out[k][0]) and torch.equal(out["sq4"][1].view(torch.int32), out[k][1].view(torch.int32))
                   for k in ("scalar", "flat"))
        ratios = [a / b for a, b in zip(rounds["sq4"], rounds["scalar"])]
        r = {"shape": "full search", "n": n, "d": d, "nq": nq, "topk": topk, "metric": name, "min": q[0], "max": q[1], "levels": 16,
             "rounds_ms": rounds, "ms": {k: float(np.median(v)) for k, v in rounds.items()},
             "spread_ms": {k: round(max(v) - min(v), 3) for k, v in rounds.items()},
             "sq4_over_scalar": round(float(np.median(rounds["sq4"]) / np.median(rounds["scalar"])), 4),
             "sq4_over_scalar_rounds": [round(x, 4) for x in ratios],
             "sq4_over_abin": round(float(np.median(rounds["sq4"]) / np.median(rounds["abin"])), 4),
             "sq4_over_flat": round(float(np.median(rounds["sq4"]) / np.median(rounds["flat"])), 4),
             "row_bytes": {"sq4": ((d + 7) // 8) * 4, "scalar": d, "abin": ((d + 31) // 32) * 4, "flat": 4 * d},
             "sq4_scalar_flat_agree_bit_for_bit": bool(same)}
        emit(r)
        for h in made.values():
            h.close()
    del V, codes, bits
    torch.cuda.empty_cache()


def two_stage(Xd, Qd, reps, emit):
    n, d = Xd.shape
    nq = Qd.shape[0]
    X, Q = Xd.cpu().numpy(), Qd.cpu().numpy()
    b = vq_amd.BinaryIndex(X)
    flat = vq_amd.FlatIndex(X, vq_amd.Distance.euclidean())
    truth = flat.search(Q, 10)[0]
    emit({"shape": "two-stage baseline", "n": n, "d": d, "nq": nq, "bq_alone_recall_vs_flat_euclidean": round(recall(b.search(Q, 10)[0], truth), 4),
          "bq_alone_ms": round(wall_ms(lambda: b.search(Q, 10), reps), 3)})

    def column(label, ix, bytes_per_row, extra):
        for c in (40, 100, 400, 1024):
            got = b.search(Q, 10, rerank=ix, candidates=c)[0]
            emit({"shape": "two-stage", "reranker": label, "metric": "euclidean", "n": n, "d": d, "nq": nq, "candidates": c,
                  "ms": round(wall_ms(lambda: b.search(Q, 10, rerank=ix, candidates=c), reps), 3),
                  "recall_vs_flat_euclidean": round(recall(got, truth), 4), "reranker_bytes_per_row": bytes_per_row, **extra})
        emit({"shape": "exhaustive search of the reranker", "reranker": label, "metric": "euclidean", "n": n, "d": d, "nq": nq,
              "recall_vs_flat_euclidean": round(recall(ix.search(Q, 10)[0], truth), 4), "reranker_bytes_per_row": bytes_per_row, **extra})

    column("FlatIndex over the original f32 rows", flat, 4 * d, {})
    del flat
    for rule in ("sigma", "minmax"):
        for levels, cls, rb in ((16, vq_amd.Scalar4Index, ((d + 7) // 8) * 4), (256, vq_amd.ScalarIndex, d)):
            mn, mx = data_range(Xd, rule, levels)
            ix = cls(X, vq_amd.ScalarQuantizer(mn, mx, levels), vq_amd.Distance.euclidean())
            column(cls.__name__, ix, rb, {"levels": levels, "range_rule": rule, "min": round(mn, 4), "max": round(mx, 4)})
            del ix
    column("AsymmetricBinaryIndex", vq_amd.AsymmetricBinaryIndex.from_packed(b.packed(), d, b.quantizer, vq_amd.Distance.euclidean()),
           ((d + 31) // 32) * 4, {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 1024])
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
        Xd, centers = clustered(a.n, d, 1)
        Qd, _ = clustered(a.nq, d, 2, centers)
        full_search(Xd, Qd, a.reps, emit)
        two_stage(Xd, Qd, a.reps, emit)
        del Xd, Qd
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "args": {k: v for k, v in vars(a).items() if k != "out"}, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
