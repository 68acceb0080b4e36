"""Asymmetric binary index figures (vq_amd.AsymmetricBinaryIndex, vq_amd/csrc/k_abin.hip) on one MI355X; prints one JSON
line per result.

  full     (i) 1024 queries over 1M x {256, 1024} bits, Euclidean and cosine, topk 10, device form, HIP events.  Three
           indexes over the same rows are alternated in one process, in three rounds: AsymmetricBinaryIndex over the
           packed words, ScalarIndex over the bits as 0/1 bytes (ScalarQuantizer(low, high, 2)) and FlatIndex over the
           dequantized f32 rows.  The latter two are the yardsticks.  Per index: the median of --reps calls in each round,
           and the three indexes' results compared (indices and distance bits) at the size that is timed.
  twostage (ii) BinaryIndex.search(Q, 10, rerank=abin, candidates=c), c in {40, 100, 400, 1024}, abin under Euclidean and
           cosine, on rows around 4096 Gaussian centres (noise 0.7, threshold 0): host-form wall time (median of --reps,
           queries up, results down) and recall@10 against FlatIndex over the original f32 rows, under Euclidean and under
           the reranker's own metric; beside it the same call with rerank=FlatIndex over the original rows, and BQ alone.
           With (low, high) = (0, 1) also the symmetric decode -a / +a, reached by mapping the query (recall only).

    python tools/abin_time.py [--reps 5] [--dims 256 1024] [--low 0 --high 1] [--out profiles/abin/time.json]
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


def full_search(Xd, Qd, low, high, reps, emit):
    n, d = Xd.shape
    nq, topk = Qd.shape[0], 10
    bits = Xd >= 0
    words = torch.empty((n, (d + 31) // 32), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().vqhip_bq_pack_device(0.0, Xd.data_ptr(), n, d, words.data_ptr()))
    codes = bits.to(torch.uint8).contiguous()
    V = torch.where(bits, float(high), float(low)).to(torch.float32).contiguous()
    del bits
    torch.cuda.synchronize()
    for name, metric in METRICS:
        made = {"abin": _lib.ABin(None, _lib.BINARY_PACKED, n, d, 0.0, low, high, metric, dev_src=words.data_ptr()),
                "scalar": _lib.SQIndex(None, False, n, d, float(low), float(high), 2, metric, dev_src=codes.data_ptr()),
                "flat": _lib.Flat(np.empty(0, np.float32), metric, dev_rows=V.data_ptr(), shape=(n, d))}
        out = {k: (torch.empty((nq, topk), dtype=torch.int32, device="cuda"), torch.empty((nq, topk), dtype=torch.float32, device="cuda"))
               for k in made}
        rounds = {k: [] for k in made}
        for _ in range(3):
            for k, h in made.items():
                i, dd = out[k]
                rounds[k].append(round(event_ms(lambda: h.search_device(Qd.data_ptr(), nq, topk, i.data_ptr(), dd.data_ptr()), reps), 3))
        torch.cuda.synchronize()
        same = all(torch.equal(out["abin"][0], out[k][0]) and torch.equal(out["abin"][1].view(torch.int32), out[k][1].view(torch.int32))
                   for k in ("scalar", "flat"))
        r = {"shape": "full search", "n": n, "d": d, "nq": nq, "topk": topk, "metric": name, "low": low, "high": high,
             "rounds_ms": rounds, "ms": {k: float(np.median(v)) for k, v in rounds.items()},
             "spread_ms": {k: round(max(v) - min(v), 3) for k, v in rounds.items()},
             "abin_over_scalar": round(float(np.median(rounds["abin"]) / np.median(rounds["scalar"])), 3),
             "abin_over_flat": round(float(np.median(rounds["abin"]) / np.median(rounds["flat"])), 3),
             "row_bytes": {"abin": ((d + 31) // 32) * 4, "scalar": d, "flat": 4 * d},
             "three_indexes_agree_bit_for_bit": bool(same)}
        emit(r)
        for h in made.values():
            h.close()
    del V, codes
    torch.cuda.empty_cache()
    return words


def two_stage(Xd, Qd, words, low, high, reps, emit):
    n, d = Xd.shape
    nq = Qd.shape[0]
    X, Q = Xd.cpu().numpy(), Qd.cpu().numpy()
    W = words.cpu().numpy().view(np.uint32)
    bq = vq_amd.BinaryQuantizer(0.0, low, high)
    b = vq_amd.BinaryIndex.from_packed(W, d, bq)
    flat = vq_amd.FlatIndex(X, vq_amd.Distance.euclidean())
    truth = {"euclidean": flat.search(Q, 10)[0]}
    fc = vq_amd.FlatIndex(X, vq_amd.Distance.cosine())
    truth["cosine"] = fc.search(Q, 10)[0]
    del fc
    emit({"shape": "two-stage baseline", "n": n, "d": d, "nq": nq, "bq_alone_recall_vs_flat_euclidean": round(recall(b.search(Q, 10)[0], truth["euclidean"]), 4),
          "bq_alone_ms": round(wall_ms(lambda: b.search(Q, 10), reps), 3)})
    for c in (40, 100, 400, 1024):
        got = b.search(Q, 10, rerank=flat, candidates=c)[0]
        emit({"shape": "two-stage", "reranker": "FlatIndex over the original f32 rows", "metric": "euclidean", "n": n, "d": d, "nq": nq,
              "candidates": c, "ms": round(wall_ms(lambda: b.search(Q, 10, rerank=flat, candidates=c), reps), 3),
              "recall_vs_flat_euclidean": round(recall(got, truth["euclidean"]), 4), "reranker_bytes_per_row": 4 * d})
    for name, _ in METRICS:
        abin = vq_amd.AsymmetricBinaryIndex.from_packed(W, d, bq, vq_amd.Distance(name))
        for c in (40, 100, 400, 1024):
            got = b.search(Q, 10, rerank=abin, candidates=c)[0]
            emit({"shape": "two-stage", "reranker": "AsymmetricBinaryIndex", "metric": name, "low": low, "high": high, "n": n, "d": d,
                  "nq": nq, "candidates": c, "ms": round(wall_ms(lambda: b.search(Q, 10, rerank=abin, candidates=c), reps), 3),
                  "recall_vs_flat_euclidean": round(recall(got, truth["euclidean"]), 4),
                  "recall_vs_flat_same_metric": round(recall(got, truth[name]), 4),
                  "reranker_bytes_per_row": ((d + 31) // 32) * 4 + (4 if name == "cosine" else 0)})
        got = abin.search(Q, 10)[0]  # the exhaustive asymmetric search: what the short list converges to
        emit({"shape": "asymmetric search alone", "metric": name, "low": low, "high": high, "n": n, "d": d, "nq": nq,
              "recall_vs_flat_euclidean": round(recall(got, truth["euclidean"]), 4),
              "recall_vs_flat_same_metric": round(recall(got, truth[name]), 4)})
        if name == "euclidean" and (low, high) == (0, 1):
            # The symmetric decode -a / +a, which u8 (low, high) cannot name, through the query: |q - a (2 b - 1)|^2 =
            # (2 a)^2 |(q + a) / (2 a) - b|^2, so the mapped query ranks the 0/1 rows as q ranks the -a / +a rows.
            a = float(np.abs(X).mean())
            Qm = ((Q + np.float32(a)) / np.float32(2 * a)).astype(np.float32)
            for c in (40, 100, 400, 1024):
                short = b.search(Q, c)[0]
                got = abin.rerank(Qm, short, 10)[0]
                emit({"shape": "two-stage", "reranker": "AsymmetricBinaryIndex, query mapped to (q + a) / (2 a)", "metric": name, "low": low,
                      "high": high, "a": round(a, 4), "n": n, "d": d, "nq": nq, "candidates": c,
                      "recall_vs_flat_euclidean": round(recall(got, truth["euclidean"]), 4)})
            emit({"shape": "asymmetric search alone", "reranker": "query mapped to (q + a) / (2 a)", "metric": name, "low": low, "high": high,
                  "a": round(a, 4), "n": n, "d": d, "nq": nq,
                  "recall_vs_flat_euclidean": round(recall(abin.search(Qm, 10)[0], truth["euclidean"]), 4)})
        del abin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--low", type=int, default=0)
    ap.add_argument("--high", type=int, default=1)
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
        words = full_search(Xd, Qd, a.low, a.high, a.reps, emit)
        two_stage(Xd, Qd, words, a.low, a.high, a.reps, emit)
        del Xd, Qd, words
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"gpu": torch.cuda.get_device_name(0), "args": vars(a), "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
