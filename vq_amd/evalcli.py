"""Evaluation report in the shape of the reference's `eval_pq` / `eval_tsvq` binaries
(src/bin/eval_pq.rs:31-72, src/bin/eval_tsvq.rs:25-59, src/bin/common.rs:9-131):

    python -m vq_amd.evalcli pq   [--seed 66 --dim 384 --m 16 --k 256 --max-iters 10]
    python -m vq_amd.evalcli tsvq [--seed 66 --dim 384 --max-depth 5]
    python -m vq_amd.evalcli sq   [--seed 66 --dim 384 --levels 256]
    python -m vq_amd.evalcli bq   [--seed 66 --dim 384]
    python -m vq_amd.evalcli ivfflat [--seed 66 --dim 384 --nlist 256 --nprobe 1 8 32 --max-iters 10]
    python -m vq_amd.evalcli ivfsq   [--seed 66 --dim 384 --nlist 256 --nprobe 1 8 32 --max-iters 10 --levels 256]
    python -m vq_amd.evalcli ivfsq4  [--seed 66 --dim 384 --nlist 256 --nprobe 1 8 32 --max-iters 10 --levels 16]
    python -m vq_amd.evalcli ivfbin  [--seed 66 --dim 384 --nlist 256 --nprobe 1 8 32 --max-iters 10 --threshold 0.5 --candidates 40 100]

For every sample count of `NUM_SAMPLES` it prints the reference's three lines -- training time,
quantization time (host matrix in, f16 matrix out: what `quantize` per vector produces there)
and the mean squared reconstruction error -- and the two `BenchmarkResult` fields the binaries
compute nowhere: recall@k with `calculate_recall`'s windowed protocol (common.rs:91-130) and
the memory reduction ratio.  `--recall-full` replaces the window by an exact search of every
sampled query over all n rows (FlatIndex) on the device.  `--json` emits one `BenchmarkResult`-shaped object per line.

`sq` / `bq` follow src/bin/eval_sq.rs / eval_bq.rs: ScalarQuantizer(0, 1, levels) and
BinaryQuantizer(0.5, 0, 1), "training" being the constructor; the reference's two lines plus the
mean squared error of dequantize(quantize(x)).

`ivfflat` has no reference counterpart: it trains an IVFFlatIndex (nlist coarse centroids, Euclidean), adds every row
and reports, per nprobe, recall@k of its search against the exact search (FlatIndex) of the same <= 1000 strided
queries over all n rows, with the mean share of the rows a query scans.

`ivfbin` reports an IVFBinaryIndex with BinaryQuantizer(threshold): per nprobe, recall@k against FlatIndex over the original
rows, as returned and with rerank=FlatIndex at each candidate count, beside BinaryIndex's figures on the same rows.
`ivfsq` is `ivfflat` for an IVFScalarIndex with ScalarQuantizer(0, 1, levels) over the same coarse centroids: per nprobe,
recall@k against the exact search over the original rows (probing and quantization loss together), recall@k against the
exact search over the dequantized rows (probing loss alone), and beside them IVFFlatIndex's recall over the original rows
in the same lists.  `ivfsq4` reports the same figures for an IVFScalar4Index, `levels` at most 16 (default 16).

Data: i.i.d. Uniform[0,1) like common.rs:43-53, from the library's counter-based generator
(the reference's StdRng stream is not reproducible outside Rust).
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import numpy as np

SEED = 66                                                    # common.rs:9
NUM_SAMPLES = [1_000, 5_000, 10_000, 50_000, 100_000, 1_000_000]  # common.rs:10
DIM, M, K, MAX_ITERS = 384, 16, 256, 10                      # common.rs:12-15


def reconstruction_error(original: np.ndarray, reconstructed: np.ndarray) -> float:
    """common.rs:61-78: sum of squared differences / number of elements"""
    diff = original.astype(np.float32) - reconstructed.astype(np.float32)
    return float((diff * diff).sum(dtype=np.float64) / original.size)


def recall_at_k(original: np.ndarray, approx: np.ndarray, k: int = 10) -> float:
    """common.rs:91-130: <= 1000 strided queries; neighbours searched inside a 5000-row window
    around the query (the whole set when n <= 10 000); true neighbours by Euclidean distance on
    the originals, approximate ones on the reconstructions; ties keep index order (stable sort)."""
    n = original.shape[0]
    eval_samples = min(n, 1000)
    step = max(n // eval_samples, 1)
    window = 5000 if n > 10_000 else n
    total = 0.0
    for i in range(0, n, step):
        lo, hi = max(i - window // 2, 0), min(i + window // 2, n)
        idx = np.arange(lo, hi)
        idx = idx[idx != i]
        d_true = ((original[idx] - original[i]) ** 2).sum(axis=1)
        d_appr = ((approx[idx] - approx[i]) ** 2).sum(axis=1)
        t = idx[np.argsort(d_true, kind="stable")[:k]]
        a = idx[np.argsort(d_appr, kind="stable")[:k]]
        total += len(np.intersect1d(t, a)) / k
    return total / (n // step)


def recall_at_k_full(original: np.ndarray, approx_f16: np.ndarray, k: int = 10) -> float:
    """recall@k without the window: the same <= 1000 strided queries, each searched exactly (FlatIndex, squared
    Euclidean) over ALL n originals (f32 index) and over all n f16 reconstructions (f16 index, the query being its own
    reconstruction).  A query's own row is excluded by searching k + 1 and dropping that row where it is returned,
    else the last one; ties go to the lower row."""
    from .distance import Distance
    from .flat import FlatIndex

    n = original.shape[0]
    k = min(k, n - 1)
    step = max(n // min(n, 1000), 1)
    qi = np.arange(0, n, step)
    dist = Distance.squared_euclidean()

    def neighbours(rows, queries):
        idx, _ = FlatIndex(rows, dist).search(queries, k + 1)
        out = np.empty((len(qi), k), idx.dtype)
        for j, i in enumerate(qi):
            hit = np.flatnonzero(idx[j] == i)
            out[j] = np.delete(idx[j], hit[0]) if hit.size else idx[j, :k]
        return out

    t = neighbours(original, original[qi])
    a = neighbours(approx_f16, approx_f16[qi].astype(np.float32))
    return float(np.mean([len(np.intersect1d(t[j], a[j])) / k for j in range(len(qi))]))


def _report(title, make_quantizer, args, code_bytes_per_vector):
    from . import _lib

    print(title)
    print("=" * len(title))
    for n in args.samples:
        X = _lib.synth_uniform_host(n, args.dim, args.seed, 0)
        t0 = time.perf_counter()
        q = make_quantizer(X)
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        f16 = q.quantize_batch(X)
        quant_ms = (time.perf_counter() - t0) * 1e3
        rec = f16.astype(np.float32)
        err = reconstruction_error(X, rec)
        res = {"n_samples": n, "n_dims": args.dim, "training_time_ms": train_ms,
               "quantization_time_ms": quant_ms, "reconstruction_error": err}
        if args.recall_k > 0:
            res["recall"] = (recall_at_k_full(X, f16, args.recall_k) if args.recall_full
                             else recall_at_k(X, rec, args.recall_k))
        # the reference keeps the f16 reconstruction (2 bytes per dimension); the codes are smaller
        res["memory_reduction_ratio"] = 4.0 * args.dim / (2.0 * args.dim)
        res["memory_reduction_ratio_codes"] = 4.0 * args.dim / code_bytes_per_vector(q)
        if args.json:
            print(json.dumps(res))
            continue
        print(f"\nSamples: {n}")
        print(f"  Training time: {train_ms:.0f} ms")
        print(f"  Quantization time: {quant_ms:.0f} ms")
        print(f"  Reconstruction error: {err:.6f}")
        if "recall" in res:
            full = " (exact, all rows)" if args.recall_full else ""
            print(f"  Recall@{args.recall_k}{full}: {res['recall']:.4f}")
        print(f"  Memory reduction: {res['memory_reduction_ratio']:.1f}x as f16, "
              f"{res['memory_reduction_ratio_codes']:.1f}x as codes")


def _report_elementwise(title, make_quantizer, args):
    """eval_sq.rs / eval_bq.rs: the constructor timed as training, one batch quantize of the whole matrix (what
    quantize per vector gives), then the reconstruction error of dequantize"""
    from . import _lib

    print(title)
    print("=" * len(title))
    for n in args.samples:
        X = _lib.synth_uniform_host(n, args.dim, args.seed, 0)
        t0 = time.perf_counter()
        q = make_quantizer()
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        codes = q.quantize_batch(X)
        quant_ms = (time.perf_counter() - t0) * 1e3
        err = reconstruction_error(X, q.dequantize_batch(codes))
        if args.json:
            print(json.dumps({"n_samples": n, "n_dims": args.dim, "training_time_ms": train_ms,
                              "quantization_time_ms": quant_ms, "reconstruction_error": err,
                              "memory_reduction_ratio": 4.0}))
            continue
        print(f"\nSamples: {n}")
        print(f"  Training time: {train_ms:.0f} ms")
        print(f"  Quantization time: {quant_ms:.0f} ms")
        print(f"  Reconstruction error: {err:.6f}")


def _report_ivfflat(args):
    """recall@k of IVFFlatIndex.search against FlatIndex.search over the same rows, per nprobe"""
    from . import _lib
    from .flat import FlatIndex
    from .ivf_flat import IVFFlatIndex

    title = "IVF-Flat Index Evaluation"
    print(title)
    print("=" * len(title))
    for n in args.samples:
        X = _lib.synth_uniform_host(n, args.dim, args.seed, 0)
        nlist = min(args.nlist, n)
        k = min(args.recall_k, n)
        t0 = time.perf_counter()
        ix = IVFFlatIndex.train(X, nlist, args.max_iters, seed=args.seed)
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ix.add(X)
        add_ms = (time.perf_counter() - t0) * 1e3
        Q = X[::max(n // min(n, 1000), 1)]
        exact = FlatIndex(X).search(Q, k)[0]
        sizes = ix.list_sizes().astype(np.int64)
        if not args.json:
            print(f"\nSamples: {n}")
            print(f"  Training time: {train_ms:.0f} ms")
            print(f"  Add time: {add_ms:.0f} ms")
        for nprobe in args.nprobe:
            p = min(nprobe, nlist)
            t0 = time.perf_counter()
            got = ix.search(Q, topk=k, nprobe=p)[0]
            search_ms = (time.perf_counter() - t0) * 1e3
            recall = float(np.mean([len(np.intersect1d(got[j], exact[j])) / k for j in range(len(Q))]))
            scanned = float(sizes[ix.probe(Q, p)].sum() / (len(Q) * n))
            if args.json:
                print(json.dumps({"n_samples": n, "n_dims": args.dim, "nlist": nlist, "nprobe": p, "training_time_ms": train_ms,
                                  "add_time_ms": add_ms, "search_time_ms": search_ms, "recall": recall, "scanned_share": scanned}))
            else:
                print(f"  nprobe {p}: Recall@{k} {recall:.4f}, {100 * scanned:.1f}% of the rows scanned, {search_ms:.0f} ms")
        ix.close()


def _report_ivfsq(args, four_bit: bool = False):
    """recall@k of IVFScalarIndex.search against FlatIndex.search over the original and over the dequantized rows, per
    nprobe, beside IVFFlatIndex's over the original rows in the same lists; four_bit: of IVFScalar4Index.search"""
    from . import _lib
    from .flat import FlatIndex
    from .ivf_flat import IVFFlatIndex
    from .ivf_scalar import IVFScalarIndex
    from .ivf_scalar4 import IVFScalar4Index
    from .sq import ScalarQuantizer

    title = "IVF-Scalar4 Index Evaluation" if four_bit else "IVF-Scalar Index Evaluation"
    print(title)
    print("=" * len(title))
    sq = ScalarQuantizer(0.0, 1.0, args.levels)

    def recall(got, want, k):
        return float(np.mean([len(np.intersect1d(got[j], want[j])) / k for j in range(len(want))]))

    for n in args.samples:
        X = _lib.synth_uniform_host(n, args.dim, args.seed, 0)
        nlist = min(args.nlist, n)
        k = min(args.recall_k, n)
        t0 = time.perf_counter()
        ix = (IVFScalar4Index if four_bit else IVFScalarIndex).train(X, nlist, sq, args.max_iters, seed=args.seed)
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ix.add(X)
        add_ms = (time.perf_counter() - t0) * 1e3
        flat = IVFFlatIndex(ix.coarse_centroids, ix.distance)
        flat.add_rows(ix.list_ids, X)
        Q = X[::max(n // min(n, 1000), 1)]
        exact = FlatIndex(X).search(Q, k)[0]
        exact_deq = FlatIndex(sq.dequantize_batch(ix.codes() if four_bit else ix.codes)).search(Q, k)[0]
        sizes = ix.list_sizes().astype(np.int64)
        if not args.json:
            print(f"\nSamples: {n}")
            print(f"  Training time: {train_ms:.0f} ms")
            print(f"  Add time: {add_ms:.0f} ms")
            print(f"  Index bytes per row: {4 * ((args.dim + 7) // 8) if four_bit else args.dim} (IVF-Flat f32: {4 * args.dim})")
        for nprobe in args.nprobe:
            p = min(nprobe, nlist)
            t0 = time.perf_counter()
            got = ix.search(Q, topk=k, nprobe=p)[0]
            search_ms = (time.perf_counter() - t0) * 1e3
            r, r_deq = recall(got, exact, k), recall(got, exact_deq, k)
            r_flat = recall(flat.search(Q, topk=k, nprobe=p)[0], exact, k)
            scanned = float(sizes[ix.probe(Q, p)].sum() / (len(Q) * n))
            if args.json:
                print(json.dumps({"n_samples": n, "n_dims": args.dim, "nlist": nlist, "nprobe": p, "levels": args.levels,
                                  "training_time_ms": train_ms, "add_time_ms": add_ms, "search_time_ms": search_ms, "recall": r,
                                  "recall_over_dequantized": r_deq, "ivfflat_recall": r_flat, "scanned_share": scanned}))
            else:
                print(f"  nprobe {p}: Recall@{k} {r:.4f} over the original rows, {r_deq:.4f} over the dequantized rows "
                      f"(IVF-Flat {r_flat:.4f}), {100 * scanned:.1f}% of the rows scanned, {search_ms:.0f} ms")
        ix.close()
        flat.close()


def _report_ivfbin(args):
    """recall@k of IVFBinaryIndex.search against FlatIndex.search over the original rows, per nprobe, as returned and with
    rerank=FlatIndex at two candidate counts, beside BinaryIndex's over the same rows: the probing loss apart from the
    binarisation loss"""
    from . import _lib
    from .binary import BinaryIndex
    from .bq import BinaryQuantizer
    from .flat import FlatIndex
    from .ivf_binary import IVFBinaryIndex

    title = "IVF-Binary Index Evaluation"
    print(title)
    print("=" * len(title))
    bq = BinaryQuantizer(args.threshold)

    def recall(got, want, k):
        return float(np.mean([len(np.intersect1d(got[j], want[j])) / k for j in range(len(want))]))

    for n in args.samples:
        X = _lib.synth_uniform_host(n, args.dim, args.seed, 0)
        nlist = min(args.nlist, n)
        k = min(args.recall_k, n)
        t0 = time.perf_counter()
        ix = IVFBinaryIndex.train(X, nlist, bq, args.max_iters, seed=args.seed)
        train_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ix.add(X)
        add_ms = (time.perf_counter() - t0) * 1e3
        bx = BinaryIndex.from_packed(ix.packed(), args.dim, bq, ix.distance)
        flat = FlatIndex(X)
        Q = X[::max(n // min(n, 1000), 1)]
        exact = flat.search(Q, k)[0]
        cands = [c for c in args.candidates if k <= c <= min(n, 1024)]
        r_bin = recall(bx.search(Q, k)[0], exact, k)
        r_bin_rr = {c: recall(bx.search(Q, k, rerank=flat, candidates=c)[0], exact, k) for c in cands}
        sizes = ix.list_sizes().astype(np.int64)
        if not args.json:
            print(f"\nSamples: {n}")
            print(f"  Training time: {train_ms:.0f} ms")
            print(f"  Add time: {add_ms:.0f} ms")
            print(f"  Index bytes per row: {4 * ((args.dim + 31) // 32)} (f32 rows: {4 * args.dim})")
            print(f"  BinaryIndex (every row): Recall@{k} {r_bin:.4f}" + "".join(f", {v:.4f} reranked from {c}" for c, v in r_bin_rr.items()))
        for nprobe in args.nprobe:
            p = min(nprobe, nlist)
            t0 = time.perf_counter()
            got = ix.search(Q, topk=k, nprobe=p)[0]
            search_ms = (time.perf_counter() - t0) * 1e3
            r = recall(got, exact, k)
            r_rr = {c: recall(ix.search(Q, topk=k, nprobe=p, rerank=flat, candidates=c)[0], exact, k) for c in cands}
            scanned = float(sizes[ix.probe(Q, p)].sum() / (len(Q) * n))
            if args.json:
                print(json.dumps({"n_samples": n, "n_dims": args.dim, "nlist": nlist, "nprobe": p, "threshold": args.threshold,
                                  "training_time_ms": train_ms, "add_time_ms": add_ms, "search_time_ms": search_ms, "recall": r,
                                  "recall_reranked": {str(c): v for c, v in r_rr.items()}, "binary_recall": r_bin,
                                  "binary_recall_reranked": {str(c): v for c, v in r_bin_rr.items()}, "scanned_share": scanned}))
            else:
                print(f"  nprobe {p}: Recall@{k} {r:.4f}" + "".join(f", {v:.4f} reranked from {c}" for c, v in r_rr.items()) +
                      f", {100 * scanned:.1f}% of the rows scanned, {search_ms:.0f} ms")
        ix.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="vq_amd.evalcli")
    sub = ap.add_subparsers(dest="alg", required=True)
    for name in ("sq", "bq"):
        p = sub.add_parser(name)
        p.add_argument("--seed", type=int, default=SEED)
        p.add_argument("--dim", type=int, default=DIM)
        p.add_argument("--samples", type=int, nargs="+", default=NUM_SAMPLES)
        p.add_argument("--json", action="store_true")
        if name == "sq":
            p.add_argument("--levels", type=int, default=256)
    for name in ("pq", "tsvq"):
        p = sub.add_parser(name)
        p.add_argument("--seed", type=int, default=SEED)
        p.add_argument("--dim", type=int, default=DIM)
        p.add_argument("--samples", type=int, nargs="+", default=NUM_SAMPLES)
        p.add_argument("--recall-k", type=int, default=10, help="0 skips the recall estimate")
        p.add_argument("--recall-full", action="store_true",
                       help="recall@k by exact search over all rows on the device instead of the windowed protocol")
        p.add_argument("--json", action="store_true")
        if name == "pq":
            p.add_argument("--m", type=int, default=M)
            p.add_argument("--k", type=int, default=K)
            p.add_argument("--max-iters", type=int, default=MAX_ITERS)
        else:
            p.add_argument("--max-depth", type=int, default=5)
    for name in ("ivfflat", "ivfsq", "ivfsq4", "ivfbin"):
        p = sub.add_parser(name)
        p.add_argument("--seed", type=int, default=SEED)
        p.add_argument("--dim", type=int, default=DIM)
        p.add_argument("--samples", type=int, nargs="+", default=NUM_SAMPLES)
        p.add_argument("--nlist", type=int, default=256)
        p.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
        p.add_argument("--max-iters", type=int, default=MAX_ITERS)
        p.add_argument("--recall-k", type=int, default=10)
        p.add_argument("--json", action="store_true")
        if name == "ivfsq":
            p.add_argument("--levels", type=int, default=256)
        if name == "ivfsq4":
            p.add_argument("--levels", type=int, default=16)
        if name == "ivfbin":
            p.add_argument("--threshold", type=float, default=0.5)
            p.add_argument("--candidates", type=int, nargs="+", default=[40, 100])
    args = ap.parse_args(argv)
    if args.alg == "ivfflat":
        _report_ivfflat(args)
        return 0
    if args.alg in ("ivfsq", "ivfsq4"):
        _report_ivfsq(args, four_bit=args.alg == "ivfsq4")
        return 0
    if args.alg == "ivfbin":
        _report_ivfbin(args)
        return 0
    from . import TSVQ, BinaryQuantizer, Distance, ProductQuantizer, ScalarQuantizer

    if args.alg == "sq":
        _report_elementwise("Scalar Quantizer Evaluation", lambda: ScalarQuantizer(0.0, 1.0, args.levels), args)
    elif args.alg == "bq":
        _report_elementwise("Binary Quantizer Evaluation", lambda: BinaryQuantizer(0.5, 0, 1), args)
    elif args.alg == "pq":
        _report("Product Quantizer Evaluation",
                lambda X: ProductQuantizer(X, args.m, args.k, args.max_iters, Distance.euclidean(), args.seed),
                args, lambda q: q.num_subspaces)
    else:
        _report("TSVQ Evaluation", lambda X: TSVQ(X, args.max_depth, Distance.euclidean()), args,
                lambda q: max(1, (int(q.tree[0].shape[0]).bit_length() + 7) // 8))
    return 0


if __name__ == "__main__":
    sys.exit(main())
