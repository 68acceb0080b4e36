#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): PQ m=8, k=256, L2 on 1,000,000 x 128 f32 rows PER GPU
(weak scaling), synthetic Uniform[0,1) rows generated on the device (reference harness
distribution, src/bin/common.rs:43-53), codebooks trained by a few untimed Lloyd iterations.

A "step" is one encode pass (nearest-centroid assignment of every resident row in all m
subspaces -> one code byte per subspace) with inputs already resident in HBM.  K steps are
timed between barrier + synchronize brackets; value = rows encoded by all ranks / max time.
The same run also times Lloyd iterations (assign + fused update + all-reduce + finalize, the
loop's decisions on the device: vqhip_kmeans_run[_sharded]) and, on rank 0 at N=1, the other
BASELINE configurations (C1, C3, C4: a `configs` block, each with its own roofline) and the
CPU restatement of the reference (oracle/, labelled "port").

    --config C5        BASELINE configs[4]'s per-GPU share: 12.5M rows per GPU, m=16 (the 8-GPU job)
    --collective torch the all-reduce through torch.distributed instead of below the C ABI
    --dump-outputs DIR the codes of the last timed step (and the codebooks they were encoded with) as DIR/*.npy in
                       float32, for output-for-output comparison of two builds (inputs are seeded: same arguments, same inputs)

One JSON line on stdout (rank 0).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# BASELINE.md section 3 / SURVEY.md section 8(d)
PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense (MI355X_MICROARCH.md)
# The bf16x3-split engine forms every fp32 product from SIX bf16 products on the bf16 matrix pipe: the roofline of the
# kernel that does the work is that pipe's dense rate / 6, in fp32-equivalent (algorithmic) flop
PEAK_BF16X3_EQUIV_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
CYCLES_PER_ISSUE_LONE_WAVE = 5.3  # profiles/ubench/valu_issue.hip: one wave per SIMD issues an instruction of any kind every 4.4-5.4 cycles
PEAK_HBM_GBS = 8000.0
N_PER_GPU, DIM, M, K = 1_000_000, 128, 8, 256
DATA_SEED, TRAIN_ITERS = 66, 4
PREWARM_STEPS = 200  # untimed encode passes in front of the warmup (GPU clocks back up after the host-side gap)
SIDE_STEPS = 20  # passes of the side timings (cold passes, f16 output, the N > 1 blocks): --steps sets the headline's alone
WORKLOADS = {  # BASELINE.json configs[1] and configs[4] (per-GPU share of the 100M x 128 job on 8 GPUs)
    "C2": dict(rows=1_000_000, dim=128, m=8, k=256, label="BASELINE.json configs[1]"),
    "C5": dict(rows=12_500_000, dim=128, m=16, k=256, label="BASELINE.json configs[4], one GPU's rows of 100M x 128 on 8 GPUs"),
}


def cpu_baseline(m, k, dim, codebooks, target_seconds=12.0):
    """The reference's encode loop (src/pq.rs:167-199, driven one vector at a time on ONE
    thread by src/bin/eval_pq.rs:54-57) as restated by the oracle, timed on this host."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import oracle as O  # cpu_baseline leg only
    from vq_amd import _lib

    orc = O.get()
    probe = 2000
    X = _lib.synth_uniform_host(probe, dim, DATA_SEED, 0)
    t0 = time.perf_counter()
    orc.pq_encode(O.SQUARED_EUCLIDEAN, X, codebooks, want_f16=True, threads=1)
    per_row = (time.perf_counter() - t0) / probe
    n = int(min(200_000, max(probe, target_seconds / max(per_row, 1e-9))))
    X = _lib.synth_uniform_host(n, dim, DATA_SEED, 0)
    t0 = time.perf_counter()
    orc.pq_encode(O.SQUARED_EUCLIDEAN, X, codebooks, want_f16=True, threads=1)
    dt = time.perf_counter() - t0
    out = {"value": n / dt, "unit": "vectors/s", "cores": 1, "kind": "port",
           "sample": f"first {n} rows of the same synthetic matrix, same codebooks; single-thread "
                     "encode like the reference (src/bin/eval_pq.rs:54-57)"}
    # context: all host cores over rows (the reference does NOT do this for encode)
    nt = orc.max_threads()
    t0 = time.perf_counter()
    orc.pq_encode(O.SQUARED_EUCLIDEAN, X, codebooks, want_f16=True, threads=nt)
    out["all_cores_value"] = n / (time.perf_counter() - t0)
    out["all_cores"] = nt
    # SURVEY.md 8(d) variant B ("generous"): same source built -O3 -march=native on this host,
    # rows over all cores -- a stand-in for the reference's `simd` + rayon-over-rows best case
    try:
        fast = O.get(native=True)
        fast.pq_encode(O.SQUARED_EUCLIDEAN, X[:2000], codebooks, want_f16=True, threads=nt)
        t0 = time.perf_counter()
        fast.pq_encode(O.SQUARED_EUCLIDEAN, X, codebooks, want_f16=True, threads=nt)
        out["generous_value"] = n / (time.perf_counter() - t0)
        out["generous_note"] = f"-O3 -march=native build, {nt} threads over rows"
    except Exception as e:  # the native build is best effort (needs gcc on the bench host)
        out["generous_note"] = f"native build unavailable: {e}"
    # k-means iteration, faithful threading (SURVEY.md 8(d) variant A): assignment over all host cores
    # like rayon's par_iter (src/core/vector.rs:417-423), update serial, subspaces one after the other
    # (src/pq.rs:121), on a bounded sample of the same matrix; a Lloyd iteration is linear in the rows
    nk = min(100_000, n)
    Xk = X[:nk]
    sd = dim // m
    t0 = time.perf_counter()
    for s_ in range(m):
        orc.lloyd_step(Xk[:, s_ * sd:(s_ + 1) * sd], codebooks[s_], threads=nt)
    dtk = time.perf_counter() - t0
    out["kmeans"] = {"rows": nk, "ms_per_iter": dtk * 1e3, "threads": nt,
                     "iter_per_s_extrapolated_to_workload_rows": 1.0 / (dtk * N_PER_GPU / nk),
                     "note": "one Lloyd iteration over all m subspaces on the sample, assign parallel / update serial"}
    return out


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` from the committed rocprofv3 PMC summary (separate
    --pmc FETCH_SIZE / WRITE_SIZE passes, profiles/run_profile.sh).  Units are KiB; FETCH_SIZE is
    doubled as MI355X_MICROARCH.md prescribes for gfx950 (it reports half of a coalesced stream).
    Returns (bytes or None, source)."""
    import glob

    base = kernel_name.split("<")[0]
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "*pmc_summary.json")), reverse=True):
        try:
            summ = json.load(open(path))
            d = summ.get(kernel_name.replace(" ", "")) or summ.get(base)  # the exact instantiation when the summary has it
            if d and "FETCH_SIZE" in d and "WRITE_SIZE" in d:
                per = lambda c: d[c].get("avg_largest", d[c]["avg_per_launch"])  # the launches of the bench line's size (summarize.py)
                kib = 2.0 * per("FETCH_SIZE") + per("WRITE_SIZE")
                return kib * 1024.0, os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def tsvq_build_traffic(rows):
    """HBM bytes per TSVQ build at C4's shape from the newest committed PMC pass over the build's kernels
    (tools/evidence_r6.sh: separate FETCH_SIZE / WRITE_SIZE runs of tools/tsvq_time.py, FETCH doubled as the guide prescribes
    for gfx950); rows = "c4" (Uniform[0,1)) or "normal" (N(0,1)).  Returns (bytes or None, source)."""
    import glob

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "tsvq_build_pmc_summary.json")), reverse=True):
        try:
            d = json.load(open(path)).get(rows)
            if d and d.get("hbm_bytes_per_build"):
                return float(d["hbm_bytes_per_build"]), os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def screen_kernel_name(sd, k, training):
    """the pipelined screen's instantiation for a shape (8 tiles, sub_dim 8 or 16), as profiles/summarize.py names it; None elsewhere"""
    if sd in (8, 16) and 225 <= k <= 256:
        return f"k_assign_screen_bf16_x32p<{sd},8,{'true' if training else 'false'}>"
    return None


def tsvq_traffic_fields(rows, algorithmic_bytes):
    t, src = tsvq_build_traffic(rows)
    return {"traffic": t, "traffic_source": src, "traffic_over_algorithmic": (t / algorithmic_bytes if t else None)}


def strided_init(n_global, m, k):
    import numpy as np

    return np.array([[(j * (n_global // k) + s) % n_global for j in range(k)] for s in range(m)], np.int64)


DUMP_BUDGET_BYTES = 60 << 20  # --dump-outputs: at most this much in all (64 MB with room for the headers)
DUMP_SAMPLE_SEED = 20240613


def dump_codes_rows(n, m, world):
    """rows of a rank's (n, m) code matrix that --dump-outputs writes: all of them when every rank's codes fit the budget as
    float32, else a fixed, seeded, sorted sample (the same rows on every run with the same arguments)"""
    import numpy as np

    per_rank = (DUMP_BUDGET_BYTES - (1 << 20)) // max(1, world)  # 1 MB kept for the codebooks
    if n * 4 * m <= per_rank:
        return None
    return np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, per_rank // (4 * m + 8), replace=False))  # + f64 index


def dump_outputs(dirname, rank, codes, codebooks, world, row_offset=0):
    """--dump-outputs: rank r's codes as `codes.npy` (rank 0) / `codes_rank<r>.npy`, float32 (n_or_sample, m); the sampled
    rows' global indices as `codes_rows[_rank<r>].npy` (float64) when the codes are sampled; `codebooks.npy` (float32,
    (m, k, sub_dim)) from rank 0.  Returns the names written."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    codes = np.asarray(codes)
    suffix = "" if rank == 0 else f"_rank{rank}"
    names = []
    rows = dump_codes_rows(codes.shape[0], codes.shape[1], world)
    if rows is not None:
        codes = codes[rows]
        np.save(os.path.join(dirname, f"codes_rows{suffix}.npy"), (rows + row_offset).astype(np.float64))
        names.append(f"codes_rows{suffix}")
    np.save(os.path.join(dirname, f"codes{suffix}.npy"), codes.astype(np.float32))
    names.append(f"codes{suffix}")
    if rank == 0:
        np.save(os.path.join(dirname, "codebooks.npy"), np.asarray(codebooks, np.float32))
        names.append("codebooks")
    return names


def pmc_issue_model(kernel_name):
    """Instruction-issue share of `kernel_name`'s run time from the committed PMC summary: a lone wave per SIMD issues one
    instruction every ~5.3 cycles whatever its kind, so (instructions per SIMD) x 5.3 cycles against the kernel's own
    cycle count (GRBM_GUI_ACTIVE, summed over the 8 XCDs) says how much of the kernel is issue slots.  SQ_INSTS_VALU
    counts the MFMAs too.  Returns a dict or None."""
    import glob

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "*pmc_summary.json")), reverse=True):
        try:
            d = json.load(open(path)).get(kernel_name.replace(" ", ""))
            if d and "SQ_INSTS_VALU" in d and "GRBM_GUI_ACTIVE" in d:
                per = lambda c: d[c].get("avg_largest", d[c]["avg_per_launch"]) if c in d else 0.0
                insts = per("SQ_INSTS_VALU") + per("SQ_INSTS_SALU")
                cycles = per("GRBM_GUI_ACTIVE") / 8.0
                return {"instructions_per_launch": insts, "mfma_per_launch": per("SQ_INSTS_MFMA") or None,
                        "simds": 1024, "cycles_per_issue": CYCLES_PER_ISSUE_LONE_WAVE, "kernel_cycles": cycles,
                        "frac_of_kernel": insts / 1024.0 * CYCLES_PER_ISSUE_LONE_WAVE / cycles, "source": os.path.relpath(path, ROOT)}
        except Exception:
            continue
    return None


def mfma_roofline(flop, ms, kernel=None, extra=None, engine=3):
    """`frac` is achieved / the peak of the pipe that does the work, <= 1 by construction: the fp32-equivalent rate of
    the bf16 matrix pipe for the bf16x3-split engine (engine 3), the fp32 MFMA rate otherwise.  The north star's 40 %
    target reads against the fp32-MFMA figure: `frac_vs_fp32_mfma_peak` (it can pass 1 for engine 3)."""
    ach = flop / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    peak = PEAK_BF16X3_EQUIV_TFLOPS if engine == 3 else PEAK_F32_MFMA_TFLOPS
    r = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
         "peak_is": ("fp32-equivalent rate of the bf16 matrix pipe: 2500 TFLOP/s dense bf16 / 6 bf16 products per fp32 product (bf16x3 split)"
                     if engine == 3 else "dense fp32 MFMA"),
         "frac_vs_fp32_mfma_peak": ach / PEAK_F32_MFMA_TFLOPS, "avg_launch_ms": ms}
    if kernel:
        r["kernel"] = kernel
        im = pmc_issue_model(kernel)
        if im:  # the binding resource of the screen: instruction issue of one wave per SIMD
            im["issue_bound_ms"] = im["frac_of_kernel"] * ms
            if "<8,8," in kernel and im.get("mfma_per_launch"):
                # two waves per SIMD (sub_dim 8): the VALU port model of profiles/ubench/valu_waves.hip -- an MFMA costs the
                # port 2.85 issue slots of 4 cycles, two waves lose 10 % to arbitration against four (P1, P2 at W = 2 / W = 4)
                valu = im["instructions_per_launch"] - im["mfma_per_launch"]
                slots = valu + 2.85 * im["mfma_per_launch"]
                im["valu_port_model"] = {"slots_per_launch": slots, "mfma_issue_slots": 2.85, "two_wave_arbitration": 1.10,
                                         "frac_of_kernel": slots / 1024.0 * 4.0 * 1.10 / im["kernel_cycles"],
                                         "source": "profiles/r6/ubench_valu_waves.txt (P1-P3)"}
            r["issue_bound"] = im
    if extra:
        r.update(extra)
    return r


def hbm_roofline(nbytes, ms, extra=None):
    ach = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    r = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS,
         "avg_launch_ms": ms, "algorithmic_bytes": nbytes}
    if extra:
        r.update(extra)
    return r


PEAK_VALU_TOPS = 78.6  # the VALU roofline for Manhattan (no contraction form), sub + abs + add = 3 ops per term


def valu_roofline(ops, ms, extra=None):
    ach = ops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    r = {"bound": "valu", "achieved": ach, "peak": PEAK_VALU_TOPS, "unit": "Tops/s", "frac": ach / PEAK_VALU_TOPS,
         "peak_is": "SURVEY.md 8(d): 157.3 TFLOP/s of fp32 VALU work counts an FMA as two: 78.6 T f32 ops/s; a Manhattan term executes "
                    "as 2 ops (sub, add with |.| as operand modifier): ops = 2*N*k*D",
         "avg_launch_ms": ms, "ops_per_launch": ops}
    if extra:
        r.update(extra)
    return r


def eval_shape(_lib, engine):
    """The reference's own evaluation shape through the HOST API, wall clock: what `make eval ALG=pq` prints upstream
    (src/bin/eval_pq.rs:42-70 with src/bin/common.rs:9-15: 1M x 384 Uniform[0,1) rows, m = 16, k = 256, 10 iterations,
    Euclidean, seed 66) -- ProductQuantizer(X_host, ...) with the rows in host memory, then every row quantized to f16
    in host memory.  Beside it the CPU port (oracle) on a stated subsample, training threaded like the reference (rayon
    over rows in the assignment), encode on one thread like eval_pq.rs."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O  # cpu leg of this block only
    from vq_amd import Distance, ProductQuantizer

    n, dim, m, k, iters, seed = 1_000_000, 384, 16, 256, 10, 66
    X = _lib.synth_uniform_host(n, dim, seed, 0)
    # (devices=[0]: this block is the single-GPU figure; the constructor's default is every visible device)
    ProductQuantizer(X[:20000], m, k, 2, Distance.euclidean(), seed, engine=engine, devices=[0])  # code objects, pinned pools
    t0 = time.perf_counter()
    pq = ProductQuantizer(X, m, k, iters, Distance.euclidean(), seed, engine=engine, devices=[0])
    train_ms = (time.perf_counter() - t0) * 1e3
    pq.quantize_batch(X[:50000])
    # the default call returns a fresh array (pyvq/src/pq.rs:96-107).  The process's FIRST result of this size has no pages
    # yet (faulted in under the copies); later results come out of recycled buffers
    # (vq_amd/_arena.py).  Both are reported; `quantize_batch_ms` is the repeated call, its median of three.
    t0 = time.perf_counter()
    q = pq.quantize_batch(X)
    quant_first_ms = (time.perf_counter() - t0) * 1e3
    del q
    qs = []
    for _ in range(3):
        t0 = time.perf_counter()
        q = pq.quantize_batch(X)
        qs.append((time.perf_counter() - t0) * 1e3)
        del q
    quant_ms = sorted(qs)[1]
    q = pq.quantize_batch(X)
    t0 = time.perf_counter()
    pq.quantize_batch(X, out=q)
    quant_reuse_ms = (time.perf_counter() - t0) * 1e3
    sub = slice(0, 100_000)
    mse = float(np.mean((q[sub].astype(np.float32) - X[sub]) ** 2))
    t0 = time.perf_counter()
    codes = pq.encode(X)
    codes_ms = (time.perf_counter() - t0) * 1e3
    del q, codes
    # the device part alone, for the PCIe-inclusive bound: rows already resident
    ds = _lib.Dataset.from_host(X)
    from vq_amd.pq import fit_codebooks
    _lib.synchronize()
    t0 = time.perf_counter()
    fit_codebooks(ds, m, k, iters, seed, engine=engine)
    fit_ms = (time.perf_counter() - t0) * 1e3
    ds.close()
    pcie_gbs = 53.0  # measured host -> device rate of this pool's boxes
    bound_ms = n * dim * 4 / (pcie_gbs * 1e9) * 1e3 + fit_ms
    # CPU port on a subsample (bounded: ~10-20 s)
    orc = O.get()
    ns = 50_000
    Xs = X[:ns]
    rng = np.random.default_rng(seed)
    init = np.stack([rng.choice(ns, k, replace=False) for _ in range(m)]).astype(np.uint64)
    reseed = rng.integers(0, ns, (m, 64)).astype(np.uint64)
    nt = orc.max_threads()
    t0 = time.perf_counter()
    cb_cpu, _ = orc.pq_fit(Xs, m, k, iters, init, reseed, threads=nt)
    cpu_train_s = time.perf_counter() - t0
    ne = 20_000
    t0 = time.perf_counter()
    orc.pq_encode(O.EUCLIDEAN, X[:ne], cb_cpu, want_f16=True, threads=1)
    cpu_enc_s = time.perf_counter() - t0
    del X
    return {
        "workload": "src/bin/eval_pq.rs + common.rs:9-15: PQ m=16 k=256 Euclidean, 10 iterations, seed 66, 1M x 384 Uniform[0,1) rows in HOST memory "
                    "(the package's own SplitMix64 draws: other codebooks than the crate's seed 66, same work)",
        "rows": n, "dim": dim, "m": m, "k": k, "iters": iters,
        "train_ms": train_ms, "train_iters_done": [int(x) for x in np.asarray(pq.fit_stats.get("iters", []))][:4],
        "train_device_fit_ms": fit_ms, "train_bound_ms": bound_ms, "train_over_bound": train_ms / bound_ms,
        "quantize_batch_ms": quant_ms, "quantize_vectors_per_s": n / (quant_ms * 1e-3),
        "quantize_batch_ms_all": qs, "quantize_batch_first_call_ms": quant_first_ms,
        "quantize_batch_out_reused_ms": quant_reuse_ms, "quantize_out_reused_vectors_per_s": n / (quant_reuse_ms * 1e-3),
        "quantize_bound_ms": n * dim * 4 / 55e9 * 1e3,
        "quantize_host_bytes_per_vector": dim * 4 + dim * 2, "quantize_pcie_gbs": n * (dim * 6) / (quant_ms * 1e-3) / 1e9,
        "encode_codes_ms": codes_ms, "encode_codes_vectors_per_s": n / (codes_ms * 1e-3),
        "reconstruction_mse_first_100k_rows": mse,
        "note": "wall clock around the host API calls, rows in pageable host memory; train_bound_ms = rows over PCIe at 53 GB/s + the fit "
                "alone on resident rows",
        "cpu_port": {"kind": "port", "train_rows": ns, "train_s": cpu_train_s, "train_threads": nt,
                     "train_s_extrapolated_to_1M_rows": cpu_train_s * n / ns,
                     "encode_rows": ne, "encode_s": cpu_enc_s, "encode_threads": 1,
                     "encode_s_extrapolated_to_1M_rows": cpu_enc_s * n / ne,
                     "note": "oracle restatement on the first rows of the same matrix; training assigns over all host threads like rayon "
                             "(src/core/vector.rs:417-423), encode is one vector at a time on one thread like eval_pq.rs:54-57; linear in rows"},
    }


def exact_update_case(_lib, engine):
    """C2 k-means with `exact_update`: the only mode whose CENTROIDS are the reference's bits (sums in the reference's row
    order, src/core/vector.rs:368-384; single GPU) -- assignment on the screen as everywhere, update by bucket + sequential
    chains instead of the fused accumulators."""
    import numpy as np

    n, d, m, k = 1_000_000, 128, 8, 256
    ds = _lib.Dataset.synthetic(n, d, DATA_SEED, 0)
    km = _lib.KMeans(ds, m, k)
    km.set_engine(engine)
    km.set_exact_update(True)
    init = strided_init(n, m, k).astype(np.uint64)
    iters = 5

    def restart():
        km.init_from_rows(init)
        km.set_active(np.ones(m, np.uint8))

    restart()
    km.run(2)
    restart()
    _lib.synchronize()
    t0 = time.perf_counter()
    it, _, _, paused = km.run(iters)
    _lib.synchronize()
    dt = time.perf_counter() - t0
    it = np.asarray(it, np.int64)
    done = max(1, int(it.max()))
    ms = dt * 1e3 / done
    km.close()
    ds.close()
    flop = 2.0 * k * d * n
    return {"workload": "C2's shape, vqhip_kmeans_set_exact_update(1): centroids bit-identical to the reference's sequential sums",
            "rows": n, "dim": d, "m": m, "k": k, "kmeans_ms_per_iter": ms, "kmeans_iter_per_s": 1e3 / ms,
            "kmeans_iters_timed": [int(it.min()), int(it.max())], "kmeans_paused": bool(paused),
            "kmeans_roofline": mfma_roofline(flop * float(it.sum()) / done / m, ms, engine=3, extra={
                "note": "whole iteration, host-driven loop (one synchronisation per iteration); against the screen's pipe -- the "
                        "update's sequential f32 chains (n/k = 3900 dependent adds per cluster and column) are what it adds"}),
            "update_hbm_roofline": hbm_roofline(4.0 * n * d * 2, ms, {"note": "rows read once by the screen and once by the ordered sums"})}


def decode_case(_lib, torch):
    """Quantizer::dequantize for a batch, device-resident (src/pq.rs:201-209): codes -> f32 centroids (vqhip_pq_decode_device:
    4*D + m bytes per vector) and f16 -> f32 (vqhip_dequantize_f16_device: 6*D bytes per vector); HBM-bound."""
    import numpy as np

    n, d, m, k = 1_000_000, 128, 8, 256
    rng = np.random.default_rng(DATA_SEED)
    cb = rng.standard_normal((m, k, d // m)).astype(np.float32)
    enc = _lib.PQEncoder(cb, _lib.SQUARED_EUCLIDEAN)
    g = torch.Generator(device="cuda").manual_seed(DATA_SEED)
    codes = torch.randint(0, k, (n, m), device="cuda", generator=g, dtype=torch.uint8)
    f16 = torch.randn((n, d), device="cuda", generator=g).to(torch.float16).contiguous()
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def timed(fn, reps=20):
        for _ in range(60):  # (clocks up: the first ~10 ms after host work run slow)
            fn()
        _lib.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        _lib.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    dec_ms = timed(lambda: enc.decode_device(codes.data_ptr(), n, out.data_ptr()))
    ok_dec = bool(torch.equal(out[:4096], torch.from_numpy(np.concatenate(
        [cb[s][codes[:4096, s].cpu().numpy()] for s in range(m)], axis=1)).cuda()))
    deq_ms = timed(lambda: _lib.dequantize_f16_device(f16.data_ptr(), n * d, out.data_ptr()))
    ok_deq = bool(torch.equal(out, f16.to(torch.float32)))
    enc.close()
    return {"workload": "1M x 128, m=8 k=256, device-resident: codes -> f32 rows, f16 rows -> f32 rows", "rows": n, "dim": d, "m": m,
            "decode_ms": dec_ms, "decode_vectors_per_s": n / (dec_ms * 1e-3), "decode_checked": ok_dec,
            "decode_roofline": hbm_roofline((4.0 * d + m) * n, dec_ms, {"kernel": "k_decode_f32_lds<8>", "note": "4*D bytes out + m code bytes in per vector (the codebooks, 128 KB, in LDS)"}),
            "dequantize_ms": deq_ms, "dequantize_vectors_per_s": n / (deq_ms * 1e-3), "dequantize_checked": ok_deq,
            "dequantize_roofline": hbm_roofline(6.0 * d * n, deq_ms, {"kernel": "k_dequant_f16", "note": "2*D bytes in + 4*D bytes out per vector"})}


def adc_case(_lib, torch, engine):
    """Asymmetric-distance search over stored codes: 64 queries against 1M x 8 device-resident codes, top 10.
    Per call: the tables, a sampled threshold per query, ONE scan of the codes per batch of 8 queries that keeps the rows at
    or below it, the exact top-k of those (k_adc.hip, round 6), results to the host."""
    import numpy as np

    n, d, m, k, nq, topk = 1_000_000, 128, 8, 256, 64, 10
    ds = _lib.Dataset.synthetic(n, d, DATA_SEED, 0)
    km = _lib.KMeans(ds, m, k)
    km.set_engine(engine)
    km.init_from_rows(strided_init(n, m, k).astype(np.uint64))
    km.run(TRAIN_ITERS)
    cb = km.get_centroids()
    km.close()
    enc = _lib.PQEncoder(cb, _lib.SQUARED_EUCLIDEAN)
    enc.set_engine(engine)
    codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
    enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
    _lib.synchronize()
    Q = _lib.synth_uniform_host(nq, d, DATA_SEED + 1, 0)
    res = {}
    for q in (nq, 8):
        for _ in range(30):
            enc.adc_search((codes.data_ptr(), n), Q[:q], topk)
        reps = 20
        t0 = time.perf_counter()
        for _ in range(reps):
            idx, dist = enc.adc_search((codes.data_ptr(), n), Q[:q], topk)
        res[q] = (time.perf_counter() - t0) * 1e3 / reps
    full_pass_queries = enc.adc_last_redone()
    passes = (nq + 7) // 8
    scan_bytes = float(n) * m * passes + 4.0 * nq * m * k
    # self-check: a query that IS the reconstruction of a stored row has ADC distance 0 to that row (ties by row index may
    # name an earlier row with the same codes); recall against exact search is the eval CLI's job (vq_amd/evalcli.py)
    c8 = codes[:8].cpu().numpy()
    recon = np.concatenate([cb[s_][c8[:, s_]] for s_ in range(m)], axis=1)
    i2, d2 = enc.adc_search((codes.data_ptr(), n), recon, 1)
    top1_is_own_code = bool((d2[:, 0] == 0.0).all() and (i2[:, 0] <= np.arange(8)).all())
    enc.close()
    ds.close()
    return {"workload": f"ADC top-{topk} of {nq} queries over {n} x {m} one-byte codes (device-resident), squared L2", "rows": n, "m": m, "k": k,
            "queries": nq, "topk": topk, "ms_per_call": res[nq], "queries_per_s": nq / (res[nq] * 1e-3),
            "ms_per_call_8_queries": res[8], "code_scans_per_call": passes, "queries_repeated_by_the_full_pass": full_pass_queries,
            "roofline": hbm_roofline(scan_bytes, res[nq], {"kernel": "k_adc_scan_thr", "note": "whole call, wall clock (tables + sample + "
                                     f"{passes} scans of the n*m code bytes + top-k + read-back): algorithmic bytes = n*m per batch of 8 queries + the tables"}),
            # what actually bounds the scan: one 4-byte LDS table read per (row, query, subspace) -- 128 B per clock and CU
            "lds_roofline": {"bound": "lds", "achieved": float(n) * nq * m / (res[nq] * 1e-3) / 1e12, "peak": 256 * 32 * 2.1e9 / 1e12,
                             "unit": "T table reads/s", "frac": float(n) * nq * m / (res[nq] * 1e-3) / (256 * 32 * 2.1e9),
                             "note": "whole call; peak = 256 CUs x 32 conflict-free 4-byte LDS reads per clock at 2.1 GHz (a row's eight terms of eight queries are two 16-byte reads at a random 32-byte slot per subspace: bank conflicts)"},
            "self_check": top1_is_own_code}


def other_configs(_lib, torch, engine):
    """BASELINE configs C1, C3, C4 on one GPU (rank 0, N=1): device-resident synthetic rows, codebooks from a few
    untimed Lloyd iterations, every entry with the roofline SURVEY.md 8(d) assigns it (HIP-event time of the
    assignment kernels from the library's profiling hooks; stream-synchronised wall time for whole iterations / builds)."""
    import numpy as np

    from vq_amd import TSVQ, Distance
    from vq_amd.tsvq import build_tree

    out = {}

    def pq_case(name, n, d, m, k, metric, label):
        ds = _lib.Dataset.synthetic(n, d, DATA_SEED, 0)
        km = _lib.KMeans(ds, m, k)
        km.set_engine(engine)
        init = strided_init(n, m, k).astype(np.uint64)
        km.init_from_rows(init)
        km.run(TRAIN_ITERS)
        cb = km.get_centroids()
        iters = 10

        def restart():  # every timed run is the first `iters` iterations of a fit: all m subspaces execute all of them
            km.init_from_rows(init)
            km.set_active(np.ones(m, np.uint8))

        for _ in range(2):
            restart()
            km.run(iters)
        restart()
        _lib.synchronize()
        t0 = time.perf_counter()
        it, _, _, paused = km.run(iters)
        _lib.synchronize()
        km_dt = time.perf_counter() - t0
        it = np.asarray(it, np.int64)
        km_iters = max(1, int(it.max()))
        km_ms = km_dt * 1e3 / km_iters
        km_active = float(it.sum()) / km_iters  # subspaces that executed, averaged over the timed iterations
        km_valid = bool(not paused and int(it.min()) == int(it.max()) == iters)
        km_engine = _lib.last_assign_stats()[1]
        km.close()
        enc = _lib.PQEncoder(cb, metric)
        enc.set_engine(engine)
        codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
        tw = time.perf_counter()  # ~60 ms of untimed passes: the clocks are down after the host work in front (see measure())
        while time.perf_counter() - tw < 0.06:
            for _ in range(5):
                enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
            _lib.synchronize()
        reps = 10 if n >= 100_000 else 200
        t0 = time.perf_counter()
        for _ in range(reps):
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
        _lib.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / reps
        # the kernel's own time from a second, instrumented loop (three HIP events per call are a third of a C1-sized step)
        _lib.set_profiling(True)
        for _ in range(reps):
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
        _lib.synchronize()
        calls, primary_ms, recheck_ms = _lib.profile_collect()
        _lib.set_profiling(False)
        rechecked, used = _lib.last_assign_stats()
        flop = 2.0 * k * d * n
        out[name] = {
            "workload": label, "rows": n, "dim": d, "m": m, "k": k, "sub_dim": d // m,
            "encode_vectors_per_s": n / (step_ms * 1e-3), "encode_ms_per_step": step_ms,
            "encode_engine": {1: "exact", 2: "fp32_mfma_screen", 3: "bf16x3_mfma_screen"}.get(used, str(used)),
            "recheck_fraction": rechecked / float(n * m),
            "encode_roofline": mfma_roofline(flop, primary_ms / max(calls, 1), kernel=screen_kernel_name(d // m, k, False), engine=used, extra={
                "step_frac": flop / (step_ms * 1e-3) / 1e12 / (PEAK_BF16X3_EQUIV_TFLOPS if used == 3 else PEAK_F32_MFMA_TFLOPS),
                "recheck_avg_launch_ms": recheck_ms / max(calls, 1), "flop_per_launch": flop}),
            "kmeans_ms_per_iter": km_ms, "kmeans_iter_per_s": 1e3 / km_ms,
            "kmeans_iters_timed": [int(it.min()), int(it.max())], "kmeans_active_subspaces": km_active,
            "kmeans_paused": bool(paused), "kmeans_valid": km_valid,
            "kmeans_roofline": mfma_roofline(flop * km_active / m, km_ms, kernel=screen_kernel_name(d // m, k, True), engine=km_engine, extra={
                "flop_per_iter": flop * km_active / m,
                "note": "whole Lloyd iteration (assign + fused update + reduce + finalize), decisions on the device; flop scaled by "
                        "the subspaces that executed"}),
        }
        enc.close()
        ds.close()

    def encode_case(name, n, d, m, k, metric, label):
        """encode only, at C2's shape under another Distance (src/core/distance.rs:57-58, 85-95): the same trained codebooks
        for both; Manhattan has no contraction form and runs on the exact VALU engine (k_assign_exact)"""
        ds = _lib.Dataset.synthetic(n, d, DATA_SEED, 0)
        km = _lib.KMeans(ds, m, k)
        km.set_engine(engine)
        km.init_from_rows(strided_init(n, m, k).astype(np.uint64))
        km.run(TRAIN_ITERS)
        cb = km.get_centroids()
        km.close()
        enc = _lib.PQEncoder(cb, metric)
        enc.set_engine(engine)
        codes = torch.empty((n, m), dtype=torch.uint8, device="cuda")
        tw = time.perf_counter()
        while time.perf_counter() - tw < 0.06:
            for _ in range(3):
                enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
            _lib.synchronize()
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
        _lib.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / reps
        _lib.set_profiling(True)
        for _ in range(reps):
            enc.encode_device(ds.device_ptr, n, codes.data_ptr(), None)
        _lib.synchronize()
        calls, primary_ms, recheck_ms = _lib.profile_collect()
        _lib.set_profiling(False)
        rechecked, used = _lib.last_assign_stats()
        kern_ms = primary_ms / max(calls, 1)
        if used == 1:  # exact VALU engine: 3 ops per (row, centroid, dimension)
            # SURVEY.md 8(d) counts a term as sub + abs + add = 3 ops against 78.6 Tops/s; |x| is an operand modifier on this
            # ISA (v_add_f32 acc, acc, |diff|), so a term is TWO instructions and the 3-op count passes the peak (1.09):
            # `frac` counts the two that execute, the 3-op figure is kept beside it
            ops = 2.0 * n * k * d
            roof = valu_roofline(ops, kern_ms, {
                "kernel": "k_assign_exact", "step_frac": ops / (step_ms * 1e-3) / 1e12 / PEAK_VALU_TOPS,
                "frac_counting_3_ops_per_term": 1.5 * ops / (kern_ms * 1e-3) / 1e12 / PEAK_VALU_TOPS,
                "note": "the kernel keeps the reference's sequential f32 sum per (row, centroid): one lane per (row, subspace)"})
        else:
            flop = 2.0 * k * d * n
            roof = mfma_roofline(flop, kern_ms, engine=used, extra={
                "step_frac": flop / (step_ms * 1e-3) / 1e12 / (PEAK_BF16X3_EQUIV_TFLOPS if used == 3 else PEAK_F32_MFMA_TFLOPS),
                "recheck_avg_launch_ms": recheck_ms / max(calls, 1), "flop_per_launch": flop})
        out[name] = {
            "workload": label, "rows": n, "dim": d, "m": m, "k": k, "sub_dim": d // m,
            "encode_vectors_per_s": n / (step_ms * 1e-3), "encode_ms_per_step": step_ms,
            "encode_engine": {1: "exact (VALU)", 2: "fp32_mfma_screen", 3: "bf16x3_mfma_screen"}.get(used, str(used)),
            "recheck_fraction": rechecked / float(n * m), "encode_roofline": roof,
        }
        enc.close()
        ds.close()

    pq_case("C1", 10_000, 64, 4, 16, _lib.EUCLIDEAN, "BASELINE.json configs[0]: PQ m=4 k=16 Euclidean, 10k x 64 (launch-latency bound on a GPU)")
    encode_case("C2_euclidean", 1_000_000, 128, 8, 256, _lib.EUCLIDEAN, "C2's shape under Distance::Euclidean (the pyvq default; sqrt collapses near-ties onto the earlier index)")
    encode_case("C2_manhattan", 1_000_000, 128, 8, 256, _lib.MANHATTAN, "C2's shape under Distance::Manhattan (no contraction form: exact VALU engine)")
    pq_case("C3", 1_000_000, 768, 96, 256, _lib.COSINE, "BASELINE.json configs[2]: PQ m=96 k=256 cosine, 1M x 768 (training is squared L2, src/core/vector.rs:352-363)")
    # one GPU's share of BASELINE configs[4] (100M x 128, m = 16 over 8 GPUs): the per-rank work of every point of the 8-GPU
    # curve; the exchange it adds per iteration is one 295 KB slab (python bench.py --gpus N reports `weak_C5` with it)
    pq_case("C5_shard", 12_500_000, 128, 16, 256, _lib.SQUARED_EUCLIDEAN,
            "BASELINE.json configs[4], ONE GPU's shard: PQ m=16 k=256 L2 on 12.5M x 128 (sub_dim 8), no collective in this block")
    out["C2_exact_update"] = exact_update_case(_lib, engine)
    out["decode"] = decode_case(_lib, torch)
    out["adc"] = adc_case(_lib, torch, engine)

    out["eval_shape"] = eval_shape(_lib, engine)

    # C4: TSVQ depth 8 on 1M x 128
    n, d, depth = 1_000_000, 128, 8
    ds = _lib.Dataset.synthetic(n, d, DATA_SEED, 0)
    build_tree(ds, depth)
    ts = []
    for _ in range(5):
        _lib.synchronize()
        t0 = time.perf_counter()
        cent, left, right = build_tree(ds, depth)
        _lib.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    build_ms = sorted(ts)[len(ts) // 2]
    # the hard case for the build's exact column sums: zero-mean rows (real embeddings are)
    g = torch.Generator(device="cuda").manual_seed(DATA_SEED)
    Xz = torch.randn((n, d), device="cuda", generator=g).contiguous()
    torch.cuda.synchronize()
    dsz = _lib.Dataset.from_device(Xz.data_ptr(), n, d)
    build_tree(dsz, depth)
    tz = []
    for _ in range(3):
        _lib.synchronize()
        t0 = time.perf_counter()
        build_tree(dsz, depth)
        _lib.synchronize()
        tz.append((time.perf_counter() - t0) * 1e3)
    build_ms_zero_mean = sorted(tz)[len(tz) // 2]
    dsz.close()
    del Xz
    split_levels = depth
    build_bytes = 4.0 * n * d * (2 * split_levels + 1)  # mean + variance pass per split level, one leaf-mean pass
    t = TSVQ.from_tree(cent, left, right, Distance.euclidean())
    leaf = torch.empty(n, dtype=torch.int32, device="cuda")
    f16 = torch.empty((n, d), dtype=torch.float16, device="cuda")
    import ctypes as C

    lib = _lib.load()

    def enc_once():
        _lib.check(lib.vqhip_tsvq_encode_device(t._enc.raw, C.c_void_p(ds.device_ptr), n, C.c_void_p(leaf.data_ptr()),
                                                C.c_void_p(f16.data_ptr())))

    for _ in range(PREWARM_STEPS):  # clocks up after the host work between the builds and here (see measure())
        enc_once()
    _lib.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        enc_once()
    _lib.synchronize()
    enc_ms = (time.perf_counter() - t0) * 1e3 / 20
    out["C4"] = {
        "workload": "BASELINE.json configs[3]: TSVQ depth 8 on 1M x 128, tree bit-identical to the reference's recursion",
        "rows": n, "dim": d, "depth": depth, "nodes": int(len(left)),
        "build_ms": build_ms, "build_ms_all": ts,
        "build_roofline": hbm_roofline(build_bytes, build_ms, dict(
            {"note": "4*N*D bytes x (2 passes x 8 split levels + 1 leaf-mean pass)"}, **tsvq_traffic_fields("c4", build_bytes))),
        "build_ms_zero_mean": build_ms_zero_mean, "build_ms_zero_mean_all": tz,
        "build_roofline_zero_mean": hbm_roofline(build_bytes, build_ms_zero_mean, dict(
            {"note": "same shape on N(0,1) rows"}, **tsvq_traffic_fields("normal", build_bytes))),
        "encode_vectors_per_s": n / (enc_ms * 1e-3), "encode_ms_per_step": enc_ms,
        "encode_roofline": hbm_roofline((4.0 * d + 2.0 * d) * n, enc_ms, {"note": "4*D bytes in + 2*D bytes (f16 reconstruction) out per vector"}),
    }
    ds.close()
    return out


def free_port() -> int:
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return int(sk.getsockname()[1])


def launch_ranks(n_ranks: int, argv, worker=None, grace_s: float = 20.0) -> int:
    """`python bench.py --gpus N` without a launcher: start N FRESH rank processes, one per GPU (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their environment, the same command line), relay rank 0's one JSON line
    to stdout and return non-zero if any rank failed.  This process never imports torch or loads libvqhip, so it
    never initialises a GPU, and it never exec()s: the ranks are children (the pool forbids exec from a process that
    has touched the GPU, and a parent that held a HIP context would share its devices with the ranks)."""
    import subprocess
    import threading

    worker = worker or [sys.executable, os.path.abspath(__file__)]
    port = free_port()
    procs, lines = [], []
    for r in range(n_ranks):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n_ranks), "LOCAL_WORLD_SIZE": str(n_ranks),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "VQ_BENCH_LAUNCHER": str(os.getpid())})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this driver
        procs.append(subprocess.Popen(list(worker) + list(argv), env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr,
                                      stderr=sys.stderr))

    def pump():
        for raw in procs[0].stdout:
            lines.append(raw.decode("utf-8", "replace").rstrip("\n"))

    t = threading.Thread(target=pump, daemon=True)
    t.start()
    failed_at, rc = None, 0
    while any(p.poll() is None for p in procs):
        time.sleep(0.1)
        bad = [p.returncode for p in procs if p.poll() is not None and p.returncode != 0]
        if bad and failed_at is None:
            failed_at, rc = time.monotonic(), bad[0]
        if failed_at is not None and time.monotonic() - failed_at > grace_s:
            for p in procs:  # a rank died: its peers may wait in a collective for ever -- stop exactly the PIDs we started
                if p.poll() is None:
                    p.terminate()
            time.sleep(2.0)
            for p in procs:
                if p.poll() is None:
                    p.kill()
    t.join(timeout=5.0)
    for p in procs:
        if p.returncode != 0 and rc == 0:
            rc = p.returncode
    js = [ln for ln in lines if ln.startswith("{")]
    if rc == 0 and not js:
        print("bench.py: rank 0 printed no JSON line", file=sys.stderr)
        rc = 3
    if js:
        print(js[-1], flush=True)
    return rc


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="C2", help="workload (default: the metric's, C2)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: the workload's rows PER GPU (default); strong: the workload's rows in all, sharded over the GPUs")
    ap.add_argument("--rows", type=int, default=0, help="rows per GPU (weak) / in all (strong); default: the workload's")
    ap.add_argument("--kmeans-iters", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the C1 / C3 / C4 block (N=1) and the strong-scaling / C5 blocks (N>1)")
    ap.add_argument("--collective", choices=["native", "torch", "gloo"], default="native",
                    help="multi-GPU all-reduce: below the C ABI (vqhip_kmeans_run_sharded, RCCL), through torch.distributed "
                         "nccl (= RCCL), or through gloo with the slab staged on the host (ranks may then share a GPU: tests)")
    ap.add_argument("--engine", choices=["auto", "exact", "mfma", "bf16"], default="auto")
    ap.add_argument("--one-process", action="store_true",
                    help="second launcher mode: ONE process drives the --gpus devices through the library's worker threads "
                         "(vqhip_mdataset / vqhip_mkmeans / vqhip_mpq_encoder: what ProductQuantizer(..., devices=) uses)")
    ap.add_argument("--device-list", default="", help="--one-process: comma-separated device ids (default 0..gpus-1; a device may repeat)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write the last step's codes (float32; a fixed seeded row sample if they pass "
                         "60 MB) and the codebooks as DIR/*.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.one_process:
        sys.exit(one_process(args))
    if "WORLD_SIZE" not in os.environ and "RANK" not in os.environ and (args.gpus > 1 or os.environ.get("VQ_BENCH_SPAWN") == "1"):
        # no launcher around us: be the launcher (before torch / libvqhip are imported: this process stays off the GPU)
        sys.exit(launch_ranks(args.gpus, argv))
    sys.exit(worker(args))


def one_process(args) -> int:
    """`python bench.py --gpus N --one-process`: the same job -- rows sharded over N devices, TRAIN_ITERS + timed Lloyd
    iterations with one slab all-reduce each, K timed encode passes over the resident rows -- driven by ONE process through
    the library's own ranks (worker threads; the in-process fixed-order exchange, or RCCL with VQHIP_MULTI_COMM=rccl).
    Same line shape as the multi-process launcher; `launcher` says which one ran."""
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import numpy as np

    from vq_amd import _lib

    _lib.load()
    devices = [int(x) for x in args.device_list.split(",")] if args.device_list else list(range(args.gpus))
    if len(devices) != args.gpus:
        print(f"bench.py: --device-list names {len(devices)} devices, --gpus {args.gpus}", file=sys.stderr)
        return 2
    if _lib.device_count() < 1:
        print("bench.py needs a MI355X (no GPU visible); there is no CPU fallback", file=sys.stderr)
        return 2
    _lib.set_device(devices[0])
    engine = {"auto": _lib.ENGINE_AUTO, "exact": _lib.ENGINE_EXACT, "mfma": _lib.ENGINE_MFMA, "bf16": _lib.ENGINE_MFMA_BF16}[args.engine]
    wl = WORKLOADS[args.config]
    dim, m_, k_ = wl["dim"], wl["m"], wl["k"]
    rows = args.rows if args.rows else wl["rows"]
    world = len(devices)
    n_global = rows * world if args.scaling == "weak" else rows
    mds = _lib.MDataset.synthetic(n_global, dim, DATA_SEED, devices)
    init = strided_init(n_global, m_, k_).astype(np.uint64)
    km = _lib.MKMeans(mds, m_, k_)
    km.set_engine(engine)
    km.init_from_rows(init)
    km.run(TRAIN_ITERS)
    codebooks = km.get_centroids()
    for _ in range(25 if n_global * dim <= 4e8 * world else 6):  # untimed: clocks up (see measure())
        km.run(10)

    def restart():
        km.init_from_rows(init)
        km.set_active(np.ones(m_, np.uint8))

    restart()
    km.run(args.kmeans_iters)
    restart()
    t0 = time.perf_counter()
    it, counts, _, paused = km.run(args.kmeans_iters)  # (returns with every rank's stream drained)
    km_dt = time.perf_counter() - t0
    it = np.asarray(it, np.int64)
    km_iters = max(1, int(it.max()))
    active_avg = float(it.sum()) / km_iters
    km_ms = km_dt / km_iters * 1e3
    comm_world, comm_kind = km.info()
    km.close()
    flop_row = 2.0 * k_ * dim
    enc = _lib.MPQEncoder(codebooks, _lib.SQUARED_EUCLIDEAN, devices)
    enc.set_engine(engine)
    enc.encode_dataset(mds, repeat=PREWARM_STEPS + args.warmup)
    t0 = time.perf_counter()
    codes = enc.encode_dataset(mds, repeat=args.steps, want_codes=False)
    dt = time.perf_counter() - t0
    last = enc.encode_dataset(mds, repeat=1, want_codes=True)  # the timed pass once more, its codes back
    checksum = int(last[: mds.rows_per_device()[0]].astype(np.int64).sum())
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, 0, last, codebooks, 1)
    del last
    rechecked, used_engine = 0, 3
    step_ms = dt / args.steps * 1e3
    rows_rank0 = int(mds.rows_per_device()[0])
    line = {
        "metric": "pq_encode_vectors_per_s", "value": n_global * args.steps / dt, "unit": "vectors/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "prewarm_steps": PREWARM_STEPS, "ms_per_step": step_ms,
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32 (bf16x3-split MFMA screen, exact f32 re-check)", "data": "synthetic",
        "launcher": "one process: the library's worker thread per device (vqhip_mdataset / vqhip_mkmeans / vqhip_mpq_encoder)",
        "devices": devices,
        "config": {
            "workload": f"PQ m={m_} k={k_} L2 encode on {n_global}x{dim} f32 rows in all, {rows_rank0} on the first device, device-resident "
                        f"({wl['label']}; {args.scaling} scaling); codes out (1 byte per subspace)",
            "rows_per_gpu": rows_rank0, "rows_global": n_global, "dim": dim, "m": m_, "k": k_, "sub_dim": dim // m_,
            "codebooks": f"{TRAIN_ITERS} Lloyd iterations from strided init rows",
            "kmeans_iter_per_s": km_iters / km_dt, "kmeans_ms_per_iter": km_ms,
            "kmeans_valid": bool(not paused and int(it.min()) == int(it.max()) == args.kmeans_iters),
            "kmeans_roofline_frac": mfma_roofline(flop_row * rows_rank0 * active_avg / m_, km_ms, engine=3)["frac"],
            "prewarm_steps": PREWARM_STEPS,
        },
        "roofline": mfma_roofline(flop_row * rows_rank0, step_ms, engine=3, extra={
            "note": "whole step wall time (the passes of all devices run side by side; per-device work = rows_per_gpu)",
            "flop_per_launch": flop_row * rows_rank0, "algorithmic_bytes_per_launch": (4.0 * dim + m_) * rows_rank0, "traffic": None}),
        "kmeans_rows_global": n_global, "kmeans_iter_per_s": km_iters / km_dt, "kmeans_ms_per_iter": km_ms,
        "kmeans_collective": {0: "none (one rank)", 1: "rccl below the C ABI, ranks = threads of this process",
                              2: "in-process fixed-order exchange through peer access (vqhip_comm_create_local)"}[comm_kind],
        "comm_world": comm_world,
        "kmeans_counts_sum_per_subspace": [int(counts[0].sum()), int(counts[-1].sum())],
        "codebooks_abs_sum": float(np.abs(codebooks.astype(np.float64)).sum()),
        "codes_checksum_rank0": checksum,
    }
    del codes
    enc.close()
    mds.close()
    os.write(json_fd, (json.dumps(line) + "\n").encode())
    return 0


class Ranks:
    """control plane of the run: barrier, max over ranks, object broadcast.  A gloo group on the host (no second RCCL
    communicator next to the library's), or none for one rank."""

    def __init__(self, world, rank):
        self.world, self.rank, self.dist = world, rank, None
        if world > 1:
            import torch.distributed as dist

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29512")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            self.dist = dist

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def reduce(self, x: float, op="max") -> float:
        if not self.dist:
            return x
        import torch

        t = torch.tensor([x], dtype=torch.float64)
        self.dist.all_reduce(t, op={"max": self.dist.ReduceOp.MAX, "min": self.dist.ReduceOp.MIN, "sum": self.dist.ReduceOp.SUM}[op])
        return float(t.item())

    def bcast(self, obj):
        if not self.dist:
            return obj
        box = [obj]
        self.dist.broadcast_object_list(box, src=0)
        return box[0]

    def close(self):
        if self.dist:
            self.dist.destroy_process_group()


def measure(args, ranks, wl_name, scaling, *, torch, _lib, engine, ncomm, collective, steps, warmup, want_f16=True, group=None,
            snapshot=False):
    """One workload on this rank's shard: codebooks from TRAIN_ITERS global Lloyd iterations, then the timed k-means
    iterations (every timed run starts from the same initial centroids, so all m subspaces execute every iteration)
    and the timed encode passes.  Returns (dict for the line, codebooks, handles to keep); with `snapshot` the dict also
    holds "_dump": (the last timed step's codes on the host, this shard's first global row) for --dump-outputs."""
    import numpy as np

    from vq_amd.sharded import HipShard, ShardedKMeans, shard_rows

    wl = WORKLOADS[wl_name]
    world, rank = ranks.world, ranks.rank
    dim, m_, k_ = wl["dim"], wl["m"], wl["k"]
    rows = args.rows if (args.rows and wl_name == args.config) else wl["rows"]
    if scaling == "weak":
        n_global, n, offset = rows * world, rows, rank * rows
    else:
        n_global = rows
        offset, n = shard_rows(n_global, world, rank)
    ds = _lib.Dataset.synthetic(n, dim, DATA_SEED, offset)
    init = strided_init(n_global, m_, k_)
    sync = torch.cuda.synchronize
    out = {"rows_global": n_global, "rows_this_rank": n, "dim": dim, "m": m_, "k": k_, "scaling": scaling}
    iters_req = args.kmeans_iters

    if collective in ("native", "none"):
        km = _lib.KMeans(ds, m_, k_)
        km.set_engine(engine)
        km.init_from_global_rows(ncomm, init, offset)
        km.run(TRAIN_ITERS, ncomm)
        codebooks = km.get_centroids()
        # untimed: the first ~100 ms of work after an idle spell run up to 10 % slow (clocks ramping up); the same count on
        # every rank (each run carries its all-reduces)
        for _ in range(25 if n * dim <= 4e8 else 6):
            km.run(10, ncomm)

        def restart():
            km.init_from_global_rows(ncomm, init, offset)
            km.set_active(np.ones(m_, np.uint8))

        restart()
        km.run(iters_req, ncomm)
        restart()
        sync()
        ranks.barrier()
        t0 = time.perf_counter()
        it, counts, _, paused = km.run(iters_req, ncomm)
        sync()
        ranks.barrier()
        km_dt = time.perf_counter() - t0
        it = np.asarray(it, np.int64)
        # the collective alone: HIP events around vqhip_kmeans_allreduce on the library's stream (= torch's current one)
        ar_ms = None
        if ncomm is not None and (ncomm.info()[0] > 1 or os.environ.get("VQ_BENCH_FORCE_COMM") == "1"):
            km.accumulate()
            for _ in range(3):
                km.allreduce(ncomm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 20
            sync()
            ranks.barrier()
            e0.record()
            for _ in range(reps):
                km.allreduce(ncomm)
            e1.record()
            sync()
            ar_ms = ranks.reduce(e0.elapsed_time(e1) / reps, "max")
            km.finalize()
        km.close()
    else:  # the all-reduce through torch.distributed (nccl = RCCL; gloo stages the slab on the host)
        from vq_amd.sharded import Comm

        comm = Comm(force=True, group=group)
        shard = HipShard(ds, m_, k_, offset, engine)
        skm = ShardedKMeans(shard, n_global, comm)
        skm.init_from_global_rows(init)
        for _ in range(TRAIN_ITERS):
            skm.step()
        codebooks = shard.get_centroids()
        for _ in range(10):
            skm.step()
        skm.init_from_global_rows(init)
        sync()
        ranks.barrier()
        t0 = time.perf_counter()
        counts = None
        for _ in range(iters_req):
            counts, _ = skm.step()
        sync()
        ranks.barrier()
        km_dt = time.perf_counter() - t0
        it, paused, ar_ms = np.full(m_, iters_req, np.int64), False, None
        shard.close()
        _lib.set_stream(torch.cuda.current_stream().cuda_stream)
    km_dt = ranks.reduce(km_dt, "max")
    km_engine = _lib.last_assign_stats()[1]  # the engine of the training passes (3 = bf16x3-split MFMA screen)
    km_iters = max(1, int(it.max()))
    # a run that paused on an empty cluster or retired subspaces did less than m subspaces x iterations of work:
    # the per-iteration flop is scaled by the subspaces that really executed
    active_avg = float(it.sum()) / km_iters
    km_ms = km_dt / km_iters * 1e3
    flop_row = 2.0 * k_ * dim
    out.update({
        "kmeans_ms_per_iter": km_ms, "kmeans_iter_per_s": km_iters / km_dt,
        "kmeans_iters_requested": iters_req, "kmeans_iters_timed": [int(it.min()), int(it.max())],
        "kmeans_active_subspaces": active_avg, "kmeans_paused": bool(paused),
        "kmeans_valid": bool(not paused and int(it.min()) == int(it.max()) == iters_req),
        "kmeans_counts_sum_per_subspace": [int(counts[0].sum()), int(counts[-1].sum())] if counts is not None else None,
        "kmeans_allreduce_ms": ar_ms,
        "codebooks_abs_sum": float(np.abs(codebooks.astype(np.float64)).sum()),  # same on every rank; ~equal for any sharding
        "kmeans_roofline": mfma_roofline(flop_row * n * active_avg / m_, km_ms, engine=km_engine, extra={
            "flop_per_iter_per_gpu": flop_row * n * active_avg / m_,
            "note": "per GPU: 2*N*k*D flop of one Lloyd iteration (assign + fused update + all-reduce + finalize) x the fraction "
                    "of subspaces that executed / its wall time; X is read once per iteration (4*N*D bytes, SURVEY.md 8(d))"}),
    })

    # ---- encode: the timed region -------------------------------------------------------
    enc = _lib.PQEncoder(codebooks, _lib.SQUARED_EUCLIDEAN)
    enc.set_engine(engine)
    codes = torch.empty((n, m_), dtype=torch.uint8, device="cuda")
    xptr = ds.device_ptr
    # the host work between the k-means block and here leaves the GPU idle and its clocks down; the first ~30 passes after
    # that run up to 10 % slow (0.44, 0.44, 0.41, 0.39 ms per pass in groups of ten, 0.365 after ~300: tools/ab_screen.py).  PREWARM_STEPS
    # untimed passes bring the clocks back before the W warmup steps the contract asks for; reported in the line.
    # first W + SIDE_STEPS passes with NO prewarm (`cold_ms_per_step`: what a caller sees right after host-side work)
    for _ in range(warmup):
        enc.encode_device(xptr, n, codes.data_ptr(), None)
    sync()
    ranks.barrier()
    t0 = time.perf_counter()
    for _ in range(SIDE_STEPS):
        enc.encode_device(xptr, n, codes.data_ptr(), None)
    sync()
    ranks.barrier()
    cold_ms = ranks.reduce(time.perf_counter() - t0, "max") / SIDE_STEPS * 1e3
    for _ in range(PREWARM_STEPS):
        enc.encode_device(xptr, n, codes.data_ptr(), None)
    for _ in range(warmup):
        enc.encode_device(xptr, n, codes.data_ptr(), None)
    sync()
    ranks.barrier()
    _lib.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        enc.encode_device(xptr, n, codes.data_ptr(), None)
    sync()
    ranks.barrier()
    dt = time.perf_counter() - t0
    calls, primary_ms, recheck_ms = _lib.profile_collect()
    _lib.set_profiling(False)
    rechecked, used_engine = _lib.last_assign_stats()
    dt = ranks.reduce(dt, "max")
    kern_ms = ranks.reduce(primary_ms / max(calls, 1), "max")
    step_ms = dt / steps * 1e3
    sd = dim // m_
    # the software-pipelined variant serves 8 tiles (k in 225..256) at sub_dim 8 / 16 when a wave's row chunk has >= 8 steps
    piped = (sd in (8, 16) and 224 < k_ <= 256 and os.environ.get("VQHIP_SCREEN_PIPE", "1")[:1] != "0" and n >= 64 * 1024)
    kernel_name = {2: f"k_assign_screen<{sd},16>",
                   3: (f"k_assign_screen_bf16_x32p<{sd},8,false>" if piped else f"k_assign_screen_bf16_x32<{sd},8,1,0,false>")
                   }.get(used_engine, "k_assign_exact")
    out.update({
        "encode_vectors_per_s": n_global * steps / dt, "encode_ms_per_step": step_ms, "prewarm_steps": PREWARM_STEPS,
        "cold_ms_per_step": cold_ms,
        "encode_engine": {1: "exact", 2: "fp32_mfma_screen+exact_recheck", 3: "bf16x3_mfma_screen+exact_recheck"}.get(used_engine, str(used_engine)),
        "recheck_fraction": rechecked / float(max(1, n * m_)),
        "encode_engine_id": int(used_engine),
        "encode_roofline": mfma_roofline(flop_row * n, kern_ms, kernel=kernel_name, engine=used_engine, extra={
            "step_frac": flop_row * n / (step_ms * 1e-3) / 1e12 / (PEAK_BF16X3_EQUIV_TFLOPS if used_engine == 3 else PEAK_F32_MFMA_TFLOPS),
            "recheck_avg_launch_ms": recheck_ms / max(calls, 1), "flop_per_launch": flop_row * n,
            "algorithmic_bytes_per_launch": (4.0 * dim + m_) * n}),
        "codes_checksum_rank0": int(codes.to(torch.int64).sum().item()),
    })
    if snapshot:  # before anything else writes `codes`
        out["_dump"] = (codes.cpu().numpy(), offset)
    if want_f16:  # same pass with the reference-shaped f16 reconstruction written too
        f16 = torch.empty((n, dim), dtype=torch.float16, device="cuda")
        # (the host work in front of this -- checksum, k-means bookkeeping -- lets the clocks fall: two warm-up calls and five
        # timed ones read 0.52 ms for a pass that is 0.44 at steady clocks, tools/decode_time.py; same prewarm as the headline)
        for _ in range(max(2, min(100, PREWARM_STEPS // 2))):
            enc.encode_device(xptr, n, codes.data_ptr(), f16.data_ptr())
        sync()
        t0 = time.perf_counter()
        reps = SIDE_STEPS
        for _ in range(reps):
            enc.encode_device(xptr, n, codes.data_ptr(), f16.data_ptr())
        sync()
        out["encode_f16_out_vectors_per_s_per_gpu"] = n * reps / (time.perf_counter() - t0)
        del f16
    return out, codebooks, (ds, enc, codes)


def worker(args) -> int:
    # stdout carries exactly ONE line, the JSON: native libraries that write to fd 1 (RCCL prints a version banner when a
    # communicator is created) are sent to stderr for the whole run
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} in the environment", file=sys.stderr)
        return 2

    import numpy as np
    import torch

    from vq_amd import _lib

    if not torch.cuda.is_available():
        print("bench.py needs a MI355X (no GPU visible); there is no CPU fallback", file=sys.stderr)
        return 2
    # VQ_BENCH_SHARE_GPU=1: every rank on device 0 (tests of the N > 1 plumbing on a one-GPU box; RCCL refuses two ranks
    # on one device, so only with --collective gloo)
    share = os.environ.get("VQ_BENCH_SHARE_GPU") in ("1", "force")  # "force": let RCCL itself refuse (or take) a shared device
    if os.environ.get("VQ_BENCH_SHARE_GPU") == "1" and world > 1 and args.collective != "gloo":
        print("bench.py: VQ_BENCH_SHARE_GPU=1 needs --collective gloo (RCCL wants one GPU per rank)", file=sys.stderr)
        return 2
    device = 0 if share else local_rank
    if device >= torch.cuda.device_count():
        print(f"bench.py: rank {rank} wants GPU {device}, {torch.cuda.device_count()} visible", file=sys.stderr)
        return 2
    torch.cuda.set_device(device)
    ranks = Ranks(world, rank)
    # VQ_BENCH_FORCE_COMM=1: keep the per-iteration RCCL all-reduce on for a single rank (measures what the
    # collective path adds to an iteration without a second GPU)
    force_comm = world == 1 and os.environ.get("VQ_BENCH_FORCE_COMM") == "1"
    _lib.load()
    _lib.set_device(device)
    stream = torch.cuda.Stream()
    engine = {"auto": _lib.ENGINE_AUTO, "exact": _lib.ENGINE_EXACT, "mfma": _lib.ENGINE_MFMA,
              "bf16": _lib.ENGINE_MFMA_BF16}[args.engine]

    with torch.cuda.stream(stream):
        _lib.set_stream(stream.cuda_stream)
        # ---- the collective: the library's own RCCL communicator (one per process; the control plane is gloo) ----
        collective, ncomm, rccl_world, rccl_rank, group = "none", None, 1, 0, None
        want = args.collective if (world > 1 or force_comm) else "none"
        if want == "native":
            ok, err = 1, ""
            try:
                uid = ranks.bcast(_lib.NativeComm.unique_id() if rank == 0 else None)
                ncomm = _lib.NativeComm(uid, world, rank)
                rccl_world, rccl_rank = ncomm.info()
            except Exception as e:  # noqa: BLE001
                ok, err = 0, str(e)
                print(f"[bench] rank {rank}: native communicator unavailable ({e})", file=sys.stderr)
            if ranks.reduce(float(ok), "min") < 1:  # every rank falls back together
                if ncomm is not None:
                    ncomm.close()
                ncomm, want = None, "torch"
            else:
                collective = "native"
        if want in ("torch", "gloo"):
            import torch.distributed as dist

            if not dist.is_initialized():  # one forced rank
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(free_port()))
                dist.init_process_group("gloo", rank=0, world_size=1)
                ranks.dist = dist
            collective = want
            if want == "torch":  # the data-plane group: nccl (= RCCL)
                try:
                    group = dist.new_group(backend="nccl", device_id=torch.device("cuda", device))
                    rccl_world, rccl_rank = dist.get_world_size(group), dist.get_rank(group)
                except Exception as e:  # noqa: BLE001
                    print(f"[bench] rank {rank}: no nccl group ({e})", file=sys.stderr)
                    return 4
        if collective == "none" and ncomm is None:
            ncomm = _lib.NativeComm(None, 1, 0)  # identity communicator

        main_out, codebooks, keep = measure(args, ranks, args.config, args.scaling, torch=torch, _lib=_lib, engine=engine,
                                            ncomm=ncomm, collective=collective, steps=args.steps, warmup=args.warmup, group=group,
                                            snapshot=bool(args.dump_outputs))
        dump = main_out.pop("_dump", None)
        ds, enc, codes = keep
        n, dim, m_, k_ = main_out["rows_this_rank"], main_out["dim"], main_out["m"], main_out["k"]

        extras = {}
        if rank == 0 and world == 1 and args.config == "C2":
            # (a) H2D-inclusive: host rows in, codes back to the host (never the headline)
            nh = min(n, 1_000_000)
            Xh = _lib.synth_uniform_host(nh, dim, DATA_SEED, 0)
            enc.encode(Xh, want_codes=True, want_f16=False)
            t0 = time.perf_counter()
            for _ in range(3):
                enc.encode(Xh, want_codes=True, want_f16=False)
            extras["encode_host_in_host_out_vectors_per_s"] = nh * 3 / (time.perf_counter() - t0)
            extras["encode_host_rows"] = nh
            # the reference-shaped call: rows in host memory, the f16 reconstruction back in host memory (768 B over PCIe
            # per vector at D = 128: 512 in + 256 out, both directions at once on two lanes below the ABI); into the
            # caller's own array (out=, pages that exist) and into a fresh array per call (its first touch included)
            out16 = np.empty((nh, dim), np.float16)
            enc.encode(Xh, want_codes=False, want_f16=True, out_f16=out16)
            t0 = time.perf_counter()
            for _ in range(3):
                enc.encode(Xh, want_codes=False, want_f16=True, out_f16=out16)
            extras["encode_host_in_f16_out_vectors_per_s"] = nh * 3 / (time.perf_counter() - t0)
            t0 = time.perf_counter()
            enc.encode(Xh, want_codes=False, want_f16=True)  # the process's first fresh result of this size: no pages yet
            extras["encode_host_in_f16_out_first_fresh_array_vectors_per_s"] = nh / (time.perf_counter() - t0)
            t0 = time.perf_counter()
            for _ in range(3):
                enc.encode(Xh, want_codes=False, want_f16=True)  # fresh arrays out of recycled buffers (vq_amd/_arena.py)
            extras["encode_host_in_f16_out_fresh_array_vectors_per_s"] = nh * 3 / (time.perf_counter() - t0)
            extras["encode_host_pcie_bound_vectors_per_s"] = 55e9 / (4.0 * dim)  # rows in at ~55 GB/s, results out concurrently
            del Xh, out16
            # (b) clustered data once (mixture of K Gaussians around the trained centroids' scale):
            # uniform data is the worst case for near-ties, this is the friendly one
            g = torch.Generator(device="cuda").manual_seed(DATA_SEED)
            centers = torch.rand((k_, dim), device="cuda", generator=g)
            which = torch.randint(0, k_, (n,), device="cuda", generator=g)
            Xc = (centers[which] + 0.02 * torch.randn((n, dim), device="cuda", generator=g)).contiguous()
            torch.cuda.synchronize()
            dsc = _lib.Dataset.from_device(Xc.data_ptr(), n, dim)
            kmc = _lib.KMeans(dsc, m_, k_)
            kmc.set_engine(engine)
            kmc.init_from_rows(strided_init(n, m_, k_).astype(np.uint64))
            for _ in range(TRAIN_ITERS):
                kmc.step()
            encc = _lib.PQEncoder(kmc.get_centroids(), _lib.SQUARED_EUCLIDEAN)
            encc.set_engine(engine)
            encc.encode_device(Xc.data_ptr(), n, codes.data_ptr(), None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                encc.encode_device(Xc.data_ptr(), n, codes.data_ptr(), None)
            torch.cuda.synchronize()
            extras["clustered_data_vectors_per_s"] = n * 5 / (time.perf_counter() - t0)
            extras["clustered_data_recheck_fraction"] = _lib.last_assign_stats()[0] / float(n * m_)
            encc.close()
            kmc.close()
            dsc.close()
            del Xc
            # (c) N(0,1) rows (zero-mean, like real embeddings): one encode + one k-means figure with the re-check share
            Xn = torch.randn((n, dim), device="cuda", generator=g).contiguous()
            torch.cuda.synchronize()
            dsn = _lib.Dataset.from_device(Xn.data_ptr(), n, dim)
            kmn = _lib.KMeans(dsn, m_, k_)
            kmn.set_engine(engine)
            init_n = strided_init(n, m_, k_).astype(np.uint64)
            kmn.init_from_rows(init_n)
            kmn.run(TRAIN_ITERS)
            cbn = kmn.get_centroids()
            kmn.init_from_rows(init_n)
            kmn.set_active(np.ones(m_, np.uint8))
            kmn.run(10)
            kmn.init_from_rows(init_n)
            kmn.set_active(np.ones(m_, np.uint8))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            itn, _, _, pausedn = kmn.run(10)
            torch.cuda.synchronize()
            kmn_ms = (time.perf_counter() - t0) * 1e3 / max(1, int(np.asarray(itn).max()))
            encn = _lib.PQEncoder(cbn, _lib.SQUARED_EUCLIDEAN)
            encn.set_engine(engine)
            for _ in range(2):
                encn.encode_device(Xn.data_ptr(), n, codes.data_ptr(), None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                encn.encode_device(Xn.data_ptr(), n, codes.data_ptr(), None)
            torch.cuda.synchronize()
            enc_n_ms = (time.perf_counter() - t0) * 1e3 / 5
            rn, en = _lib.last_assign_stats()
            flop_n = 2.0 * k_ * dim * n
            extras["normal_data"] = {
                "rows": "N(0,1), same shape", "encode_vectors_per_s": n / (enc_n_ms * 1e-3), "encode_ms_per_step": enc_n_ms,
                "recheck_fraction": rn / float(n * m_),
                "encode_roofline": mfma_roofline(flop_n, enc_n_ms, engine=en, extra={"note": "whole step (screen + re-check), wall time"}),
                "kmeans_ms_per_iter": kmn_ms, "kmeans_paused": bool(pausedn), "kmeans_iters_timed": [int(np.asarray(itn).min()), int(np.asarray(itn).max())],
                "kmeans_roofline": mfma_roofline(flop_n * float(np.asarray(itn).sum()) / max(1, int(np.asarray(itn).max())) / m_, kmn_ms, engine=en),
            }
            encn.close()
            kmn.close()
            dsn.close()
            del Xn
        enc.close()
        ds.close()
        del codes, keep
        torch.cuda.empty_cache()

        # ---- N > 1: the same job strong-scaled, and BASELINE configs[4] (12.5M x 128 rows per GPU, m = 16) -------------
        blocks = {}
        if world > 1 and not args.no_configs:
            def block(name, wl_name, scaling):
                try:
                    o, _, kp = measure(args, ranks, wl_name, scaling, torch=torch, _lib=_lib, engine=engine, ncomm=ncomm,
                                       collective=collective, steps=SIDE_STEPS // 2, warmup=2, want_f16=False, group=group)
                    kp[1].close()
                    kp[0].close()
                    del kp
                    torch.cuda.empty_cache()
                    blocks[name] = o
                except Exception as e:  # noqa: BLE001  (every rank runs the same code: they fail or pass together)
                    blocks[name] = {"error": str(e)}

            if not (args.config == "C2" and args.scaling == "strong"):
                block("strong_C2", "C2", "strong")
            if args.config != "C5":
                block("weak_C5", "C5", "weak")
        configs = None
        if rank == 0 and world == 1 and not args.no_configs:
            configs = other_configs(_lib, torch, engine)

    if dump is not None:
        dump_outputs(args.dump_outputs, rank, dump[0], codebooks, world, row_offset=dump[1])
    rc = 0
    if rank == 0:
        o = main_out
        wl = WORKLOADS[args.config]
        traffic, traffic_src = (pmc_traffic(o["encode_roofline"]["kernel"])
                                if (n == N_PER_GPU and args.config == "C2") else (None, None))
        roof = dict(o["encode_roofline"])
        roof.update({
            "note": "achieved = algorithmic 2*k*D flop per row / device time of the screen kernel (HIP events on the "
                    "launch stream, max over ranks); frac = achieved / peak of the pipe that does the work (peak_is): with the "
                    "bf16x3-split engine every fp32 product is six bf16 products on the bf16 matrix pipe, so the roofline is "
                    "2500 / 6 TFLOP/s of algorithmic fp32 work; frac_vs_fp32_mfma_peak reads the same rate against the 157.3 TFLOP/s "
                    "the north star names (its 40 % target) and can pass 1.  What binds the kernel: issue_bound (every "
                    "instruction at the lone wave's ~5.3 cycles) and DESIGN.md 4.1 (VALU + MFMA issue 64 %, stalls behind the matrix pipe 19 %); step_frac = the same work over the whole "
                    "driver-timed step (screen + exact re-check)",
            "traffic": traffic, "traffic_source": traffic_src,
            "kmeans_frac": (o.get("kmeans_roofline") or {}).get("frac"),
            "kmeans_achieved": (o.get("kmeans_roofline") or {}).get("achieved"),
            "kmeans_ms_per_iter": o.get("kmeans_ms_per_iter")})
        line = {
            "metric": "pq_encode_vectors_per_s",
            "value": o["encode_vectors_per_s"],
            "unit": "vectors/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "prewarm_steps": o.get("prewarm_steps"),  # untimed passes in front of the warmup steps (GPU clocks back up after host work)
            "ms_per_step": o["encode_ms_per_step"],
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": ("f32 (bf16x3-split MFMA screen, exact f32 re-check)" if o.get("encode_engine_id") == 3 else "f32"),
            "data": "synthetic",
            "config": {
                "workload": f"PQ m={m_} k={k_} L2 encode on {o['rows_global']}x{dim} f32 rows in all, {n} on this GPU, device-resident "
                            f"({wl['label']}; {args.scaling} scaling); codes out (1 byte per subspace)",
                "rows_per_gpu": n, "rows_global": o["rows_global"], "dim": dim, "m": m_, "k": k_, "sub_dim": dim // m_,
                "engine": o["encode_engine"], "recheck_fraction": o["recheck_fraction"],
                "codebooks": f"{TRAIN_ITERS} Lloyd iterations from strided init rows",
                # the k-means half of BASELINE's metric and the untimed-pass disclosure, in a dict the driver keeps
                "kmeans_iter_per_s": o.get("kmeans_iter_per_s"), "kmeans_ms_per_iter": o.get("kmeans_ms_per_iter"),
                "kmeans_valid": o.get("kmeans_valid"), "kmeans_roofline_frac": (o.get("kmeans_roofline") or {}).get("frac"),
                "kmeans_roofline_frac_vs_fp32_mfma_peak": (o.get("kmeans_roofline") or {}).get("frac_vs_fp32_mfma_peak"),
                "prewarm_steps": o.get("prewarm_steps"), "cold_ms_per_step": o.get("cold_ms_per_step"),
                "cold_vectors_per_s": (o["rows_global"] / (o["cold_ms_per_step"] * 1e-3) if o.get("cold_ms_per_step") else None),
            },
            "roofline": roof,
            "kmeans_rows_global": o["rows_global"],
            "kmeans_collective": {"native": "rccl below the C ABI (vqhip_kmeans_run_sharded)", "torch": "torch.distributed nccl",
                                  "gloo": "torch.distributed gloo (host-staged)", "none": "none"}[collective],
            "rccl_world": rccl_world, "rccl_rank": rccl_rank,
        }
        for key in ("kmeans_iter_per_s", "kmeans_ms_per_iter", "kmeans_iters_requested", "kmeans_iters_timed",
                    "kmeans_active_subspaces", "kmeans_paused", "kmeans_valid", "kmeans_counts_sum_per_subspace",
                    "kmeans_allreduce_ms", "codebooks_abs_sum", "kmeans_roofline", "encode_f16_out_vectors_per_s_per_gpu", "codes_checksum_rank0"):
            line[key] = o.get(key)
        line.update(extras)
        line.update(blocks)
        if configs is not None:
            line["configs"] = configs
        r32, r16, trusted = _lib.selftest()
        line["bf16_mfma_selftest"] = {"ratio_32x32x16": r32, "ratio_16x16x32": r16, "model_bound": 18.1, "budget": 20.0,
                                      "trusted": trusted, "basis": "hardware == bit-exact adder model on 2^22 operand sets"}
        if world == 1 and not args.no_cpu_baseline and args.config == "C2":
            line["cpu_baseline"] = cpu_baseline(m_, k_, dim, codebooks)
        os.write(json_fd, (json.dumps(line) + "\n").encode())
        if not o["kmeans_valid"]:
            print("[bench] the timed k-means run paused or retired subspaces: kmeans_* fields are scaled by the subspaces "
                  "that executed (kmeans_active_subspaces)", file=sys.stderr)
    if ncomm is not None:
        ncomm.close()
    ranks.close()
    return rc


if __name__ == "__main__":
    main()
