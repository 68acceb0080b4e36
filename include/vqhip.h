/*
 * vqhip.h -- C ABI of libvqhip: the MI355X (gfx950) back end for the k-means codebook
 * training and nearest-centroid encode path of CogitatorTech/vq (crate `vq` 0.2.1).
 *
 * This header IS the drop-in boundary.  The reference's only native seam is the per-pair
 * hsdlib FFI (src/core/hsdlib_ffi.rs:37-62: caller-owned pointers + length, one out
 * pointer, int status).  One launch per 16-float pair is useless on a GPU, so the seam
 * moves one level up: each entry point below replaces the BODY of one reference function
 * while the public Rust / Python signatures above it stay as they are (INTEGRATION.md
 * shows the binding a maintainer adds).  Conventions follow hsdlib_ffi.rs:8-35:
 *   - plain C types only; the caller owns every host buffer, the library owns device
 *     memory behind opaque handles released by *_destroy;
 *   - every function returns an int status: 0 ok, negative = error, text of the last
 *     error of the calling thread via vqhip_last_error();
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point
 *     returns VQHIP_ERR_NO_DEVICE.
 *
 * Shape/parameter validation that the reference reports as VqError::EmptyInput /
 * DimensionMismatch / InvalidParameter (src/pq.rs:91-117, src/core/vector.rs:396-410,
 * src/tsvq.rs:196-210) is done by the host-language layer BEFORE the call so that the
 * reference's own messages are preserved; the library re-checks and returns
 * VQHIP_ERR_INVALID_INPUT.  Device failures map to VqError::FfiError (src/core/error.rs:26).
 *
 * RNG: the reference draws initial centroids and empty-cluster reseeds from rand 0.9's
 * StdRng (src/core/vector.rs:412-413, 448-452).  Those draws stay on the host side of this
 * ABI: the caller passes row ids in (vqhip_kmeans_init_from_rows, *_patch_from_row).
 *
 * Threading: every handle may be used from any number of threads at once -- the reference's
 * quantizers are plain data, `Send + Sync`, and `quantize(&self)` runs on thread pools
 * (src/pq.rs:39-45, 167-199; src/tsvq.rs:186-191, 239-255).  Each handle carries a lock that an
 * entry point holds while it touches the handle's state; a call that returns with work still
 * queued (the *_device forms, vqhip_kmeans_accumulate, _patch_from_row) is followed, on whatever
 * stream the next call on that handle arrives, by a wait for that work (an event; no host wait).
 * Per-vector calls (vqhip_pq_encode / vqhip_tsvq_encode with n <= 8) stage through buffers owned by
 * the CALL and give the handle back before they launch, so calls from many threads on one
 * quantizer overlap on the device.  A vqhip_dataset is immutable and complete when it is handed
 * out: share it freely; so is a vqhip_range (every range search, the *_device forms too, waits for
 * its result).  The search handles (flat, sqindex, binary, ivfpq, ivfflat, ivfsq, ivfsq4, ivfbin) serialise
 * their calls on the handle's lock: each call owns every workspace of the handle, a filtered call's
 * row mask is in force for that call alone, and a call that needs a larger workspace frees the old
 * one only after the device has finished with it.  An add to an inverted file may run beside
 * searches of it from other threads: add and search take turns, so a search sees all rows of every
 * add that had returned when it started and none or all of one that ran beside it -- n, list_sizes
 * and the row mask's length (ceil(n / 32) words, read at the time of the call; a longer mask is
 * fine, its bits at or past n are ignored) follow the same rule.  What stays with the caller: a
 * handle must outlive the calls on it (destroy is not a synchronisation point), and caller-owned
 * device buffers passed to *_device forms are ordered by the caller -- a later call of ANOTHER
 * thread on the handle is ordered behind the queued work, the caller's own reads of the outputs
 * are not.  Work is enqueued on the calling thread's current stream
 * (vqhip_set_stream; default: a per-thread stream the library creates) of the current HIP device.
 * vqhip_last_error / vqhip_last_assign_stats / vqhip_set_profiling are per calling thread.
 */
#ifndef VQHIP_H
#define VQHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQHIP_VERSION_MAJOR 0
#define VQHIP_VERSION_MINOR 1

/* status codes: 0/-1/-3/-4/-99 keep hsdlib's meaning (src/core/hsdlib_ffi.rs:8-16) */
#define VQHIP_OK 0
#define VQHIP_ERR_NULL_PTR (-1)
#define VQHIP_ERR_INVALID_INPUT (-3)
#define VQHIP_ERR_NO_DEVICE (-4)   /* hsdlib: "CPU not supported"; here: no gfx950 GPU */
#define VQHIP_ERR_RUNTIME (-5)     /* HIP runtime / launch failure */
#define VQHIP_ERR_UNSUPPORTED (-6) /* valid input outside what this build handles */
#define VQHIP_ERR_FAILURE (-99)

/* distance metrics, same order as `enum Distance` (src/core/distance.rs:8-17) */
#define VQHIP_SQUARED_EUCLIDEAN 0
#define VQHIP_EUCLIDEAN 1
#define VQHIP_MANHATTAN 2
#define VQHIP_COSINE 3
/* Opt-in, UNPINNED: the cosine distance of the reference's `simd` build (which pyvq always uses,
 * pyvq/Cargo.toml:13): `1.0 - hsd_sim_cosine_f32(a, b)` with no EPSILON rule and no clamp
 * (src/core/distance.rs:97-105).  hsdlib's source is not part of the reference tree, so its summation order is
 * unknown; this id keeps the scalar path's three sequential sums and changes only what is visible in the Rust
 * source: d = 1 - dot / (|a| |b|), which may exceed 1, dip below 0 by rounding, and is NaN / inf for a zero norm
 * (a NaN distance never wins the argmin, as in the reference's `<` scan).  Exact engines only (no screen). */
#define VQHIP_COSINE_UNCLAMPED 4

/* assignment engines (results are bit-identical; this is a speed/diagnostic knob) */
#define VQHIP_ENGINE_AUTO 0  /* fastest available: bf16-split MFMA screen, fp32 MFMA screen, exact */
#define VQHIP_ENGINE_EXACT 1 /* exact VALU scan of every centroid */
#define VQHIP_ENGINE_MFMA 2  /* fp32 MFMA screen + exact re-check (error if the shape is unsupported) */
#define VQHIP_ENGINE_MFMA_BF16 3 /* 3-way bf16-split MFMA screen + exact re-check */

typedef struct vqhip_dataset vqhip_dataset;
typedef struct vqhip_kmeans vqhip_kmeans;
typedef struct vqhip_pq_encoder vqhip_pq_encoder;
typedef struct vqhip_tsvq vqhip_tsvq;

/* ---- library / device -------------------------------------------------------------- */

/* analogue of hsd_get_backend() (src/core/hsdlib_ffi.rs:61, 144-155): static string */
const char *vqhip_backend(void);
/* text of the calling thread's last error ("" if none); valid until the next failing call */
const char *vqhip_last_error(void);
/* number of visible gfx950 devices (0 if none / no HIP runtime) */
int vqhip_device_count(void);
/* select the HIP device for the calling thread (like hipSetDevice) */
int vqhip_set_device(int device);
/* the calling thread's current device (what the single-device handles below run on) */
int vqhip_get_device(int *device);
/* hipStream_t (as void*) the calling thread's subsequent calls enqueue on; NULL = the
 * library's own per-thread non-blocking stream */
int vqhip_set_stream(void *hip_stream);
/* block until the calling thread's stream is idle */
int vqhip_synchronize(void);
/* One-time device self-test behind the bf16-split engine.  The screen's margin uses a bound on the
 * accumulation error of v_mfma_f32_32x32x16_bf16 that is derived from a bit-exact software model of its
 * adder (vqhip_mfma_bf16_model below); the self-test checks on the running device that the hardware
 * equals the model (2^22 generated operand sets, bit equality) and reports the worst observed error of
 * both bf16 MFMA shapes in units of 2^-24 (|C| + sum|a*b|) (the model's bound is 18.1, the margins
 * budget 20).  *trusted = 1 iff no mismatch was found; otherwise ENGINE_AUTO uses the fp32 MFMA screen
 * and ENGINE_MFMA_BF16 is refused.  Any out-pointer may be NULL. */
int vqhip_selftest(float *bf16_32x32x16_ratio, float *bf16_16x16x32_ratio, int *bf16_engine_trusted);
/* Diagnostics: d[t] = the f32 result of ONE v_mfma_f32_32x32x16_bf16 for the dot product of the bf16
 * vectors a[t][0..16) and b[t][0..16) (raw bf16 bit patterns) added to c[t] -- the instruction the
 * screen's contraction runs on.  tests/ hold a bit-exact software model of its adder against this
 * entry point (DESIGN.md "screen soundness").  Host buffers. */
int vqhip_mfma_bf16_probe(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d);
/* The library's bit-exact software model of that instruction's adder (vq_amd/csrc/mfma_model.hpp: two
 * passes of 8 products, truncation to 2^(Ep-24), a 32-bit frame with C, round to nearest even), from
 * which the screen's margin is derived: same arguments, evaluated on the host (no device needed). */
int vqhip_mfma_bf16_model(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d);
/* model == hardware on `trials` operand sets generated on the device from `seed` (eight families that
 * reach every branch of the model); *mismatches must be 0, *first_bad_trial names the first failure. */
int vqhip_mfma_bf16_model_check(uint64_t trials, uint64_t seed, uint64_t *mismatches, uint64_t *first_bad_trial);
/* the same run, reporting up to `cap` failing trial numbers; and the operand set (a[16], b[16], *c) that the
 * check generates for one (seed, trial), on the host: together they reproduce a reported failure */
int vqhip_mfma_bf16_model_failures(uint64_t trials, uint64_t seed, uint64_t *trial_ids, uint32_t cap, uint64_t *n_failures);
int vqhip_mfma_bf16_model_case(uint64_t seed, uint64_t trial, uint16_t *a, uint16_t *b, float *c);
/* statistics of the most recent assign/encode launch of this thread: rows sent to the
 * exact re-check, and the engine used (VQHIP_ENGINE_EXACT / _MFMA) */
int vqhip_last_assign_stats(uint64_t *rechecked, int *engine);
/* bf16 products per dimension of the screen kernel behind that launch: 6 (three-slice operands), 3 (the two-slice
 * form of the sub_dim-16 encode screen), 0 when no bf16 screen ran (exact or fp32-MFMA engine).  Per calling thread. */
int vqhip_last_screen_products(int *products);

/* per-call HIP-event timing of the assignment stages on the launch stream.  While on, every
 * assign/encode call records events; collect() synchronises, returns the number of calls and
 * the summed device time of the primary stage (MFMA screen, or the exact scan when that is
 * the engine) and of the exact re-check stage, and clears the record. */
int vqhip_set_profiling(int on);
int vqhip_profile_collect(uint32_t *n_calls, double *primary_ms, double *recheck_ms);
/* process-wide count of host-batch calls (vqhip_pq_encode / vqhip_tsvq_encode / vqhip_dataset_from_host on host
 * pointers) that went through the library's transfer lanes (several host threads, each with its own stream: uploads,
 * kernels and downloads of different chunks overlap) rather than the one-stream path -- diagnostics and tests */
int vqhip_xfer_lane_calls(uint64_t *calls);
/* process-wide count of the HIP events the library's event pool holds (stage times with profiling on, the ordering
 * event a call's last kernel carries): bounded by the events in use at one time, not by the number of calls --
 * diagnostics and tests */
int vqhip_event_pool_count(uint64_t *events);
/* device-to-device copy on the current stream (plumbing for callers that all-reduce the
 * k-means slab in their own buffers) */
int vqhip_memcpy_device(void *dst, const void *src, uint64_t bytes);

/* ---- datasets: a row-major [n][d] f32 matrix resident in HBM -------------------------
 * replaces the `&[&[f32]]` argument of ProductQuantizer::new / TSVQ::new (src/pq.rs:84,
 * src/tsvq.rs:195) and the per-subspace copies of src/pq.rs:122-129 (never materialised:
 * kernels index X[row][s*sub_dim ..] in place). */
int vqhip_dataset_from_host(const float *rows, uint64_t n, uint32_t d, vqhip_dataset **out);
/* borrow an existing device buffer (not freed by _destroy) */
int vqhip_dataset_from_device(const void *dev_rows, uint64_t n, uint32_t d, vqhip_dataset **out);
/* i.i.d. Uniform[0,1) rows generated on the device by the counter-based generator of
 * vqhip_synth_uniform_host: element (row, col) depends only on (seed, row_offset+row, col).
 * Mirrors the reference harness data, src/bin/common.rs:43-53. */
int vqhip_dataset_synthetic(uint64_t n, uint32_t d, uint64_t seed, uint64_t row_offset,
                            vqhip_dataset **out);
int vqhip_dataset_info(const vqhip_dataset *ds, uint64_t *n, uint32_t *d, const void **dev_rows);
int vqhip_dataset_read(const vqhip_dataset *ds, uint64_t row0, uint64_t nrows, float *out);
int vqhip_dataset_destroy(vqhip_dataset *ds);
/* host twin of the device generator (pure data generation; no compute fallback) */
int vqhip_synth_uniform_host(float *out, uint64_t n, uint32_t d, uint64_t seed,
                             uint64_t row_offset);

/* ---- code width ----------------------------------------------------------------------
 * The reference keeps a `usize` best_idx per subspace (src/pq.rs:183-191, vector.rs:417); this
 * library stores it in the narrowest of two widths, chosen by k alone:
 *     k <= 256          one byte per (row, subspace)
 *     256 < k <= 65536  one little-endian uint16_t per (row, subspace)
 * Every `codes` buffer below (host or device) is [n][m] of that width, i.e.
 * n * m * vqhip_code_bytes(k) bytes; the parameter stays `uint8_t *` for both.  Above 256 the bf16
 * screen runs in up to 16 centroid groups per subspace (sub_dim 8/12/16/24: k <= 4096, 32: 2048,
 * 48/64: 1024), the exact VALU engine serves every other shape. */
uint32_t vqhip_code_bytes(uint32_t k);

/* ---- k-means (Lloyd / LBG) over all m subspaces at once -------------------------------
 * replaces the body of lbg_quantize (src/core/vector.rs:415-458) as called once per
 * subspace by ProductQuantizer::new (src/pq.rs:120-132).  m == 1 with sub_dim == d is
 * plain lbg_quantize (src/core/vector.rs:390-395).  Assignment is always squared L2,
 * first minimum wins (vector.rs:352-363), whatever metric the quantizer later uses. */
int vqhip_kmeans_create(const vqhip_dataset *ds, uint32_t m, uint32_t k, vqhip_kmeans **out);
int vqhip_kmeans_destroy(vqhip_kmeans *km);
/* centroids [m][k][d/m] from the host */
int vqhip_kmeans_set_centroids(vqhip_kmeans *km, const float *centroids);
/* centroids[s][j] = row init_rows[s*k+j] restricted to subspace s (vector.rs:412-413 with
 * the choose_multiple draw made by the caller) */
int vqhip_kmeans_init_from_rows(vqhip_kmeans *km, const uint64_t *init_rows);
int vqhip_kmeans_get_centroids(vqhip_kmeans *km, float *centroids);
/* which subspaces still iterate (each converges on its own, src/pq.rs:121 + vector.rs:455);
 * active [m] of 0/1.  Default: all active. */
int vqhip_kmeans_set_active(vqhip_kmeans *km, const uint8_t *active);
/* the set as the library holds it now: what _set_active last wrote, minus the subspaces vqhip_kmeans_run retired
 * since (it retires a converged subspace in the iteration it converges, vector.rs:455-457).  A host that mirrors the
 * set must re-read it after every _run / _run_sharded: a subspace may have retired iterations BEFORE the one that
 * paused the run, and `counts` of a subspace that did not execute the last iteration are 0, not "empty clusters". */
int vqhip_kmeans_get_active(const vqhip_kmeans *km, uint8_t *active);
int vqhip_kmeans_set_engine(vqhip_kmeans *km, int engine);
/* exact_update != 0: cluster means are the reference's sequential f32 sums in row order
 * (bit-identical to mean_vector_by_indices, vector.rs:368-384) instead of the default
 * blocked f32 + f64 combination (faster; within the tolerance stated in DESIGN.md).
 * Needs k <= 16384. */
int vqhip_kmeans_set_exact_update(vqhip_kmeans *km, int exact_update);

/* One Lloyd iteration = assign + accumulate + reduce + finalize for every active subspace:
 *   counts  [m][k] out (optional): members per cluster (0 => caller reseeds, vector.rs:448)
 *   changed [m]    out (optional): 1 iff some non-empty cluster moved >= 1e-6 (vector.rs:444)
 * Empty clusters keep their previous centroid until the caller patches them.
 * (For launch-bound sizes, n*m <= 4M, the step is captured once per active set and replayed as
 * a hipGraph; results are identical.  VQHIP_GRAPH=0 disables.) */
int vqhip_kmeans_step(vqhip_kmeans *km, uint32_t *counts, uint8_t *changed);

/* The loop of lbg_quantize (vector.rs:415-458) without a host round trip per iteration: up to max_iters iterations
 * are queued back to back and the loop's decisions are taken on the device -- a subspace whose centroids did not move
 * (`changed` false, vector.rs:455-457) stops being processed, and an empty cluster in an active subspace PAUSES the run
 * after that iteration (*paused = 1) because the reseed row is the caller's draw (vector.rs:448-452): read the active
 * set (vqhip_kmeans_get_active: subspaces that converged in an EARLIER iteration of this call are already retired and
 * their counts read 0), patch the empty clusters (counts == 0) of the subspaces still active, retire those of them with
 * changed == 0 (vqhip_kmeans_set_active) and call again with the iterations that are left.  Out (all optional): iters_done [m] iterations executed per subspace in this call; counts
 * [m][k] and changed [m] of the last executed iteration.  Without a pause the converged subspaces are already retired
 * when the call returns.  Shapes without the fused update take the same decisions on the host, one step at a time. */
int vqhip_kmeans_run(vqhip_kmeans *km, uint32_t max_iters, uint32_t *iters_done, uint32_t *counts, uint8_t *changed,
                     int *paused);

/* Split form for row-sharded multi-GPU training (one process per GPU):
 *   accumulate: assign + per-cluster partial sums/counts of THIS shard into a device slab
 *               of f64 [m][k][d/m + 1] (last column = count)
 *   partials:   device pointer + length of that slab, for the caller's all-reduce(sum)
 *   finalize:   means, 1e-6 convergence test, new centroids (identical on every rank after
 *               an all-reduce) */
int vqhip_kmeans_accumulate(vqhip_kmeans *km);
/* (the slab entries of subspaces that are not active -- retired, or gated off inside vqhip_kmeans_run[_sharded] -- are
 * undefined: nothing rewrites them, and a sharded run's all-reduce keeps summing what was there) */
int vqhip_kmeans_partials(vqhip_kmeans *km, void **dev_slab, uint64_t *n_doubles);
int vqhip_kmeans_finalize(vqhip_kmeans *km, uint32_t *counts, uint8_t *changed);

/* ---- row-sharded training over the GPUs of one node (RCCL over xGMI, below this ABI) ----------
 * Generalises the reference's only parallel loop (rayon over rows in the assignment step,
 * src/core/vector.rs:417-423): one process (or thread) per GPU holds a contiguous block of rows as
 * its vqhip_dataset and runs the SAME sequence of calls; each Lloyd iteration exchanges exactly one
 * buffer -- the f64 slab [m][k][d/m+1] of per-cluster sums and counts -- with ncclAllReduce(sum) on
 * the calling thread's stream, after which every rank computes identical means and `changed` flags.
 *   comm_unique_id : ncclGetUniqueId; rank 0 calls it, the host program hands the 128 bytes to the
 *                    other ranks (environment, file, socket: the library does not care)
 *   comm_create    : ncclCommInitRank on the calling thread's current device; collective over the
 *                    ranks.  id == NULL with world == 1 makes a communicator whose collectives are
 *                    the identity (RCCL is then not even loaded)
 *   comm_adopt     : borrow a caller-owned ncclComm_t (e.g. the one a framework already holds)
 * librccl is opened with dlopen at first use (VQHIP_RCCL_LIB overrides its path). */
typedef struct vqhip_comm vqhip_comm;
#define VQHIP_COMM_ID_BYTES 128
int vqhip_comm_unique_id(uint8_t *id /* [VQHIP_COMM_ID_BYTES] out */);
int vqhip_comm_create(const uint8_t *id, int world, int rank, vqhip_comm **out);
int vqhip_comm_adopt(void *nccl_comm, vqhip_comm **out);
int vqhip_comm_info(const vqhip_comm *comm, int *world, int *rank);
int vqhip_comm_destroy(vqhip_comm *comm);
/* The ranks of ONE process (a host thread per GPU) need no communicator library: an in-process group exchanges the slab
 * directly -- every rank publishes its slab on its own device, every rank's stream then adds all published slabs IN RANK
 * ORDER through peer access (xGMI): stream-ordered like ncclAllReduce, the same bits on every rank and run to run.
 *   comm_group_create : the shared state of `world` ranks (<= 16)
 *   comm_create_local : rank `rank` of the group, on the calling thread's current device; collective over the group's
 *                       ranks, each called from its own thread.  Two ranks may name the same device.
 *   comm_kind         : 0 identity (one rank), 1 RCCL, 2 in-process exchange
 * Destroy the ranks' communicators (streams drained) before the group. */
typedef struct vqhip_comm_group vqhip_comm_group;
int vqhip_comm_group_create(int world, vqhip_comm_group **out);
int vqhip_comm_create_local(vqhip_comm_group *group, int rank, vqhip_comm **out);
int vqhip_comm_group_destroy(vqhip_comm_group *group);
int vqhip_comm_kind(const vqhip_comm *comm, int *kind);
/* Failure containment.  Every host-side wait of an in-process group is bounded (VQHIP_COMM_TIMEOUT_S, default 60 s), and
 * a rank whose sharded call fails on its own (allocation, launch) poisons its group so that the peers' calls return
 * VQHIP_ERR_RUNTIME at once instead of waiting for it; a poisoned group stays poisoned, its handles destroy normally.
 * vqhip_comm_create_local ends -- and vqhip_comm_create with an id continues -- with an exchange self-test: a
 * rank-dependent pattern is published, every peer's buffer is read on its own and all-reduced, and a wrong word fails
 * the call naming the device pair.
 *   comm_abort : from ANY thread: poison the group of an in-process communicator / ncclCommAbort an owned RCCL one, so
 *                that a thread blocked in a collective with it returns (what the one-process handles below do when one
 *                of their ranks fails) */
int vqhip_comm_abort(vqhip_comm *comm);
/* in-place all-reduce of the slab between _accumulate and _finalize (NULL comm: no-op) */
int vqhip_kmeans_allreduce(vqhip_kmeans *km, vqhip_comm *comm);
/* = accumulate + allreduce + finalize: vqhip_kmeans_step for a sharded data set; counts are global */
int vqhip_kmeans_step_sharded(vqhip_kmeans *km, vqhip_comm *comm, uint32_t *counts, uint8_t *changed);
/* vqhip_kmeans_run for a sharded data set: the all-reduce is queued between accumulate and finalize of every
 * iteration; every rank pauses / retires alike because every rank sees the same global counts and flags */
int vqhip_kmeans_run_sharded(vqhip_kmeans *km, vqhip_comm *comm, uint32_t max_iters, uint32_t *iters_done,
                             uint32_t *counts, uint8_t *changed, int *paused);
/* vqhip_kmeans_init_from_rows with GLOBAL row ids [m][k]: this rank owns rows [row_offset,
 * row_offset + n); the owner of each row supplies its bits, one u32-sum all-reduce hands them to
 * everyone (a float sum would lose the sign of -0.0) */
int vqhip_kmeans_init_from_global_rows(vqhip_kmeans *km, vqhip_comm *comm, const uint64_t *global_rows,
                                       uint64_t row_offset);
/* vqhip_kmeans_patch_from_row with a GLOBAL row id (empty-cluster reseed, vector.rs:448-452) */
int vqhip_kmeans_patch_from_global_row(vqhip_kmeans *km, vqhip_comm *comm, uint32_t s, uint32_t j,
                                       uint64_t global_row, uint64_t row_offset);
/* for hosts that run their own collective: bits_out [m][k][d/m] (host) = bit patterns of the owned
 * rows among global_rows [m][k], zero words for rows of other ranks; ONE gather launch + ONE copy */
int vqhip_kmeans_gather_owned_rows(vqhip_kmeans *km, const uint64_t *global_rows, uint64_t row_offset,
                                   uint32_t *bits_out);

/* ---- one call, one process, several GPUs ------------------------------------------------------
 * `ProductQuantizer::new` is ONE call in ONE process (src/pq.rs:83-141).  These handles put the ranks of the
 * row-sharded fit above INSIDE the library: a worker thread per entry of `devices` (its device current, its own
 * stream), each holding a contiguous block of the rows (the first n % n_devices blocks one row longer), a vqhip_kmeans
 * on it and a communicator -- the in-process exchange by default, RCCL with VQHIP_MULTI_COMM=rccl -- and every call
 * below runs the per-rank entry point of the same name on all workers at once (init_from_rows / patch_from_row take
 * GLOBAL row ids; run = vqhip_kmeans_run_sharded).  Same results contract as the sharded fit; with one device the
 * bits of the single-device handles.  `devices` may name a device more than once (in-process exchange only).
 * The Rust shim's `ProductQuantizer::new` keeps its signature and passes the visible devices. */
typedef struct vqhip_mdataset vqhip_mdataset;
typedef struct vqhip_mkmeans vqhip_mkmeans;
typedef struct vqhip_mpq_encoder vqhip_mpq_encoder;
int vqhip_mdataset_from_host(const float *rows, uint64_t n, uint32_t d, const int *devices, int n_devices,
                             vqhip_mdataset **out);
int vqhip_mdataset_synthetic(uint64_t n, uint32_t d, uint64_t seed, const int *devices, int n_devices,
                             vqhip_mdataset **out);
/* rows_per_device [n_devices] out (optional) */
int vqhip_mdataset_info(const vqhip_mdataset *ds, uint64_t *n, uint32_t *d, int *n_devices, uint64_t *rows_per_device);
int vqhip_mdataset_destroy(vqhip_mdataset *ds);
/* the data set must outlive the k-means handle */
int vqhip_mkmeans_create(vqhip_mdataset *ds, uint32_t m, uint32_t k, vqhip_mkmeans **out);
int vqhip_mkmeans_destroy(vqhip_mkmeans *km);
/* world = n_devices; comm_kind as vqhip_comm_kind */
int vqhip_mkmeans_info(vqhip_mkmeans *km, int *world, int *comm_kind);
int vqhip_mkmeans_set_engine(vqhip_mkmeans *km, int engine);
/* vqhip_kmeans_set_exact_update; VQHIP_ERR_UNSUPPORTED with more than one device slot */
int vqhip_mkmeans_set_exact_update(vqhip_mkmeans *km, int exact_update);
int vqhip_mkmeans_init_from_rows(vqhip_mkmeans *km, const uint64_t *init_rows);
int vqhip_mkmeans_set_centroids(vqhip_mkmeans *km, const float *centroids);
int vqhip_mkmeans_get_centroids(vqhip_mkmeans *km, float *centroids);
int vqhip_mkmeans_set_active(vqhip_mkmeans *km, const uint8_t *active);
int vqhip_mkmeans_get_active(vqhip_mkmeans *km, uint8_t *active);
int vqhip_mkmeans_run(vqhip_mkmeans *km, uint32_t max_iters, uint32_t *iters_done, uint32_t *counts, uint8_t *changed,
                      int *paused);
int vqhip_mkmeans_patch_from_row(vqhip_mkmeans *km, uint32_t s, uint32_t j, uint64_t row);
/* vqhip_pq_encode with the host rows split in row blocks over the devices (no collective) */
int vqhip_mpq_encoder_create(const float *codebooks, uint32_t m, uint32_t k, uint32_t sub_dim, int metric,
                             const int *devices, int n_devices, vqhip_mpq_encoder **out);
int vqhip_mpq_encoder_set_engine(vqhip_mpq_encoder *enc, int engine);
int vqhip_mpq_encode(vqhip_mpq_encoder *enc, const float *rows, uint64_t n, uint8_t *codes, uint16_t *f16_out);
/* the RESIDENT rows of a sharded data set (same device list) through the encoder, `repeat` passes per device; codes_host
 * [n][m] (optional) receives the last pass's codes */
int vqhip_mpq_encode_dataset(vqhip_mpq_encoder *enc, vqhip_mdataset *ds, uint32_t repeat, uint8_t *codes_host);
int vqhip_mpq_encoder_destroy(vqhip_mpq_encoder *enc);
/* the other row-sharded paths (no collective): reconstruction from codes and f16 -> f32 in blocks over the encoder's
 * devices (the batch forms of Quantizer::dequantize, src/pq.rs:201-209) */
int vqhip_mpq_decode(vqhip_mpq_encoder *enc, const uint8_t *codes, uint64_t n, float *out);
int vqhip_mpq_dequantize_f16(vqhip_mpq_encoder *enc, const uint16_t *f16_in, uint64_t count, float *out);
/* TSVQ::quantize / dequantize for a batch (src/tsvq.rs:239-265) over several devices: the flattened tree replicated,
 * host rows in row blocks, each device descends its own; arguments as vqhip_tsvq_create / _encode / _last_stats
 * (undecided summed over the devices) */
typedef struct vqhip_mtsvq vqhip_mtsvq;
int vqhip_mtsvq_create(const float *centroids, const int32_t *left, const int32_t *right, uint32_t n_nodes, uint32_t d,
                       int metric, const int *devices, int n_devices, vqhip_mtsvq **out);
int vqhip_mtsvq_encode(vqhip_mtsvq *t, const float *rows, uint64_t n, int32_t *leaf, uint16_t *f16_out);
int vqhip_mtsvq_dequantize_f16(vqhip_mtsvq *t, const uint16_t *f16_in, uint64_t count, float *out);
int vqhip_mtsvq_last_stats(vqhip_mtsvq *t, int *screened, uint64_t *undecided);
int vqhip_mtsvq_destroy(vqhip_mtsvq *t);
/* the contiguous row block of `rank` among `world` ranks: the first n % world blocks are one row longer */
int vqhip_shard_rows(uint64_t n, int world, int rank, uint64_t *offset, uint64_t *count);

/* empty-cluster reseed (vector.rs:448-452): the caller draws the row */
int vqhip_kmeans_patch_centroid(vqhip_kmeans *km, uint32_t s, uint32_t j, const float *sub_row);
int vqhip_kmeans_patch_from_row(vqhip_kmeans *km, uint32_t s, uint32_t j, uint64_t row);
/* assignment codes [n][m] (see "code width") of the most recent step/accumulate (the
 * reference's `assignments`, vector.rs:417-429), copied to the host */
int vqhip_kmeans_get_assignments(vqhip_kmeans *km, uint8_t *codes);

/* ---- PQ encode -----------------------------------------------------------------------
 * replaces the loop of ProductQuantizer::quantize (src/pq.rs:177-196) for a whole batch.
 * codebooks [m][k][sub_dim] f32 on the host; k <= 65536 (see "code width"). */
int vqhip_pq_encoder_create(const float *codebooks, uint32_t m, uint32_t k, uint32_t sub_dim,
                            int metric, vqhip_pq_encoder **out);
int vqhip_pq_encoder_destroy(vqhip_pq_encoder *enc);
int vqhip_pq_encoder_set_engine(vqhip_pq_encoder *enc, int engine);
/* host batch: rows [n][m*sub_dim];  codes [n][m] (optional, "code width") = best_idx per subspace
 * (pq.rs:183-191);  f16_out [n][m*sub_dim] (optional) = selected centroids as IEEE
 * binary16 bits, round-to-nearest-even (pq.rs:193-195).  Calls with n <= 8 (the reference's
 * one-vector-per-call `quantize`) take a single-kernel latency path over pinned memory with the
 * same results (~20 us per call instead of ~60). */
int vqhip_pq_encode(vqhip_pq_encoder *enc, const float *rows, uint64_t n, uint8_t *codes,
                    uint16_t *f16_out);
/* device batch: all pointers are device pointers; asynchronous on the current stream */
int vqhip_pq_encode_device(vqhip_pq_encoder *enc, const void *dev_rows, uint64_t n,
                           void *dev_codes, void *dev_f16_out);
/* Quantizer::dequantize for a batch (src/pq.rs:201-209): f16 bits -> f32, host buffers */
int vqhip_dequantize_f16(const uint16_t *f16_in, uint64_t count, float *out);
/* reconstruction from codes: out[n][m*sub_dim] f32 = codebook[s][codes[n][s]] (new API) */
int vqhip_pq_decode(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, float *out);
/* device forms of the two: device pointers, asynchronous on the current stream; codes must lie in [0, k) (the host
 * form checks them, this one cannot) */
int vqhip_pq_decode_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, void *dev_out);
int vqhip_dequantize_f16_device(const void *dev_f16_in, uint64_t count, void *dev_out);

/* ---- ScalarQuantizer / BinaryQuantizer (src/sq.rs, src/bq.rs) ------------------------
 * Stateless elementwise maps, bit-identical to the reference's `quantize` / `dequantize`:
 *   SQ encode  code = min(sat(round((clamp(x, min, max) - min) / step)), levels - 1), step = (max - min) / (levels - 1)
 *              (f32 throughout; round half away from zero; NaN -> 0, +inf -> levels - 1)
 *   SQ decode  min + (float)code * step for every byte (codes >= levels included; no fused multiply-add)
 *   BQ encode  x >= threshold ? high : low (NaN -> low)
 *   BQ decode  code >= high ? high : low
 * Parameters are checked first, in the reference's order, before any device is touched: VQHIP_ERR_INVALID_INPUT with
 * its `Display` text ("Invalid parameter 'max': must be greater than min") in vqhip_last_error.  count == 0 is OK.
 * Host forms take host buffers and return when the results are there; the _device forms take device pointers of any
 * element alignment and are asynchronous on the current stream. */
int vqhip_sq_check(float min, float max, uint32_t levels, float *step); /* no device; step may be NULL */
/* b[0..levels): b[0] = -inf, b[i] = the smallest f32 whose code is >= i (NaN if no input reaches i); no device */
int vqhip_sq_thresholds(float min, float max, uint32_t levels, float *b);
int vqhip_sq_encode(float min, float max, uint32_t levels, const float *x, uint64_t count, uint8_t *codes);
int vqhip_sq_encode_device(float min, float max, uint32_t levels, const void *dev_x, uint64_t count, void *dev_codes);
int vqhip_sq_decode(float min, float max, uint32_t levels, const uint8_t *codes, uint64_t count, float *out);
int vqhip_sq_decode_device(float min, float max, uint32_t levels, const void *dev_codes, uint64_t count, void *dev_out);
int vqhip_bq_check(float threshold, uint32_t low, uint32_t high); /* no device; low, high <= 255 */
int vqhip_bq_encode(float threshold, uint32_t low, uint32_t high, const float *x, uint64_t count, uint8_t *codes);
int vqhip_bq_encode_device(float threshold, uint32_t low, uint32_t high, const void *dev_x, uint64_t count,
                           void *dev_codes);
int vqhip_bq_decode(float threshold, uint32_t low, uint32_t high, const uint8_t *codes, uint64_t count, float *out);
int vqhip_bq_decode_device(float threshold, uint32_t low, uint32_t high, const void *dev_codes, uint64_t count,
                           void *dev_out);

/* ---- pairwise distances --------------------------------------------------------------
 * Distance::compute (src/core/distance.rs:48-64, scalar paths 76-82, 94, 107-119) for n
 * independent pairs: out[i] = metric(a[i][0..d), b[i][0..d)).  Host buffers. */
int vqhip_distance_batch(int metric, const float *a, const float *b, uint64_t n, uint32_t d,
                         float *out);

/* ---- asymmetric distance search over stored codes --------------------
 * No reference counterpart (the crate stores f16 reconstructions, src/pq.rs:165-199); semantics =
 * oracle/vq_oracle.c:vqo_adc_search: D(q, i) = sum over subspaces, in order, of the reference's
 * per-subspace distance (squared L2 or L1) between the query's sub-vector and centroid
 * codes[i][s]; the topk rows by (D, row index) ascending; Euclidean reports sqrt(D); cosine is
 * not separable (VQHIP_ERR_UNSUPPORTED).  codes [n][m] u8, queries [nq][dim] host f32,
 * idx_out / dist_out [nq][topk] host; 1 <= topk <= min(n, 1024).
 * Two schedules, one result: n >= 32768 and topk <= 256 take ONE scan of the codes per batch of
 * queries against a threshold from a sample of the rows and keep only the rows at or below it; a
 * query whose threshold let fewer than topk (or more than 8192) rows pass -- and every other shape
 * -- goes through the full pass (all distances, histogram cut).  vqhip_pq_adc_last_redone: how many
 * queries of the encoder's last call took the full pass (diagnostics; VQHIP_ADC_FAST=0 sends all).
 * Table limit: m * k <= 38400 (one query's f32 table in 150 KiB of LDS), the same for both schedules;
 * a larger table is refused with VQHIP_ERR_UNSUPPORTED before any work, whatever n and topk. */
int vqhip_pq_adc_search(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, const float *queries,
                        uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out);
int vqhip_pq_adc_search_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n,
                               const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                               float *dist_out);
/* a code store searched repeatedly: set_codes checks the codes against k and uploads them once into the encoder
 * (replacing an earlier set; n = 0 drops them); search_resident = search_device over that copy */
int vqhip_pq_adc_set_codes(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n);
int vqhip_pq_adc_search_resident(vqhip_pq_encoder *enc, const float *queries, uint32_t nq,
                                 uint32_t topk, uint32_t *idx_out, float *dist_out);
int vqhip_pq_adc_last_redone(vqhip_pq_encoder *enc, uint32_t *queries_out);
/* Filtered ADC search: the three calls above under a ROW MASK, `allowed`: ceil(n / 32) u32 words in HOST
 * memory (copied once per call into a buffer of the encoder), n the rows of the call (the resident store's for
 * search_resident_masked); row i is ALLOWED iff bit i & 31 of word i >> 5 is set; bits at or past n are ignored; one mask
 * serves all queries of the call.  The result is the unfiltered statement restricted to the allowed rows: per query the
 * first topk allowed rows by (adc_key(D), row index) ascending, D the sum above bit for bit; NaN sorts last and is reported
 * as 0x7FC00000; Euclidean reports sqrtf(D); slots past the allowed rows of a query with fewer than topk of them hold idx
 * 0xFFFFFFFF and dist +inf; topk keeps 1 .. min(n, 1024) whatever the mask.  All ones gives the unfiltered result bit for
 * bit, all zeros padding only.  A filtered call always takes the full pass (a sample of evenly spaced rows says nothing
 * about the allowed ones): its scan reads a wave's 64 rows' two mask words once, skips a wave without an allowed row and
 * computes, writes and counts allowed rows only; vqhip_pq_adc_last_redone reports nq after it.  A NULL pointer, the mask
 * among them, is VQHIP_ERR_NULL_PTR before the encoder is looked at; the other checks are the unfiltered calls'. */
int vqhip_pq_adc_search_masked(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, const float *queries, uint32_t nq,
                               uint32_t topk, const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_pq_adc_search_masked_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, const float *queries,
                                      uint32_t nq, uint32_t topk, const uint32_t *allowed, uint32_t *idx_out,
                                      float *dist_out);
int vqhip_pq_adc_search_resident_masked(vqhip_pq_encoder *enc, const float *queries, uint32_t nq, uint32_t topk,
                                        const uint32_t *allowed, uint32_t *idx_out, float *dist_out);

/* ---- exact k-NN search over resident rows, exact rerank (k_knn.hip) ------------------------
 * No reference counterpart (the crate has no search function).  An index holds n rows of d floats, given as f32
 * (dtype 0) or as f16 bits (dtype 1: the output of quantize / vqhip_pq_encode's f16_out, widened exactly to f32 before
 * any arithmetic), uploaded once (create_device copies).  Limits: 1 <= d, 1 <= n < 2^32, any of the five metrics.
 *   D(q, i) = vqhip_distance_batch(metric, q, row_i) bit for bit: each pair summed sequentially over t = 0..d-1 from
 *             -0.0f, no fused multiply-add; Euclidean = sqrtf of the squared sum; cosine through the EPSILON rule and
 *             the clamp (neither for VQHIP_COSINE_UNCLAMPED), the norms sqrtf(sum x_t^2) computed once per row (at
 *             create) and once per query (per call) -- a norm depends on its own vector only, no bit changes.
 *   search  = per query the topk rows by (D, row index) ascending, 1 <= topk <= min(n, 1024), in the order of the
 *             order-preserving key of the ADC search: NaN sorts last and is reported as 0x7FC00000, ties go to the
 *             lower row.  Unlike ADC, Euclidean orders by the REPORTED sqrtf value: two rows whose squared sums differ
 *             but round to the same root tie, and the lower row wins.
 *   rerank  = per query the topk (<= c) of its c candidate ids (1 <= c <= 4096, distinct within the query) under the
 *             same order.  An id >= n reads nothing; the device flags it and the call returns VQHIP_ERR_INVALID_INPUT.
 * queries [nq][d] f32, idx / dist [nq][topk].  Parameters are checked before any device work.  Host forms return
 * when the results are there; search_device is asynchronous on the current stream.  The handle has a lock like the
 * encoders' (one call at a time runs on it).  info: any output pointer may be NULL. */
typedef struct vqhip_flat vqhip_flat;
int vqhip_flat_create(const void *rows, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out);
int vqhip_flat_create_device(const void *dev_rows, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out);
int vqhip_flat_destroy(vqhip_flat *f);
int vqhip_flat_info(const vqhip_flat *f, uint64_t *n, uint32_t *d, int *dtype, int *metric);
int vqhip_flat_search(vqhip_flat *f, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                      float *dist_out);
int vqhip_flat_search_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                             void *dev_dist);
int vqhip_flat_rerank(vqhip_flat *f, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c,
                      uint32_t topk, uint32_t *idx_out, float *dist_out);

/* ---- binary index: Hamming top-k over packed BQ codes (k_binary.hip) -------------------------
 * No reference counterpart.  A BinaryQuantizer(threshold, low, high) fixes the bit rule; nothing else depends on it.
 *   bits    f32 x: x >= threshold (NaN -> 0, -0.0 == 0.0), the BQ encode rule; u8 code c: c >= high, the decode rule.
 *   layout  row i, dimension t in u32 word i * W + t / 32, bit t % 32 (LSB first), W = ceil(d / 32), pad bits zero,
 *           little-endian words: np.packbits(bits, bitorder="little") padded to 32 bits and viewed as "<u4".
 *   D(q, i) = Distance::compute(dequantize(quantize(q)), dequantize(code_i)) bit for bit, for squared Euclidean,
 *           Euclidean and Manhattan: with H = popcount(bits(q) xor bits(row_i)), a = f32(high) - f32(low) (an exact
 *           integer in 1..255) and t = a * a (squared / Euclidean) or a (Manhattan), the sequential sum is the table
 *           S(0) = +0.0, S(j) = fl(S(j - 1) + t) (an agreeing dimension adds +0.0, which changes no non-negative sum and
 *           turns the -0.0 start into +0.0), D = S(H), Euclidean sqrtf(S(H)).  Cosine: VQHIP_ERR_UNSUPPORTED.
 *   search  per query the topk rows by (D, row id) ascending, ties to the lower row, no NaN possible.  Every table is
 *           strictly increasing for a in 1..255 and d <= 8192, so the order is that of (H, row id).
 * Limits: 1 <= d <= 8192, 1 <= n < 2^32, 1 <= topk <= min(n, 1024), nq < 2^32 (internal batches of 1024).  The source
 * of create is f32 rows [n][d] (kind VQHIP_BINARY_F32), u8 codes [n][d] (VQHIP_BINARY_U8) or packed words [n][W]
 * (VQHIP_BINARY_PACKED: a set pad bit is VQHIP_ERR_INVALID_INPUT); create_device copies.  Queries are f32 [nq][d],
 * binarised on the device by the same rule.  Every parameter is checked before any device work.  Host forms return
 * when the results are there; search_device and bq_pack_device are asynchronous on the current stream.  One lock per
 * handle.  info: any output pointer may be NULL.  vqhip_binary_packed copies the words [n][W] to the host. */
#define VQHIP_BINARY_F32 0
#define VQHIP_BINARY_U8 1
#define VQHIP_BINARY_PACKED 2
#define VQHIP_BINARY_MAX_DIM 8192
#define VQHIP_BINARY_RANGE_BLOCK 8192 /* rows a workgroup of vqhip_binary_range_search counts and fills (k_bin_range) */
int vqhip_bq_pack(float threshold, const float *x, uint64_t n, uint32_t d, uint32_t *words);
int vqhip_bq_pack_device(float threshold, const void *dev_x, uint64_t n, uint32_t d, void *dev_words);
typedef struct vqhip_binary vqhip_binary;
int vqhip_binary_create(const void *src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high,
                        int metric, vqhip_binary **out);
int vqhip_binary_create_device(const void *dev_src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low,
                               uint32_t high, int metric, vqhip_binary **out);
int vqhip_binary_destroy(vqhip_binary *b);
int vqhip_binary_info(const vqhip_binary *b, uint64_t *n, uint32_t *d, float *threshold, uint32_t *low, uint32_t *high,
                      int *metric);
int vqhip_binary_packed(vqhip_binary *b, uint32_t *words);
int vqhip_binary_search(vqhip_binary *b, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                        float *dist_out);
int vqhip_binary_search_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                               void *dev_dist);

/* ---- scalar index: exact top-k over resident SQ codes (k_sqindex.hip) -------------------------
 * No reference counterpart.  An index is fixed by a ScalarQuantizer(min, max, levels), a metric (any of the five, as in
 * the flat index) and codes [n][d] u8, one byte per dimension, kept on the device; the f32 rows are never kept.  The
 * quantizer passes vqhip_sq_check first and its error text is reported unchanged.  Queries are f32 and never quantized.
 *   v(c)    = min + (float)c * step, step = (max - min) / (levels - 1): the SQ decode rule above, un-fused, for every
 *             byte value.  Codes >= levels are legal and decode by the same formula, as vqhip_sq_decode does.
 *   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit: the pair summed sequentially over t = 0..d-1 from -0.0f, one
 *             rounding per operation, no fused multiply-add; Euclidean = sqrtf of the sum; cosine through
 *             vq_cosine_finish, the row norm sqrtf(sum v^2) computed once at create and the query norm once per call.
 *   search / rerank = vqhip_flat_search / vqhip_flat_rerank over the rows vqhip_sq_decode gives for the codes: equal
 *             indices, distances equal as uint32 bits.  That is the order (key(D), row), NaN last and reported as
 *             0x7FC00000, ties to the lower row, Euclidean ordered by the reported root; a rerank id >= n is flagged on
 *             the device, never read, and gives VQHIP_ERR_INVALID_INPUT.
 *   A degenerate quantizer is no special case: (-3e38, 3e38, 2) has step = inf, v(0) = 0 * inf = NaN; such rows have NaN
 *   distances and sort last by row id.
 * Limits: 1 <= d, 1 <= n < 2^32, 1 <= topk <= min(n, 1024), nq < 2^32 (served in batches), rerank lists of 1..4096
 * distinct ids.  create / create_device take codes (host: uploaded once; device: copied, any alignment);
 * create_rows / create_rows_device take f32 rows [n][d] (device: 4-byte aligned) and encode them on the device with
 * the SQ encode rule, so that only the codes stay.  vqhip_sqindex_codes copies the codes [n][d] to the host.  Every
 * parameter is checked before any device work.  Host forms return when the results are there; search_device is
 * asynchronous on the current stream.  One lock per handle, as vqhip_flat's.  info: any output pointer may be NULL. */
typedef struct vqhip_sqindex vqhip_sqindex;
int vqhip_sqindex_create(float min, float max, uint32_t levels, const uint8_t *codes, uint64_t n, uint32_t d, int metric,
                         vqhip_sqindex **out);
int vqhip_sqindex_create_device(float min, float max, uint32_t levels, const void *dev_codes, uint64_t n, uint32_t d,
                                int metric, vqhip_sqindex **out);
int vqhip_sqindex_create_rows(float min, float max, uint32_t levels, const float *rows, uint64_t n, uint32_t d, int metric,
                              vqhip_sqindex **out);
int vqhip_sqindex_create_rows_device(float min, float max, uint32_t levels, const void *dev_rows, uint64_t n, uint32_t d,
                                     int metric, vqhip_sqindex **out);
int vqhip_sqindex_destroy(vqhip_sqindex *x);
int vqhip_sqindex_info(const vqhip_sqindex *x, uint64_t *n, uint32_t *d, int *metric, float *min, float *max,
                       uint32_t *levels);
int vqhip_sqindex_codes(vqhip_sqindex *x, uint8_t *codes);
int vqhip_sqindex_search(vqhip_sqindex *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                         float *dist_out);
int vqhip_sqindex_search_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                                void *dev_dist);
int vqhip_sqindex_rerank(vqhip_sqindex *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c,
                         uint32_t topk, uint32_t *idx_out, float *dist_out);

/* ---- exact range search over the flat and the scalar index (range.hpp) ------------------------
 * No reference counterpart.  (The inverted-file forms, vqhip_ivfflat_range_search and vqhip_ivfsq_range_search, are
 * declared with their indexes below and return the same vqhip_range, as do the Hamming-radius forms of the two binary
 * indexes, vqhip_binary_range_search and vqhip_ivfbin_range_search.)  Per query q with radius r_q (one f32 per query, radii [nq] in HOST memory in both forms):
 *   hit     row i is a hit iff D(q, i) <= r_q as an f32 comparison, D being the index's distance exactly as search
 *           reports it (the root for Euclidean, the finished value for cosine).  A NaN distance never hits; r_q = +inf
 *           returns every row whose distance is not NaN; a negative radius returns nothing except where D can be
 *           negative (VQHIP_COSINE_UNCLAMPED); -0.0 <= 0.0 holds (a float comparison, not one of keys).  A NaN radius
 *           is VQHIP_ERR_INVALID_INPUT.
 *   result  CSR, owned by a vqhip_range on the device: lims [nq + 1] u64 with lims[0] = 0, idx [total] u32 row ids and
 *           dist [total] f32 (the bits of D), total = lims[nq]; the hits of query q are idx / dist [lims[q], lims[q + 1]).
 *   order   within a query ascending row id: deterministic, no sort.  The same call on the same data returns identical
 *           arrays every time.  nq = 0 gives lims = [0].
 *   cap     max_results >= 1 (0: VQHIP_ERR_INVALID_INPUT) caps total.  A call that would exceed it returns
 *           VQHIP_ERR_UNSUPPORTED -- the message gives the count reached and the cap -- and *out stays NULL; the index
 *           is usable afterwards.
 * Checked in this order, before any device work: out, queries / radii (NULL with nq > 0), max_results, the radii, and
 * only then the index handle -- so every one of these checks runs without a device or an index.  dev_queries must be
 * 4-byte aligned.  Both forms return when the result is complete (the total decides the result's size, so the host
 * waits once per internal batch of queries -- the batches of search -- and once at the end); they take the index's lock
 * like search.  A vqhip_range is immutable: info / read / device may be called from any thread; read copies to host
 * arrays of nq + 1, total and total elements (any of the three may be NULL); device gives the device addresses, valid
 * until destroy. */
typedef struct vqhip_range vqhip_range;
int vqhip_flat_range_search(vqhip_flat *f, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                            vqhip_range **out);
int vqhip_flat_range_search_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, const float *radii,
                                   uint64_t max_results, vqhip_range **out);
int vqhip_sqindex_range_search(vqhip_sqindex *x, const float *queries, uint32_t nq, const float *radii,
                               uint64_t max_results, vqhip_range **out);
int vqhip_sqindex_range_search_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, const float *radii,
                                      uint64_t max_results, vqhip_range **out);
int vqhip_range_info(const vqhip_range *r, uint32_t *nq, uint64_t *total);
int vqhip_range_read(const vqhip_range *r, uint64_t *lims, uint32_t *idx, float *dist);
int vqhip_range_device(const vqhip_range *r, const void **dev_lims, const void **dev_idx, const void **dev_dist);
int vqhip_range_destroy(vqhip_range *r);

/* ---- filtered search: a row mask on the flat and the scalar index (knn_tile.hpp, topk.hpp, range.hpp) -------------
 * No reference counterpart.  A ROW MASK of an index of n rows is ceil(n / 32) u32 words; row i is ALLOWED iff bit i & 31
 * of word i >> 5 is set (a bool array through np.packbits(m, bitorder="little"), zero-padded to whole words and read as
 * little-endian u32).  Bits at or past n are ignored, whatever they hold: those of the last word, and any further words of
 * a longer mask, which are never read.  One mask serves all queries of a call.
 *   search_masked        per query the first topk words (adc_key(D) << 32) | row, ascending, over the ALLOWED rows only;
 *                        D is exactly the distance vqhip_flat_search / vqhip_sqindex_search report.  NaN distances of
 *                        allowed rows sort last and are reported as 0x7FC00000; ties go to the lower allowed row; a query
 *                        with fewer than topk allowed rows has the padding behind them, idx 0xFFFFFFFF and dist +inf (an
 *                        allowed row with a NaN distance is a result and comes before the padding).  topk keeps its
 *                        bound 1 .. min(n, 1024): the number of allowed rows does not bound it.
 *   range_search_masked  row i is a hit of query q iff it is allowed and D(q, i) <= radii[q] as an f32 comparison; the
 *                        CSR result, its order (ascending row id) and max_results are vqhip_flat_range_search's.
 * A mask of all ones gives the unmasked call's result bit for bit; a mask of all zeros gives padding only (lims = 0 for a
 * range search); the masked scalar index equals the masked flat index over the decoded rows.  A call without a mask (the
 * entry points above) runs the kernels it always ran.
 * allowed: HOST memory in the host forms (copied into a workspace of the handle), a 4-byte aligned DEVICE pointer in the
 * device forms (else VQHIP_ERR_INVALID_INPUT); NULL is VQHIP_ERR_NULL_PTR.  The other arguments, their checks and the
 * order of the checks are the unmasked siblings'; the mask's pointer is checked with the other pointers (range: behind
 * the radii, before the index handle), all before any device work.  A row tile of 64 rows without an allowed row costs
 * two mask words: no row is read and no distance computed. */
int vqhip_flat_search_masked(vqhip_flat *f, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                             uint32_t *idx_out, float *dist_out);
int vqhip_flat_search_masked_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, uint32_t topk,
                                    const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_sqindex_search_masked(vqhip_sqindex *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                                uint32_t *idx_out, float *dist_out);
int vqhip_sqindex_search_masked_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, uint32_t topk,
                                       const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_flat_range_search_masked(vqhip_flat *f, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   const uint32_t *allowed, vqhip_range **out);
int vqhip_flat_range_search_masked_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, const float *radii,
                                          uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out);
int vqhip_sqindex_range_search_masked(vqhip_sqindex *x, const float *queries, uint32_t nq, const float *radii,
                                      uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_sqindex_range_search_masked_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, const float *radii,
                                             uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out);

/* Hamming-radius range search over the binary index (k_binary.hip, k_bin_range; the result object and its rules are
 * vqhip_flat_range_search's).  The query is stated in bits: query q has a radius h_q, one u32 per query, hradii [nq] in
 * HOST memory in both forms, and row i is a hit iff H(q, i) <= h_q, H being exactly what vqhip_binary_search selects on
 * (the query binarised by the index's rule, pad bits zero).  Any u32 is accepted: h_q >= d returns every row, h_q = 0 the
 * exact bit matches.  dist holds the value search reports for the row, S[H] (sqrtf(S[H]) under Euclidean), as bits; the
 * table is strictly increasing, so the integer cut is exact and there is no float boundary.  Within a query ascending row
 * id; the same call returns identical arrays every time.  Checked in this order, before any device work: out, queries /
 * hradii (NULL with nq > 0), max_results, and only then the index handle.  Batches: 1024 queries, fewer where
 * nb * ceil(n / VQHIP_BINARY_RANGE_BLOCK) would pass 2^17 for nb > 1. */
int vqhip_binary_range_search(vqhip_binary *b, const float *queries, uint32_t nq, const uint32_t *hradii, uint64_t max_results,
                              vqhip_range **out);
int vqhip_binary_range_search_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, const uint32_t *hradii,
                                     uint64_t max_results, vqhip_range **out);

/* ---- filtered search on the binary index (k_binary.hip) ------------------------------------------------
 * No reference counterpart.  The ROW MASK is the flat index's (vqhip_flat_search_masked above): ceil(n / 32) u32 words,
 * row i ALLOWED iff bit i & 31 of word i >> 5 is set, bits at or past n ignored, one mask for all queries of a call.
 *   search_masked        per query the first topk of the allowed rows by (H, row id) ascending; dist is the value
 *                        vqhip_binary_search reports for the row, as bits.  topk keeps its bound 1 .. min(n, 1024) whatever
 *                        the mask; slots past the number of allowed rows hold idx 0xFFFFFFFF and dist +inf.
 *   range_search_masked  row i is a hit of query q iff it is allowed and H(q, i) <= h_q; the CSR result, its order
 *                        (ascending row id), max_results, nq = 0 and the statuses are vqhip_binary_range_search's.
 * A mask of all ones gives the unmasked call's result bit for bit; a mask of all zeros gives padding only (lims = 0 for a
 * range search).  A call without a mask (the entry points above) launches the kernels it always launched.
 * allowed: HOST memory in the host forms (copied into a workspace of the handle), a 4-byte aligned DEVICE pointer in the
 * device forms (else VQHIP_ERR_INVALID_INPUT); NULL is VQHIP_ERR_NULL_PTR.  The other arguments, their checks and the
 * order of the checks are the unmasked siblings'; the mask's pointer is checked with the other pointers (range: behind
 * the radii, before the index handle), all before any device work.  The mask is read inside the scans: the 64 rows a
 * wave takes at a time are two mask words, and a wave without an allowed row among them reads no row and no query word
 * and counts no bit. */
int vqhip_binary_search_masked(vqhip_binary *b, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                               uint32_t *idx_out, float *dist_out);
int vqhip_binary_search_masked_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_binary_range_search_masked(vqhip_binary *b, const float *queries, uint32_t nq, const uint32_t *hradii,
                                     uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_binary_range_search_masked_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, const uint32_t *hradii,
                                            uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out);
/* Rows per scan workgroup of vqhip_binary_search_masked over n rows and `groups` query groups of a batch (host only, no
 * device): a multiple of 64, so that a wave's 64 rows are two whole mask words, and at most 65472, so that no 16-bit half
 * of a workgroup's histogram carries.  Workgroup x scans rows [x * slice, min(n, (x + 1) * slice)). */
uint64_t vqhip_binary_masked_slice(uint64_t n, uint32_t groups);

/* ---- adding and removing rows: the flat, the scalar and the binary index (k_compact.hip, compact.hpp) ----
 * No reference counterpart.  An index is a sequence of rows R[0 .. n).
 *   add(B), b >= 1 rows   R' = R ++ B: the new rows get the ids n .. n + b - 1.  What is stored for a new row is exactly
 *                         what create stores for it: a flat index its bytes (in the index's own dtype), a scalar index its
 *                         codes as given (add_codes) or the codes of the SQ encode rule, made on the device as
 *                         vqhip_sqindex_create_rows makes them (add_rows), a binary index its packed bits from f32 rows, u8
 *                         codes or packed words (`kind`, as in vqhip_binary_create; the pad-bit check of create applies to
 *                         the added words, in the host and the device form).  Under the cosines the new rows' norms come
 *                         from the launcher create uses, run over the appended slice.  n + b must stay below 2^32, else
 *                         VQHIP_ERR_INVALID_INPUT.  n_add == 0 is VQHIP_OK and needs no device (only the handle is checked).
 *   remove(S)             S is a mask of ceil(n / 32) u32 words: row i is removed iff bit i & 31 of word i >> 5 is set, bits
 *                         at or past n ignored (the row mask's layout, with the other meaning).  R' is R without those rows,
 *                         the order kept: a surviving row i becomes row i - |{s in S : s < i}|.  *removed = the number of
 *                         rows removed.  Removing nothing changes nothing and allocates no payload (the host form does not
 *                         touch the device for it).  Removing every row is VQHIP_ERR_INVALID_INPUT, since an index holds at
 *                         least one row, and leaves the index as it was.
 * INVARIANT: after any sequence of adds and removes, every call on the index -- search, its masked form, range search and
 * its masked form, rerank, codes / packed, info -- returns bit for bit what a fresh index created from R' returns; the
 * bounds on topk and the length of a row mask follow the current n.
 * A call that fails (the allocation, the pad-bit check, the bound on n) leaves the index unchanged: the new buffer is
 * allocated first and swapped in behind the last step that can fail.
 * Threads and streams: these entry points take the handle's lock and order the caller's stream behind the handle's queued
 * work like every other call on it.  They may free the old payload, so they synchronise their stream before they free and
 * return synchronised: a search_device queued earlier on another stream completes on the old rows.  They allocate, so
 * they cannot be captured into a graph.
 * Memory: the payload grows geometrically -- a full buffer is replaced by one of max(needed, 1.5 x capacity) bytes -- so a
 * sequence of small adds copies O(total) bytes.  A removal compacts out of place into an allocation sized for the
 * survivors (peak: old + new) and frees the old buffer, which gives the memory back.
 * rows / codes / src / remove_words: HOST memory in the host forms, DEVICE pointers in the _device forms (f32 rows, packed
 * words and the remove mask 4-byte aligned, else VQHIP_ERR_INVALID_INPUT); NULL is VQHIP_ERR_NULL_PTR. */
int vqhip_flat_add(vqhip_flat *f, const void *rows, uint64_t n_add);
int vqhip_flat_add_device(vqhip_flat *f, const void *dev_rows, uint64_t n_add);
int vqhip_flat_remove(vqhip_flat *f, const uint32_t *remove_words, uint64_t *removed);
int vqhip_flat_remove_device(vqhip_flat *f, const uint32_t *dev_remove_words, uint64_t *removed);
int vqhip_sqindex_add_codes(vqhip_sqindex *x, const uint8_t *codes, uint64_t n_add);
int vqhip_sqindex_add_codes_device(vqhip_sqindex *x, const void *dev_codes, uint64_t n_add);
int vqhip_sqindex_add_rows(vqhip_sqindex *x, const float *rows, uint64_t n_add);
int vqhip_sqindex_add_rows_device(vqhip_sqindex *x, const void *dev_rows, uint64_t n_add);
int vqhip_sqindex_remove(vqhip_sqindex *x, const uint32_t *remove_words, uint64_t *removed);
int vqhip_sqindex_remove_device(vqhip_sqindex *x, const uint32_t *dev_remove_words, uint64_t *removed);
int vqhip_binary_add(vqhip_binary *b, const void *src, int kind, uint64_t n_add);
int vqhip_binary_add_device(vqhip_binary *b, const void *dev_src, int kind, uint64_t n_add);
int vqhip_binary_remove(vqhip_binary *b, const uint32_t *remove_words, uint64_t *removed);
int vqhip_binary_remove_device(vqhip_binary *b, const uint32_t *dev_remove_words, uint64_t *removed);

/* ---- asymmetric binary index: f32 queries over packed BQ bits, exact (k_abin.hip, bit_decode.hpp) -------
 * No reference counterpart.  The binary index above binarises the query and ranks by the Hamming distance.  This index
 * keeps the same bits and nothing else, leaves the query in f32 and computes its exact distance to the DEQUANTIZED row:
 * the third index of exact distances beside vqhip_flat and vqhip_sqindex, at d / 8 bytes a row (W words, plus 4 bytes
 * for the row norm under the cosines).
 *   bits    a BinaryQuantizer(threshold, low, high) fixes them on the way in, as vqhip_binary's: f32 x: x >= threshold
 *           (NaN -> 0, -0.0 == 0.0); u8 code c: c >= high.
 *   layout  vqhip_binary's: row i, dimension t in u32 word i * W + t / 32, bit t % 32 (LSB first), W = ceil(d / 32), pad
 *           bits zero.  vqhip_abin_packed gives exactly what vqhip_binary_packed gives for the same source.
 *   v(bit)  = bit ? (float)high : (float)low, the BQ decode rule, on the way out.
 *   D(q, i) = Distance::compute(q, v(bits[i])) bit for bit, for all five metrics, the cosines included: the pair summed
 *           sequentially over t = 0..d-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean = sqrtf
 *           of the sum; cosine through vq_cosine_finish, the row norm sqrtf of the sequential sum of v^2 computed once at
 *           create (and for the rows of an add) and the query norm once per call.  Queries are f32 and never quantized.
 *   search / rerank / range_search and their masked forms = vqhip_flat_* over the rows vqhip_bq_decode gives for the
 *           bits, and = vqhip_sqindex_* over the bits as 0/1 bytes under ScalarQuantizer(low, high, 2) (low + 1 * (high -
 *           low) is exact for u8 values): equal indices, distances equal as uint32 bits.  That is the order (key(D),
 *           row), NaN last and reported as 0x7FC00000, ties to the lower row; a masked query with fewer than topk allowed
 *           rows is padded with idx 0xFFFFFFFF and dist +inf; a rerank id >= n is flagged on the device, never read, and
 *           gives VQHIP_ERR_INVALID_INPUT.  Under a cosine with low = 0 a row without a set bit has norm 0 and takes
 *           vq_cosine_finish's EPSILON rule, as the same row does in the flat index.
 *   add / remove = the rules of "adding and removing rows" above: add takes create's three source kinds with create's
 *           checks; a removal moves the row norms with the rows and computes none anew.
 * Limits: 1 <= d <= 8192, 1 <= n < 2^32, 1 <= topk <= min(n, 1024), nq < 2^32 (served in batches), rerank lists of
 * 1..4096 distinct ids.  The source of create and add is f32 rows [n][d] (kind VQHIP_BINARY_F32), u8 codes [n][d]
 * (VQHIP_BINARY_U8) or packed words [n][W] (VQHIP_BINARY_PACKED: a set pad bit is VQHIP_ERR_INVALID_INPUT, in the host
 * and the device form); device f32 rows and words are 4-byte aligned, else VQHIP_ERR_INVALID_INPUT.  Every metric of the
 * flat index is accepted.  Every parameter is checked before any device work, in the order of the sibling entry points
 * of vqhip_sqindex.  Host forms return when the results are there; search_device is asynchronous on the current stream.
 * One lock per handle, as vqhip_flat's.  info: any output pointer may be NULL. */
typedef struct vqhip_abin vqhip_abin;
int vqhip_abin_create(const void *src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high,
                      int metric, vqhip_abin **out);
int vqhip_abin_create_device(const void *dev_src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low,
                             uint32_t high, int metric, vqhip_abin **out);
int vqhip_abin_destroy(vqhip_abin *x);
int vqhip_abin_info(const vqhip_abin *x, uint64_t *n, uint32_t *d, float *threshold, uint32_t *low, uint32_t *high,
                    int *metric);
int vqhip_abin_packed(vqhip_abin *x, uint32_t *words);
int vqhip_abin_search(vqhip_abin *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out);
int vqhip_abin_search_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                             void *dev_dist);
int vqhip_abin_search_masked(vqhip_abin *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                             uint32_t *idx_out, float *dist_out);
int vqhip_abin_search_masked_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, uint32_t topk,
                                    const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_abin_rerank(vqhip_abin *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk,
                      uint32_t *idx_out, float *dist_out);
int vqhip_abin_range_search(vqhip_abin *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                            vqhip_range **out);
int vqhip_abin_range_search_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, const float *radii,
                                   uint64_t max_results, vqhip_range **out);
int vqhip_abin_range_search_masked(vqhip_abin *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   const uint32_t *allowed, vqhip_range **out);
int vqhip_abin_range_search_masked_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, const float *radii,
                                          uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out);
int vqhip_abin_add(vqhip_abin *x, const void *src, int kind, uint64_t n_add);
int vqhip_abin_add_device(vqhip_abin *x, const void *dev_src, int kind, uint64_t n_add);
int vqhip_abin_remove(vqhip_abin *x, const uint32_t *remove_words, uint64_t *removed);
int vqhip_abin_remove_device(vqhip_abin *x, const uint32_t *dev_remove_words, uint64_t *removed);

/* ---- 4-bit scalar index: f32 queries over SQ codes packed eight to a word, exact (k_sq4index.hip, nibble_decode.hpp;
 * DESIGN.md 29) -------
 * No reference counterpart.  The scalar index above keeps one byte per dimension.  This index keeps the codes of a
 * ScalarQuantizer of at most 16 levels at four bits a dimension and nothing else, leaves the query in f32 and computes
 * its exact distance to the DEQUANTIZED row: the fourth index of exact distances beside vqhip_flat, vqhip_sqindex and
 * vqhip_abin, at d / 2 bytes a row (W words, plus 4 bytes for the row norm under the cosines).
 *   codes   a ScalarQuantizer(min, max, levels) with 2 <= levels <= 16 fixes them on the way in.  f32 rows go through
 *           the SQ encode (vqhip_sq_quantize's code of every value, bit for bit, < levels); u8 codes are taken as they
 *           are and must be <= 15.  Every nibble value 0..15 is legal, codes >= levels included, as every byte value is
 *           in vqhip_sqindex.
 *   layout  row i, dimension t in bits 4 (t % 8) .. 4 (t % 8) + 3 of u32 word i * W + t / 8 (dimension 8 j in the low
 *           nibble), W = ceil(d / 8), pad nibbles zero.  Rows are word-aligned.
 *   v(c)    = min + (float)c * step, step = (max - min) / (levels - 1): two roundings, never fused -- the decode of
 *           vqhip_sqindex, on the way out.
 *   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit, for all five metrics: the pair summed sequentially over
 *           t = 0..d-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean = sqrtf of the sum; cosine
 *           through vq_cosine_finish, the row norm sqrtf of the sequential sum of v^2 from -0.0f computed once at create
 *           (and for the rows of an add) and the query norm once per call.  Queries are f32 and never quantized.
 *   search / rerank / range_search and their masked forms = vqhip_sqindex_* over the same codes as bytes under the same
 *           quantizer, and = vqhip_flat_* over the rows v(codes): equal indices, distances equal as uint32 bits.  That is
 *           the order (key(D), row), NaN last and reported as 0x7FC00000, ties to the lower row; a masked query with
 *           fewer than topk allowed rows is padded with idx 0xFFFFFFFF and dist +inf; a rerank id >= n is flagged on the
 *           device, never read, and gives VQHIP_ERR_INVALID_INPUT.
 *   add / remove = the rules of "adding and removing rows" above: add takes create's three source kinds with create's
 *           checks, and a refused add leaves the index as it was; a removal moves the row norms with the rows.
 * Limits: vqhip_sqindex's -- d >= 1, 1 <= n < 2^32, 1 <= topk <= min(n, 1024), nq < 2^32 (served in batches), rerank
 * lists of 1..4096 distinct ids.  The source of create and add is f32 rows [n][d] (kind VQHIP_SQ4_F32), u8 codes [n][d]
 * (VQHIP_SQ4_U8) or packed words [n][W] (VQHIP_SQ4_PACKED).  VQHIP_ERR_INVALID_INPUT: levels > 16; a u8 code above 15; a
 * set pad nibble in packed words (both in the host and the device form: a host source is read before any device work, a
 * device source is checked behind the pack / the copy with a flag word read back); device f32 rows or words that are not
 * 4-byte aligned.  Every metric of the flat index is accepted.  Every parameter is checked before any device work, in the
 * order of vqhip_sqindex_create: out, the quantizer, levels <= 16, the source pointer, d, n, the metric, the kind, the
 * source.  Host forms return when the results are there; search_device is asynchronous on the current stream.  One lock
 * per handle, as vqhip_flat's.  packed: words [n][W].  info: any output pointer may be NULL. */
#define VQHIP_SQ4_F32 0
#define VQHIP_SQ4_U8 1
#define VQHIP_SQ4_PACKED 2
typedef struct vqhip_sq4index vqhip_sq4index;
int vqhip_sq4index_create(float min, float max, uint32_t levels, const void *src, int kind, uint64_t n, uint32_t d,
                          int metric, vqhip_sq4index **out);
int vqhip_sq4index_create_device(float min, float max, uint32_t levels, const void *dev_src, int kind, uint64_t n,
                                 uint32_t d, int metric, vqhip_sq4index **out);
int vqhip_sq4index_destroy(vqhip_sq4index *x);
int vqhip_sq4index_info(const vqhip_sq4index *x, uint64_t *n, uint32_t *d, int *metric, float *min, float *max,
                        uint32_t *levels);
int vqhip_sq4index_packed(vqhip_sq4index *x, uint32_t *words);
int vqhip_sq4index_search(vqhip_sq4index *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                          float *dist_out);
int vqhip_sq4index_search_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                                 void *dev_dist);
int vqhip_sq4index_search_masked(vqhip_sq4index *x, const float *queries, uint32_t nq, uint32_t topk,
                                 const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_sq4index_search_masked_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, uint32_t topk,
                                        const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_sq4index_rerank(vqhip_sq4index *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c,
                          uint32_t topk, uint32_t *idx_out, float *dist_out);
int vqhip_sq4index_range_search(vqhip_sq4index *x, const float *queries, uint32_t nq, const float *radii,
                                uint64_t max_results, vqhip_range **out);
int vqhip_sq4index_range_search_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, const float *radii,
                                       uint64_t max_results, vqhip_range **out);
int vqhip_sq4index_range_search_masked(vqhip_sq4index *x, const float *queries, uint32_t nq, const float *radii,
                                       uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_sq4index_range_search_masked_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, const float *radii,
                                              uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out);
int vqhip_sq4index_add(vqhip_sq4index *x, const void *src, int kind, uint64_t n_add);
int vqhip_sq4index_add_device(vqhip_sq4index *x, const void *dev_src, int kind, uint64_t n_add);
int vqhip_sq4index_remove(vqhip_sq4index *x, const uint32_t *remove_words, uint64_t *removed);
int vqhip_sq4index_remove_device(vqhip_sq4index *x, const uint32_t *dev_remove_words, uint64_t *removed);

/* ---- inverted-file PQ index: search only the probed lists (k_ivf.hip) -----------------------
 * No reference counterpart.  An index holds coarse centroids C [nlist][dim] f32 (1 <= nlist <= 65536), PQ codebooks
 * cb [m][k][sub_dim] (dim = m * sub_dim) and a metric: squared Euclidean, Euclidean or Manhattan (cosine is refused with
 * VQHIP_ERR_UNSUPPORTED, as ADC refuses it; m * k <= 38400, ADC's table limit).  add appends rows: row i (ids in add
 * order, n < 2^32 in all) gets a list id list[i] < nlist and codes[i][m] in the library's code width (one byte up to
 * k = 256, u16 above), both checked on the host.  Several adds equal one add of the concatenation.  Non-residual: the
 * codes encode the rows themselves, so the ADC tables are per query and a PQIndex's codes go into lists unchanged.
 *   P(q)    = the nprobe lists vqhip_flat_search over C (same metric) returns: Distance::compute bit for bit, ordered by
 *             (key, list id); Euclidean by the reported root, as in the flat index.  1 <= nprobe <= min(nlist, 1024).
 *   S(q)    = { i : list[i] in P(q) }.
 *   D(q, i) = the ADC definition (vqhip_pq_adc_search): per-subspace distance2 or L1 terms summed in subspace order, f32.
 *   search  = the topk rows of S(q) by (key(D), row id) ascending, 1 <= topk <= min(n, 1024): NaN sorts last and is
 *             reported as 0x7FC00000, ties go to the lower row, Euclidean orders by the squared sum and reports sqrtf.
 *             If |S(q)| < topk the remaining slots hold idx 0xFFFFFFFF and dist +inf, after every real row.
 *             With nprobe == nlist the result equals vqhip_pq_adc_search over the codes in row order, bit for bit.
 *             Run-to-run deterministic.
 * queries [nq][dim] f32, lists_out [nq][nprobe], idx / dist [nq][topk]; nq = 0 is a no-op.  create, add, info and
 * list_sizes (sizes [nlist]) are host-only, and every parameter is checked before any device work.  The index belongs to
 * the device current at create (when create sees no device: the one current at the first probe or search); the first
 * probe or search builds its device state there (the flat index over C, the rows in list order), the first one after an
 * add rebuilds it, and a call made with another device current returns VQHIP_ERR_INVALID_INPUT.  Host forms return when the results are there;
 * search_device takes device queries and results and is asynchronous on the current stream.  One lock per handle. */
typedef struct vqhip_ivfpq vqhip_ivfpq;
int vqhip_ivfpq_create(const float *coarse, uint32_t nlist, const float *codebooks, uint32_t m, uint32_t k,
                       uint32_t sub_dim, int metric, vqhip_ivfpq **out);
int vqhip_ivfpq_destroy(vqhip_ivfpq *ix);
int vqhip_ivfpq_add(vqhip_ivfpq *ix, const uint32_t *list_ids, const void *codes, uint64_t n);
int vqhip_ivfpq_info(const vqhip_ivfpq *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, uint32_t *m, uint32_t *k,
                     int *metric);
int vqhip_ivfpq_list_sizes(vqhip_ivfpq *ix, uint64_t *sizes);
int vqhip_ivfpq_probe(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out);
int vqhip_ivfpq_search(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                       uint32_t *idx_out, float *dist_out);
int vqhip_ivfpq_search_device(vqhip_ivfpq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                              void *dev_idx, void *dev_dist);

/* Residual lists (IVFADC): create_ex with flags = VQHIP_IVF_RESIDUAL (unknown bits: VQHIP_ERR_INVALID_INPUT, before any
 * device work; create is create_ex with flags 0).  The parts, the limits, P(q), S(q), the order, ties, NaN, Euclidean's
 * sqrtf and the padding are those above; the probe does not depend on the flag.  What changes: the codes of a row in
 * list l quantise x - C[l], so for i in list l
 *   r       = q - C[l], element by element in f32 (one rounding each),
 *   D(q, i) = the ADC definition at r in place of q: per subspace s, diff = r[t] - cb[s][j][t] for t ascending,
 *             accumulated from -0.0 (squared terms) or 0.0 (Manhattan, |diff|) with no contraction, the terms summed in
 *             subspace order in f32.
 * When every C[l] is the zero vector, r == q bit for bit (-0.0, inf and NaN included) and the result equals the
 * non-residual index's with the same codebooks and rows.  The device state also holds C; a search builds one table per
 * (query, probed list), batches of queries keep those under 256 MB (a batch of one query always runs).
 * vqhip_ivfpq_flags reports the flags given at create; add, probe, search, search_device, info, list_sizes and destroy
 * serve both kinds. */
#define VQHIP_IVF_RESIDUAL 1u
int vqhip_ivfpq_create_ex(const float *coarse, uint32_t nlist, const float *codebooks, uint32_t m, uint32_t k,
                          uint32_t sub_dim, int metric, uint32_t flags, vqhip_ivfpq **out);
int vqhip_ivfpq_flags(const vqhip_ivfpq *ix, uint32_t *flags);
/* Filtered search, plain and residual lists alike: the row mask, the view of the allowed rows and the rules
 * of vqhip_ivfflat_search_masked (below) over this index's D.  n is the rows in the index at the time of the call; probing
 * takes no mask; S_a(q) = { i in S(q) : i allowed }; per query the first topk of S_a(q) by (adc_key(D), row id), D the ADC
 * sum above bit for bit (a residual index: of its list's table); NaN last as 0x7FC00000; Euclidean reports sqrtf(D); slots
 * past |S_a(q)| hold idx 0xFFFFFFFF and dist +inf; topk keeps 1 .. min(n, 1024).  All ones equals the unmasked call bit for
 * bit; with nprobe == nlist a non-residual index equals vqhip_pq_adc_search_masked over the codes in add order, indices
 * and distance bits.  The scans read the codes of position j of the view at row pick[j] of the payload (64-bit offsets);
 * a probe slot without an allowed row gets no residual table.  Arguments, checks and statuses are
 * vqhip_ivfflat_search_masked[_device]'s: NULL (the mask included) is VQHIP_ERR_NULL_PTR and a device mask off 4-byte
 * alignment VQHIP_ERR_INVALID_INPUT, both before the handle is looked at. */
int vqhip_ivfpq_search_masked(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                              const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_ivfpq_search_masked_device(vqhip_ivfpq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                     const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);

/* ---- inverted-file flat index: exact distances over the probed lists (k_ivfflat.hip) ---------
 * No reference counterpart.  An index holds coarse centroids C [nlist][dim] f32 (1 <= nlist <= 65536), a metric (any of
 * the five: nothing is summed over subspaces, so the cosines are allowed) and a row dtype: 0 (f32) or 1 (the f16 bits
 * vqhip_quantize returns, widened exactly to f32 as the flat index widens them).  add appends rows: row i (ids in add
 * order, n < 2^32 in all) gets a list id list[i] < nlist, checked on the host before anything is stored, and row_i [dim].
 * Several adds equal one add of the concatenation.
 *   P(q)    = the nprobe lists vqhip_flat_search over C (same metric) returns, ordered by (key, list id).
 *             1 <= nprobe <= min(nlist, 1024).
 *   S(q)    = { i : list[i] in P(q) }.
 *   D(q, i) = the flat index's distance, Distance::compute(q, row_i) bit for bit: the pair summed sequentially over
 *             t = 0..dim-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean = sqrtf of the sum;
 *             cosine through vq_cosine_finish, the row norms (sequential chains) computed once per add's upload and the
 *             query norms once per call.
 *   search  = the topk rows of S(q) by (key(D), row id) ascending, 1 <= topk <= min(n, 1024): NaN sorts last and is
 *             reported as 0x7FC00000, ties go to the lower row, Euclidean orders by the reported root (as the flat index,
 *             unlike ADC).  If |S(q)| < topk the remaining slots hold idx 0xFFFFFFFF and dist +inf, after every real row.
 *             With nprobe == nlist the result equals vqhip_flat_search over the rows in add order: indices and distance
 *             bits.  Run-to-run deterministic.
 * queries [nq][dim] f32, lists_out [nq][nprobe], idx / dist [nq][topk]; nq = 0 is a no-op.  create, add, info and
 * list_sizes (sizes [nlist]) are host-only, and every parameter is checked before any device work.  The device
 * ownership rule is vqhip_ivfpq's: the index belongs to the device current at create (or, when create sees none, at the
 * first probe or search); the first probe or search builds its device state there (the flat index over C, the rows in
 * list order, uploaded through a bounded staging buffer), the first one after an add rebuilds it, and a call made with
 * another device current returns VQHIP_ERR_INVALID_INPUT.  Host forms return when the results are there; search_device
 * takes device queries and results and is asynchronous on the current stream.  Queries are served in batches of at most
 * 1024 whose distances stay under 1 GB (one query's when that alone is more).  One lock per handle.  info: any output
 * pointer may be NULL. */
typedef struct vqhip_ivfflat vqhip_ivfflat;
int vqhip_ivfflat_create(const float *coarse, uint32_t nlist, uint32_t dim, int dtype, int metric, vqhip_ivfflat **out);
int vqhip_ivfflat_destroy(vqhip_ivfflat *ix);
int vqhip_ivfflat_add(vqhip_ivfflat *ix, const uint32_t *list_ids, const void *rows, uint64_t n);
int vqhip_ivfflat_info(const vqhip_ivfflat *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *dtype, int *metric);
int vqhip_ivfflat_list_sizes(vqhip_ivfflat *ix, uint64_t *sizes);
int vqhip_ivfflat_probe(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out);
int vqhip_ivfflat_search(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                         uint32_t *idx_out, float *dist_out);
int vqhip_ivfflat_search_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                void *dev_idx, void *dev_dist);
/* Exact range search over the probed lists (ivf_range.hpp; the result object and its rules are vqhip_flat_range_search's,
 * above).  P(q), S(q) and D(q, i) are search's at the same nprobe; row i is a hit of query q iff i is in S(q) and
 * D(q, i) <= radii[q] as an f32 comparison (NaN never hits, +inf returns every non-NaN row of S(q), -0.0 <= 0.0 holds; a
 * NaN radius is VQHIP_ERR_INVALID_INPUT).  idx holds row ids, ascending within a query -- the positions of an inverted
 * file are not in row order, so the batch's hits go through a segmented stable radix sort by id -- and dist the bits of
 * D.  With nprobe == nlist the result equals vqhip_flat_range_search over the rows in add order: lims, idx and distance
 * bits.  Run-to-run deterministic.  nq = 0 gives lims = [0], an index without rows all-zero lims.  max_results as
 * above: past it VQHIP_ERR_UNSUPPORTED, *out NULL, the index usable.  Checked in this order before any device work: out,
 * queries / radii (NULL with nq > 0), max_results, the radii, the index handle, the alignment of dev_queries (4 bytes),
 * nprobe (search's rule).  radii [nq] is in HOST memory in both forms; both return when the result is complete (one
 * host wait per batch of search's batches), build or rebuild the device state as search does and take the index's
 * lock. */
int vqhip_ivfflat_range_search(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                               uint64_t max_results, vqhip_range **out);
int vqhip_ivfflat_range_search_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                      const float *radii, uint64_t max_results, vqhip_range **out);

/* ---- inverted-file scalar index: exact distances to SQ codes over the probed lists (k_ivfsq.hip) ---------
 * No reference counterpart.  vqhip_ivfflat with each row kept as one SQ byte per dimension.  An index is fixed by a
 * ScalarQuantizer(min, max, levels) -- the parameters go through vqhip_sq_check, whose status and text create reports
 * unchanged --, coarse centroids C [nlist][dim] f32 (1 <= nlist <= 65536), a metric (any of the five) and, per row i (ids
 * in add order, n < 2^32 in all), a list id list[i] < nlist and codes[i][dim] u8.  Several adds equal one add of the
 * concatenation.  With v(c) = min + (float)c * step as vqhip_sqindex's (un-fused, two roundings; every byte value is
 * legal, codes >= levels decode by the same formula):
 *   P(q)    = the nprobe lists vqhip_flat_search over C (same metric) returns, ordered by (key, list id): exactly
 *             vqhip_ivfflat_probe.  1 <= nprobe <= min(nlist, 1024).
 *   S(q)    = { i : list[i] in P(q) }.
 *   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit, in the flat index's arithmetic and order: the pair summed
 *             sequentially over t = 0..dim-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean =
 *             sqrtf of the sum; cosine through vq_cosine_finish, the row norms sqrtf(sum v^2) (sequential chains, as
 *             vqhip_sqindex's) computed once per add's upload and the query norms once per call.
 *   search  = the topk rows of S(q) by (key(D), row id) ascending, 1 <= topk <= min(n, 1024): NaN sorts last and is
 *             reported as 0x7FC00000, ties go to the lower row, Euclidean orders by the reported root.  If |S(q)| < topk
 *             the remaining slots hold idx 0xFFFFFFFF and dist +inf, after every real row.  Run-to-run deterministic.
 * Two identities follow.  (1) The index equals vqhip_ivfflat (dtype 0, same C and metric) over the rows vqhip_sq_decode
 * gives for the codes, in the same lists, for every nprobe and topk: indices, and distances as uint32 bits.  (2) With
 * nprobe == nlist it equals vqhip_sqindex_search over the codes in add order.  A degenerate quantizer is no special case:
 * (-3e38, 3e38, 2) has step = +inf, so v(0) = NaN and v(c > 0) = +inf, and those rows sort last by id.
 * add_codes takes host u8 codes [n][dim] and is host-only.  add_rows takes host f32 rows [n][dim], encodes them on the
 * device as vqhip_sq_encode does (the codes are equal) and keeps only the codes; it needs the device.  Both check every
 * list id on the host before anything is stored (VQHIP_ERR_INVALID_INPUT).  codes copies the codes out in add order
 * (codes_out [n][dim]; host-only).  info: any output pointer may be NULL.  queries [nq][dim] f32, lists_out
 * [nq][nprobe], idx / dist [nq][topk]; nq = 0 is a no-op; every parameter is checked before any device work.  Device
 * ownership, the lazy build of the device state (the flat index over C, the codes in list order in a buffer the index
 * owns, gathered through a bounded staging buffer) and its rebuild after an add, the batches (at most 1024 queries whose
 * distances stay under 1 GB, one query's when that alone is more), the two forms of search and the lock are
 * vqhip_ivfflat's.  The host keeps n * dim bytes, the device n * dim (+ 4 n under the cosines, + 4 n of row ids). */
typedef struct vqhip_ivfsq vqhip_ivfsq;
int vqhip_ivfsq_create(float min, float max, uint32_t levels, const float *coarse, uint32_t nlist, uint32_t dim, int metric,
                       vqhip_ivfsq **out);
int vqhip_ivfsq_destroy(vqhip_ivfsq *ix);
int vqhip_ivfsq_add_codes(vqhip_ivfsq *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n);
int vqhip_ivfsq_add_rows(vqhip_ivfsq *ix, const uint32_t *list_ids, const float *rows, uint64_t n);
int vqhip_ivfsq_info(const vqhip_ivfsq *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, float *min, float *max,
                     uint32_t *levels);
int vqhip_ivfsq_list_sizes(vqhip_ivfsq *ix, uint64_t *sizes);
int vqhip_ivfsq_codes(vqhip_ivfsq *ix, uint8_t *codes_out);
int vqhip_ivfsq_probe(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out);
int vqhip_ivfsq_search(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                       uint32_t *idx_out, float *dist_out);
int vqhip_ivfsq_search_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                              void *dev_idx, void *dev_dist);
/* vqhip_ivfflat_range_search over the decoded rows: the same stage behind this index's distances.  Two identities follow,
 * as for search: at every nprobe the result equals vqhip_ivfflat_range_search (dtype 0, same C and metric) over the rows
 * vqhip_sq_decode gives for the codes, in the same lists; with nprobe == nlist it equals vqhip_sqindex_range_search over
 * the codes in add order -- lims, idx and distance bits. */
int vqhip_ivfsq_range_search(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                             uint64_t max_results, vqhip_range **out);
int vqhip_ivfsq_range_search_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                    uint64_t max_results, vqhip_range **out);

/* ---- filtered search on the inverted-file flat and scalar index (ivf_view.hpp, ivf_tile.hpp) ------------------------
 * No reference counterpart.  The ROW MASK is the flat index's (vqhip_flat_search_masked above): ceil(n / 32) u32 words,
 * 4-byte aligned, n the rows in the index at the time of the call (it grows with every add); row i is ALLOWED iff bit
 * i & 31 of word i >> 5 is set; bits at or past n are ignored; one mask serves all queries of a call.
 *   probing              is unchanged: P(q) is the nprobe nearest lists, and vqhip_*_probe takes no mask (a list without an
 *                        allowed row is probed like any other), which keeps nprobe == nlist equal to the exact filtered search.
 *   searched set         S_a(q) = { i in S(q) : i allowed }.
 *   search_masked        per query the first topk of S_a(q) by (adc_key(D), row id) ascending; D is exactly what the
 *                        unmasked call reports.  Allowed rows with a NaN distance sort last, are reported as 0x7FC00000 and
 *                        come before the padding; slots past |S_a(q)| hold idx 0xFFFFFFFF and dist +inf.  topk keeps its
 *                        bound 1 .. min(n, 1024), whatever the mask.
 *   range_search_masked  row i is a hit of query q iff i is in S_a(q) and D(q, i) <= radii[q] as an f32 comparison; the CSR
 *                        result, its order (ascending row id within a query) and max_results are vqhip_ivfflat_range_search's.
 * Identities: a mask of all ones gives the unmasked call's result bit for bit; with nprobe == nlist the result equals
 * vqhip_flat_search_masked / vqhip_flat_range_search_masked (vqhip_sqindex_* for the scalar index) over the rows in add
 * order under the same mask, indices and distance bits; at every nprobe the masked scalar index equals the masked flat
 * index (dtype 0) over the rows vqhip_sq_decode gives for the codes; a mask of all zeros gives padding only (lims = 0 for
 * a range search).  A call without a mask (the entry points above) launches the kernels it always launched.
 * allowed: HOST memory in the host forms (copied into a workspace of the handle), a 4-byte aligned DEVICE pointer in the
 * device forms (else VQHIP_ERR_INVALID_INPUT); NULL is VQHIP_ERR_NULL_PTR, reported with the other pointers (range: behind
 * the radii, before the index handle) and before any device is touched.  The other arguments, their checks and the order
 * of the checks are the unmasked siblings'.  A filtered call builds, once, the inverted file of its allowed rows on the
 * device (8 bytes per row of workspace on the handle) and searches that: work behind the probe is proportional to the
 * allowed rows of the probed lists.  vqhip_ivfbin (below) and vqhip_ivfpq (above) take the same
 * view. */
int vqhip_ivfflat_search_masked(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_ivfflat_search_masked_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                       const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_ivfflat_range_search_masked(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                      uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_ivfflat_range_search_masked_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                             const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                             vqhip_range **out);
int vqhip_ivfsq_search_masked(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                              const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_ivfsq_search_masked_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                     const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_ivfsq_range_search_masked(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                    uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_ivfsq_range_search_masked_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                           const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                           vqhip_range **out);

/* ---- inverted-file 4-bit scalar index: exact distances to packed 4-bit SQ codes over the probed lists (k_ivfsq4.hip;
 * DESIGN.md 30) ---------
 * No reference counterpart.  vqhip_ivfsq with each row kept as vqhip_sq4index keeps it: four bits a dimension, eight
 * dimensions a word.  An index is fixed by a ScalarQuantizer(min, max, levels) with 2 <= levels <= 16 -- the parameters go
 * through vqhip_sq_check, whose status and text create reports unchanged, and behind it levels > 16 is
 * VQHIP_ERR_INVALID_INPUT with vqhip_sq4index_create's text --, coarse centroids C [nlist][dim] f32 (1 <= nlist <= 65536), a
 * metric (any of the five) and, per row i (ids in add order, n < 2^32 in all), a list id list[i] < nlist and dim four-bit
 * codes.  Several adds equal one add of the concatenation.
 *   layout  vqhip_sq4index's: dimension t of row i is bits 4 (t % 8) .. + 3 of u32 word i * W + t / 8, W = ceil(dim / 8);
 *           pad nibbles (dimensions >= dim of the last word) are zero.
 *   decode  v(c) = min + (float)c * step, un-fused, two roundings, for every nibble value 0 .. 15: codes >= levels are
 *           legal and decode by the same formula.
 *   P(q)    = exactly vqhip_ivfflat_probe over C under the same metric.  1 <= nprobe <= min(nlist, 1024).
 *   S(q)    = { i : list[i] in P(q) }.
 *   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit, in the flat index's arithmetic and order (vqhip_ivfsq's D);
 *             under the cosines the row norms are vqhip_sq4index's, computed once per upload of the rows.
 *   search  = vqhip_ivfsq_search's: the topk rows of S(q) by (key(D), row id) ascending, 1 <= topk <= min(n, 1024), NaN
 *             last as 0x7FC00000, padding idx 0xFFFFFFFF / dist +inf behind every real row.  Run-to-run deterministic.
 * Identities, each for indices and for distances as uint32 bits, for search, search_masked, range_search and
 * range_search_masked at every nprobe and topk: (1) the index equals vqhip_ivfsq over the same codes, one byte each, in the
 * same lists; (2) it equals vqhip_ivfflat (dtype 0) over the rows vqhip_sq_decode gives for the codes, in the same lists; (3)
 * with nprobe == nlist it equals vqhip_sq4index over the codes in add order on the same call; (4) after any sequence of
 * adds and removes it equals a fresh index given the remaining rows in one add ("removing rows from an inverted file"
 * below), a current device state staying current.
 * add_codes takes host u8 codes [n][dim], each <= 15, and packs them on the host; add_packed takes host words [n][W]
 * with every pad nibble zero; both are host-only.  add_rows takes host f32 rows [n][dim], encodes them on the device as
 * vqhip_sq_encode does and packs them there (vqhip_sq4index's path for f32 rows), and keeps only the words; it is the one
 * add that needs the device.  All three check every list id, then every code / pad nibble, on the host before anything is
 * stored (VQHIP_ERR_INVALID_INPUT): a refused add leaves the index as it was.  codes copies the codes out unpacked
 * (codes_out [n][dim] u8), packed copies the words (words_out [n][W]), both in add order and host-only.  info: any output
 * pointer may be NULL.  The other entry points -- list_sizes, probe, search, search_device, the two range searches, the
 * four masked forms (the ROW MASK of "filtered search on the inverted-file flat and scalar index" above), remove, uploads,
 * destroy -- have vqhip_ivfsq's signatures, checks, order of checks, device ownership, batches and lock.  The host keeps
 * 4 n W bytes, the device 4 n W (+ 4 n under the cosines, + 4 n of row ids): half of vqhip_ivfsq's for dim % 8 == 0. */
typedef struct vqhip_ivfsq4 vqhip_ivfsq4;
int vqhip_ivfsq4_create(float min, float max, uint32_t levels, const float *coarse, uint32_t nlist, uint32_t dim, int metric,
                        vqhip_ivfsq4 **out);
int vqhip_ivfsq4_destroy(vqhip_ivfsq4 *ix);
int vqhip_ivfsq4_add_codes(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n);
int vqhip_ivfsq4_add_packed(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const uint32_t *words, uint64_t n);
int vqhip_ivfsq4_add_rows(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const float *rows, uint64_t n);
int vqhip_ivfsq4_info(const vqhip_ivfsq4 *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, float *min, float *max,
                      uint32_t *levels);
int vqhip_ivfsq4_list_sizes(vqhip_ivfsq4 *ix, uint64_t *sizes);
int vqhip_ivfsq4_codes(vqhip_ivfsq4 *ix, uint8_t *codes_out);
int vqhip_ivfsq4_packed(vqhip_ivfsq4 *ix, uint32_t *words_out);
int vqhip_ivfsq4_probe(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out);
int vqhip_ivfsq4_search(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                        uint32_t *idx_out, float *dist_out);
int vqhip_ivfsq4_search_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               void *dev_idx, void *dev_dist);
int vqhip_ivfsq4_range_search(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                              uint64_t max_results, vqhip_range **out);
int vqhip_ivfsq4_range_search_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                     const float *radii, uint64_t max_results, vqhip_range **out);
int vqhip_ivfsq4_search_masked(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_ivfsq4_search_masked_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_ivfsq4_range_search_masked(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                     uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_ivfsq4_range_search_masked_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                            const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                            vqhip_range **out);
int vqhip_ivfsq4_remove(vqhip_ivfsq4 *ix, const uint32_t *remove_words, uint64_t *removed);
int vqhip_ivfsq4_uploads(const vqhip_ivfsq4 *ix, uint64_t *uploads);

/* ---- inverted-file binary index: Hamming top-k over packed BQ bits in the probed lists (k_ivfbin.hip) ---------
 * No reference counterpart.  vqhip_ivfflat's probe and schedule over vqhip_binary's codes.  An index is fixed by a
 * BinaryQuantizer(threshold, low, high) -- the parameters go through vqhip_bq_check, whose status and text create reports
 * unchanged --, coarse centroids C [nlist][dim] f32 (1 <= nlist <= 65536, 1 <= dim <= 8192), two metrics and, per row i
 * (ids in add order, n < 2^32 in all), a list id list[i] < nlist and words[i][W] u32, W = ceil(dim / 32), in
 * vqhip_binary's layout: dimension t in word t / 32, bit t % 32, pad bits zero.  The bit of an f32 element (rows and
 * queries) is x >= threshold (NaN gives 0, -0.0 equals 0.0), of a u8 code c >= high.
 *   metric        of the reported distance: squared Euclidean, Euclidean or Manhattan; the cosines are refused exactly
 *                 as vqhip_binary_create refuses them (VQHIP_ERR_UNSUPPORTED, the same text).
 *   coarse_metric of the probe (and, above this ABI, of the assignment of rows to lists): any of the five.
 *   P(q)    = the nprobe lists vqhip_flat_search over C under coarse_metric returns for the f32 query -- the query is
 *             never binarised for probing: exactly vqhip_ivfflat_probe of an index over (C, coarse_metric).
 *             1 <= nprobe <= min(nlist, 1024).
 *   S(q)    = { i : list[i] in P(q) }.
 *   H(q, i) = popcount(bits(q) xor words[i]).
 *   D(q, i) = vqhip_binary's reported distance for H: S[H] of the sequential f32 table (S[0] = +0.0, S[j] = S[j - 1] + t,
 *             t = (high - low)^2, or high - low under Manhattan), sqrtf(S[H]) under Euclidean: Distance::compute of the two
 *             dequantized vectors bit for bit.
 *   search  = the topk rows of S(q) by (D, row id) ascending, which is (H, row id): the table and its root are strictly
 *             increasing.  Ties go to the lower row.  1 <= topk <= min(n, 1024).  If |S(q)| < topk the remaining slots
 *             hold idx 0xFFFFFFFF and dist +inf, after every real row.  Run-to-run deterministic.
 * Identity: with nprobe == nlist the result equals vqhip_binary_search over the words in add order (same quantizer and
 * metric), indices and distance bits.
 * add_packed takes host words [n][W] and is host-only; a set pad bit is refused with vqhip_binary_create's status and
 * text (VQHIP_ERR_INVALID_INPUT, "row %llu has a pad bit set", the row counted within the call).  add_codes takes host
 * u8 codes [n][dim], packs them on the host with c >= high and is host-only.  add_rows takes host f32 rows [n][dim] and
 * packs them on the device as vqhip_bq_pack does with this threshold; it is the one add that needs the device.  All three
 * check every list id on the host before anything is stored; several adds equal one add of the concatenation.  packed
 * copies the words out in add order (words_out [n][W]; host-only).  info: any output pointer may be NULL.  queries
 * [nq][dim] f32, lists_out [nq][nprobe], idx / dist [nq][topk]; nq = 0 is a no-op; every parameter is checked before any
 * device work.  Device ownership, the lazy build of the device state (the flat index over C, off, ids ascending within a
 * list, the words in list order in a buffer the index owns) and its rebuild after an add, the batches, the two forms of
 * search and the lock are vqhip_ivfflat's.  The host keeps 4 n W bytes, the device 4 n W + 4 n of row ids. */
typedef struct vqhip_ivfbin vqhip_ivfbin;
int vqhip_ivfbin_create(float threshold, uint32_t low, uint32_t high, const float *coarse, uint32_t nlist, uint32_t dim,
                        int metric, int coarse_metric, vqhip_ivfbin **out);
int vqhip_ivfbin_destroy(vqhip_ivfbin *ix);
int vqhip_ivfbin_add_packed(vqhip_ivfbin *ix, const uint32_t *list_ids, const uint32_t *words, uint64_t n);
int vqhip_ivfbin_add_codes(vqhip_ivfbin *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n);
int vqhip_ivfbin_add_rows(vqhip_ivfbin *ix, const uint32_t *list_ids, const float *rows, uint64_t n);
int vqhip_ivfbin_info(const vqhip_ivfbin *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, int *coarse_metric,
                      float *threshold, uint32_t *low, uint32_t *high);
int vqhip_ivfbin_list_sizes(vqhip_ivfbin *ix, uint64_t *sizes);
int vqhip_ivfbin_packed(vqhip_ivfbin *ix, uint32_t *words_out);
int vqhip_ivfbin_probe(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out);
int vqhip_ivfbin_search(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                        uint32_t *idx_out, float *dist_out);
int vqhip_ivfbin_search_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               void *dev_idx, void *dev_dist);
/* Hamming-radius range search over the probed lists: row i is a hit of query q iff list[i] is in P(q) and H(q, i) <= h_q
 * (hradii [nq] u32 in HOST memory, any value; the rules of vqhip_binary_range_search), the result and its order those of
 * vqhip_ivfflat_range_search.  The stage behind the distances is that call's: the host hands it the f32 radius
 * reported[min(h_q, dim)] of the index's table, and D <= that radius iff H <= h_q because the reported table is strictly
 * increasing.  With nprobe == nlist the result equals vqhip_binary_range_search over the words in add order: lims, idx
 * and distance bits.  The checks run in vqhip_ivfflat_range_search's order; an index without rows gives empty ranges. */
int vqhip_ivfbin_range_search(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, const uint32_t *hradii,
                              uint64_t max_results, vqhip_range **out);
int vqhip_ivfbin_range_search_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                     const uint32_t *hradii, uint64_t max_results, vqhip_range **out);
/* Filtered search: vqhip_ivfflat_search_masked's mask, view and rules over this index's H and D.  n is the
 * rows in the index at the time of the call; probing is unchanged; S_a(q) = { i in S(q) : i allowed }.
 *   search_masked        per query the first topk of S_a(q) by (H, row id); dist as vqhip_ivfbin_search reports it;
 *                        slots past |S_a(q)| hold idx 0xFFFFFFFF and dist +inf; topk keeps 1 .. min(n, 1024).
 *   range_search_masked  row i is a hit of query q iff i is in S_a(q) and H(q, i) <= h_q; result, order, max_results and
 *                        statuses are vqhip_ivfbin_range_search's; a mask on an index without rows gives empty ranges.
 * Identities: all ones equals the unmasked call bit for bit; all zeros gives padding only (lims = 0); with nprobe == nlist
 * the result equals vqhip_binary_search_masked / vqhip_binary_range_search_masked over the words in add order under the
 * same mask.  allowed: as vqhip_ivfflat_search_masked takes it (NULL: VQHIP_ERR_NULL_PTR; a device mask that is not
 * 4-byte aligned: VQHIP_ERR_INVALID_INPUT, both before the handle is looked at). */
int vqhip_ivfbin_search_masked(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               const uint32_t *allowed, uint32_t *idx_out, float *dist_out);
int vqhip_ivfbin_search_masked_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist);
int vqhip_ivfbin_range_search_masked(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe,
                                     const uint32_t *hradii, uint64_t max_results, const uint32_t *allowed, vqhip_range **out);
int vqhip_ivfbin_range_search_masked_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                            const uint32_t *hradii, uint64_t max_results, const uint32_t *dev_allowed,
                                            vqhip_range **out);

/* ---- removing rows from an inverted file (k_ivf_remove.hip, ivf_remove.hpp, ivf_view.hpp) ----------------
 * No reference counterpart.  An index is the sequence of its rows R[0 .. n) with their list ids L[0 .. n).
 *   remove(S)   S is a HOST mask of ceil(n / 32) u32 words: row i is removed iff bit i & 31 of word i >> 5 is set, bits at
 *               or past n ignored (vqhip_flat_remove's layout).  R', L' are R, L without those rows, the order kept: a
 *               surviving row i becomes row i - |{s in S : s < i}|, in the list it was in.  *removed = the number of rows
 *               removed.  Removing nothing changes nothing.  Removing every row is allowed, unlike on the resident
 *               indexes: an inverted file may be empty, as a created one is, and later adds work.
 * INVARIANT: after any sequence of adds and removes, every call on the index -- probe, search, search_device, the masked
 * forms, range search and its masked forms, list_sizes, codes / packed, info -- returns bit for bit what a fresh index
 * returns that was given L', R' in one add; the bounds on topk and the length of a row mask follow the current n.
 * A call that fails leaves the index exactly as it was: everything that can fail runs before anything is swapped in.
 * Where the work is done: without a current device state (no probe or search yet, or an add since the last one) the host
 * rows are compacted in place and no device is touched, so a removal, like an add, works on a machine without a GPU.  With
 * a current device state the removal runs on the device and the state STAYS current: the next search pays no upload
 * (vqhip_*_uploads does not move).  The device state after it is byte for byte the one the first search of the fresh
 * index would upload.  Peak device memory: old + new payload.
 * There is no device-mask form: a handle keeps a host twin of every row (it is what an add rebuilds the device state
 * from), and compacting the twin needs the mask on the host.
 * Threads and streams: as vqhip_flat_remove -- the handle's lock, the caller's stream ordered behind the handle's queued
 * work, synchronised before an old buffer is freed and on return: a search_device queued earlier on another stream
 * completes on the old rows.  Not capturable into a graph.
 * NULL ix, remove_words or removed: VQHIP_ERR_NULL_PTR, before anything else happens.
 *   uploads     *uploads = the times the device state has been built from the host rows since create (by the first probe or
 *               search, and by the first one after an add): whether the next search pays an upload.  Host only. */
int vqhip_ivfpq_remove(vqhip_ivfpq *ix, const uint32_t *remove_words, uint64_t *removed);
int vqhip_ivfflat_remove(vqhip_ivfflat *ix, const uint32_t *remove_words, uint64_t *removed);
int vqhip_ivfsq_remove(vqhip_ivfsq *ix, const uint32_t *remove_words, uint64_t *removed);
int vqhip_ivfbin_remove(vqhip_ivfbin *ix, const uint32_t *remove_words, uint64_t *removed);
int vqhip_ivfpq_uploads(const vqhip_ivfpq *ix, uint64_t *uploads);
int vqhip_ivfflat_uploads(const vqhip_ivfflat *ix, uint64_t *uploads);
int vqhip_ivfsq_uploads(const vqhip_ivfsq *ix, uint64_t *uploads);
int vqhip_ivfbin_uploads(const vqhip_ivfbin *ix, uint64_t *uploads);

/* ---- TSVQ ----------------------------------------------------------------------------
 * build replaces TSVQNode::build (src/tsvq.rs:31-115); the tree comes back flattened in
 * pre-order (node 0 = root, left subtree, right subtree): centroids [cap][d], left/right
 * child index or -1.  cap must be >= min(2^(max_depth+1)-1, 2n-1). */
int vqhip_tsvq_build(const vqhip_dataset *ds, uint32_t max_depth, uint32_t cap, float *centroids,
                     int32_t *left, int32_t *right, int32_t *n_nodes);
/* encoder over a flattened tree; encode replaces find_leaf + quantize (tsvq.rs:117-132,
 * 239-255) for a batch: leaf [n] (optional) node index, f16_out [n][d] (optional) */
int vqhip_tsvq_create(const float *centroids, const int32_t *left, const int32_t *right,
                      uint32_t n_nodes, uint32_t d, int metric, vqhip_tsvq **out);
int vqhip_tsvq_destroy(vqhip_tsvq *t);
int vqhip_tsvq_encode(vqhip_tsvq *t, const float *rows, uint64_t n, int32_t *leaf,
                      uint16_t *f16_out);
int vqhip_tsvq_encode_device(vqhip_tsvq *t, const void *dev_rows, uint64_t n, void *dev_leaf,
                             void *dev_f16_out);
/* diagnostics of the last encode on this tree: *screened = 1 if the screened descent ran
 * (squared-L2 / Euclidean, d a multiple of 4 up to 1024), *undecided = rows
 * handed to the exact continuation.  Synchronises the stream. */
int vqhip_tsvq_last_stats(vqhip_tsvq *t, int *screened, uint64_t *undecided);

#ifdef __cplusplus
}
#endif
#endif /* VQHIP_H */
