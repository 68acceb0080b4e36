// kernels.hpp -- launch wrappers of the gfx950 kernels (implemented in k_*.hip).
// Every wrapper enqueues on `stream` and returns a vqhip status.
#pragma once

#include <hip/hip_ext.h>

#include <mutex>
#include <vector>

#include "common.hpp"

namespace vqhip {

// ---- code width --------------------------------------------------------------------
// A code is one byte per (row, subspace) while k <= 256 and a little-endian u16 above; every buffer the
// ABI types `uint8_t *codes` holds n*m*code_bytes(k) bytes. The width is a function of k alone so that no
// kernel needs an extra argument for it.
__host__ __device__ __forceinline__ uint32_t code_bytes(uint32_t k) { return k <= 256u ? 1u : 2u; }
__device__ __forceinline__ uint32_t load_code(const uint8_t *codes, size_t i, uint32_t k) {
    return k <= 256u ? (uint32_t)codes[i] : (uint32_t)reinterpret_cast<const uint16_t *>(codes)[i];
}
__device__ __forceinline__ void store_code(uint8_t *codes, size_t i, uint32_t j, uint32_t k) {
    if (k <= 256u) codes[i] = (uint8_t)j;
    else reinterpret_cast<uint16_t *>(codes)[i] = (uint16_t)j;
}
constexpr uint32_t kMaxCentroids = 65536;
constexpr uint32_t kX32MaxGroups = 16;  // centroid groups of the bf16 X32 screen at k > 256

// ---- prepared codebook ------------------------------------------------------------
// Device-side view of m codebooks of k centroids of sub_dim floats, plus what the
// assignment kernels derive from it once per codebook change.
struct CodebookView {
    uint32_t m = 0, k = 0, sd = 0;
    const float *cb = nullptr;       // [m][k][sd]
    // MFMA screen operands (null when the shape has no MFMA instantiation)
    uint32_t nt = 0, ks = 0;         // 16-centroid tiles (padded, power of two), k-steps = sd/4
    const float *prepA = nullptr;    // [m][nt][ks][64]   -2*c in MFMA A-operand lane order
    const float *prepCn = nullptr;   // [m][nt*16]        |c|^2 (padding = +inf)
    const float *meta = nullptr;     // [m][4]            {max|c|, margin coefficient, -, -}
    const float *cnsqrt = nullptr;   // [m][k]            sqrt(sum c^2) (cosine's norm_b)
    const uint32_t *prepA32 = nullptr;  // [m][ceil(k/32)][NMF][4][64] same, 32x32x16 MFMA lane order
    const uint32_t *prepA32_3 = nullptr;  // [m][8][2][4][64] the two rounded slices of -2(c - mu), once each; three products (sub_dim 16 encode), or null
    const float *cen = nullptr;      // [m][sd+4]  X32, L2: {mu[sd], max|c-mu|, margin coefficient, same for three products, -}
    const float *cn32 = nullptr;     // [m][ceil(k/32)*32]  X32, L2: |c-mu|^2, finite padding
};

// MFMA screen availability for a shape
bool screen_supported(uint32_t sd, uint32_t k);
void screen_tiling(uint32_t sd, uint32_t k, uint32_t *nt, uint32_t *ks);

// per-MFMA accumulation error (in units of 2^-24 (|C| + sum|ab|)) that the bf16 margin coefficients budget:
// >= kBf16ModelUlps = 18.1, the bound that follows from the bit-exact adder model (mfma_model.hpp)
constexpr float kBf16AssumedUlps = 20.0f;
// one-time device check that the hardware equals that model (k_selftest.hip); trusted = zero mismatches
int bf16_mfma_selftest(float *ratio32, float *ratio16, int *trusted);
// d[t] = one v_mfma_f32_32x32x16_bf16 of (a[t][0..16), b[t][0..16), c[t]); host buffers (diagnostics)
int mfma_bf16_probe(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d);
// software model of that instruction (mfma_model.hpp): on the host, and compared with the hardware on the device
void mfma_bf16_model_host(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d);
int mfma_bf16_model_check(uint64_t trials, uint64_t seed, uint64_t *mismatches, uint64_t *first_bad, uint64_t *fail_ids,
                          uint32_t fail_cap);
void mfma_bf16_model_case(uint64_t seed, uint64_t trial, uint16_t *a, uint16_t *b, float *c);

// bf16-split screen (k_screen_bf16.hip)
uint32_t x32_padded_sd(uint32_t sd);  // sub_dim of the X32 kernel serving `sd` (zero padding for 5..63), 0 = none
bool screen_bf16_x32_supported(uint32_t sd, uint32_t k);
bool screen_bf16_fused_update_supported(uint32_t sd, uint32_t k);
void screen_bf16_x32_tiling(uint32_t sd, uint32_t k, uint32_t *nt32_per_group, uint32_t *groups);
uint32_t screen_bf16_x32_mfmas(uint32_t sd);
bool screen_bf16_three_products_supported(uint32_t sd, uint32_t k);  // shapes with a three-product pipelined screen
int launch_prepare_bf16_x32(const CodebookView &v, uint32_t *prepA32, int cosine, float *cbc, float *cen,
                            float *cn32, hipStream_t stream, uint32_t *prepA32_3 = nullptr);

int launch_prepare_codebook(const CodebookView &v, float *prepA, float *prepCn, float *meta,
                            float *cnsqrt, hipStream_t stream);

// ---- assignment -------------------------------------------------------------------
// LDS row pitch of k_codes_transpose's [256][pitch] tile: a multiple of 4 above m that is never a multiple of 128
// bytes (m = 124: m + 4 would put every row's byte s into one bank, a 32-way conflict on the scatter)
__host__ __device__ constexpr uint32_t codes_transpose_pitch(uint32_t m) { return m + 4 + (((m + 4) % 128 == 0) ? 4u : 0u); }

// Events that the kernels of one stage of a pass carry in their own dispatch (hipExtLaunchKernelGGL): they are filled
// from the dispatch's completion signal.  A stop event adds nothing to the stream; a start event costs what a
// recorded one does, so a pass has at most one.
struct LaunchStage {
    hipEvent_t start = nullptr;  // bound by the stage's first kernel
    hipEvent_t stop = nullptr;   // bound by every kernel of the stage: its last kernel keeps it
    uint32_t launches = 0;
};

// hipLaunchKernelGGL for the launch sites of a pass: with a stage that holds an event the kernel carries it
template <class... P, class... A>
inline void vq_launch(LaunchStage *st, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                      A &&...args) {
    if (st && (st->start || st->stop)) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, st->start, st->stop, 0u, static_cast<P>(args)...);
        st->start = nullptr;
        ++st->launches;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<P>(args)...);
    }
}

struct AssignArgs {
    LaunchStage *stage = nullptr;  // the stage the next launch belongs to, or null
    const float *X = nullptr;  // [n][d]
    uint64_t n = 0;
    uint32_t d = 0;
    int metric = VQHIP_SQUARED_EUCLIDEAN;
    bool encode = false;  // an encode pass (no training behind it): may take the three-product screen
    const uint32_t *sub_list = nullptr;  // device [n_sub] subspace ids to process
    uint32_t n_sub = 0;
    uint8_t *codes = nullptr;  // [n][m]
    // optional scratch [m][codes_t_pitch] (pitch = n rounded up to 256): the single-pass bf16 screen writes a subspace's
    // codes contiguously there and a transposition forms [n][m] (byte stores m apart cost 15 x the code bytes in
    // write traffic at m = 96); nullptr = the screen writes [n][m] itself
    uint8_t *codes_t = nullptr;
    uint64_t codes_t_pitch = 0;
    // per-subspace work lists of rows needing the exact re-check (screen -> exact)
    uint32_t *wl_rows = nullptr;   // [m][wl_stride]
    uint32_t *wl_count = nullptr;  // [m]
    uint64_t wl_stride = 0;
    // segmented form (wave-private segments, no atomics): wl_seg [m][n_seg][2] = {first slot, count};
    // a screen launch that uses it sets n_seg (> 0) for the re-check launch that follows
    uint32_t *wl_seg = nullptr;
    uint32_t wl_seg_cap = 0;
    void *part = nullptr;            // grouped X32 screen: [m][G][n] uint4 partial verdicts
    mutable uint32_t n_seg = 0;
    mutable uint32_t products = 0;   // out (bf16 screen): bf16 products per dimension of the kernel that ran, 6 or 3
    // fused update (training, screen_bf16_fused_update_supported shapes): partial slabs [chunk][n_sub][k][sd] /
    // [chunk][n_sub][k] that the screen fills with the sums / counts of the rows it proves; it reports the chunks it
    // used (acc_chunk_cap = slabs available / n_sub)
    float *acc_sums = nullptr;
    uint32_t *acc_counts = nullptr;
    uint32_t acc_chunk_cap = 0;
    mutable uint32_t acc_chunks = 0;
    // vqhip_kmeans_run: device flags checked by the fused screen (active [m] bytes, *halt != 0 = run paused)
    const uint8_t *gate_active = nullptr;
    const uint32_t *gate_halt = nullptr;
};

// exact VALU scan of every centroid (reference op order); if use_worklist, only the rows
// listed per subspace in wl_rows/wl_count are processed
int launch_assign_exact(const CodebookView &cb, const AssignArgs &a, bool use_worklist,
                        hipStream_t stream);
// MFMA screen: writes a provisional code for every row and appends the rows whose winner is
// not provably the reference's to the work lists (wl_count must be zeroed before)
int launch_assign_screen(const CodebookView &cb, const AssignArgs &a, hipStream_t stream);
int launch_assign_screen_bf16(const CodebookView &cb, const AssignArgs &a, hipStream_t stream);

// out[i] = metric(a[i], b[i]) in the reference's arithmetic (Distance::compute)
int launch_distance_batch(int metric, const float *a, const float *b, uint64_t n, uint32_t d,
                          float *out, hipStream_t stream);

// ---- centroid update --------------------------------------------------------------
struct UpdatePlan {
    uint32_t m = 0, k = 0, sd = 0;
    uint32_t subs_per_chunk = 0;  // subspaces whose accumulators share one workgroup's LDS
    uint32_t k_range = 0;         // clusters per workgroup (= k unless k*(sd+2) words exceed the LDS)
    uint32_t n_k_ranges = 1;
    uint32_t n_sub_chunks = 0;
    uint32_t n_row_chunks = 0;
    uint32_t owned_waves = 0;     // > 0: wave-owned (atomic-free) accumulate, waves per workgroup = subspaces x row splits
    uint32_t owned_row_split = 1; // waves of a workgroup that share a subspace, each with its own part of the chunk's rows and its own slab
    size_t partial_floats = 0;    // per row chunk: m*k*sd sums
    size_t partial_counts = 0;    // per row chunk: m*k counts
};
int plan_update(uint32_t m, uint32_t k, uint32_t sd, uint64_t n, UpdatePlan *plan);

// true when launch_accumulate adds the rows with a wave-owned kernel (ascending row order inside a cluster, the same
// bits every run); the k-means update sends every other shape with k <= 16384 to launch_exact_sums
bool accumulate_owned(const UpdatePlan &p, const float *X, uint32_t d);
// per-workgroup LDS accumulation of sums/counts by code -> partial slabs
int launch_accumulate(const UpdatePlan &p, const float *X, uint64_t n, uint32_t d,
                      const uint8_t *codes, const uint8_t *active, float *partial_sums,
                      uint32_t *partial_counts, hipStream_t stream);
// the rows the screen handed to the exact re-check (segmented work lists), added into `n_patch` more partial slabs
// behind the `first_chunk` the fused screen filled; codes must already hold the re-check's answers
int launch_accumulate_listed(uint32_t m, uint32_t k, uint32_t sd, const float *X, uint32_t d, const uint8_t *codes,
                             const uint32_t *sub_list, uint32_t n_sub, const uint32_t *wl_rows, uint64_t wl_stride,
                             const uint32_t *wl_seg, uint32_t n_seg, uint32_t first_chunk, uint32_t n_patch,
                             float *partial_sums, uint32_t *partial_counts, hipStream_t stream, LaunchStage *stage = nullptr);
// fixed-order f64 combination of the fused path's slabs [chunk][position in the active list][k][sd]
int launch_reduce_partials_pos(uint32_t m, uint32_t k, uint32_t sd, const float *partial_sums, const uint32_t *partial_counts,
                               uint32_t n_chunks, uint32_t n_sub, const int32_t *sub_pos, double *slab, hipStream_t stream,
                               const uint8_t *gate_active = nullptr, const uint32_t *gate_halt = nullptr,
                               uint32_t *clear_changed = nullptr);  // device-driven run: also clears the iteration's `changed` flags [m]
// fixed-order f64 combination of the partial slabs -> slab [m][k][sd+1] (last = count)
int launch_reduce_partials(const UpdatePlan &p, const float *partial_sums,
                           const uint32_t *partial_counts, const uint8_t *active, double *slab,
                           hipStream_t stream);
// exact (reference-order) cluster sums: stable bucket by code + sequential f32 chains
int launch_exact_sums(uint32_t m, uint32_t k, uint32_t sd, const float *X, uint64_t n, uint32_t d,
                      const uint8_t *codes, const uint8_t *active, void *workspace,
                      size_t workspace_bytes, double *slab, hipStream_t stream);
size_t exact_sums_workspace_bytes(uint32_t m, uint32_t k, uint64_t n);
bool exact_sums_supported(uint32_t k);  // k <= 16384
// means + 1e-6 convergence test; exact_div: slab sums are f32-exact values -> f32 divide
int launch_finalize(uint32_t m, uint32_t k, uint32_t sd, const double *slab, const uint8_t *active,
                    float *centroids, uint32_t *counts, uint32_t *changed, int exact_div,
                    hipStream_t stream);
// the same + the end of one iteration of a device-driven run (vqhip_kmeans_run): retire converged subspaces, count the
// iteration, raise *halt on an empty cluster; `changed` must have been cleared by the gated launch_reduce_partials_pos
int launch_finalize_run(uint32_t m, uint32_t k, uint32_t sd, const double *slab, uint8_t *active, float *centroids,
                        uint32_t *counts, uint32_t *changed, uint32_t *halt, uint32_t *iters, uint32_t *done_blocks,
                        hipStream_t stream);
int launch_reduce_finalize_run(uint32_t m, uint32_t k, uint32_t sd, const float *partial_sums, const uint32_t *partial_counts,
                               uint32_t n_chunks, uint32_t n_sub, const int32_t *sub_pos, double *slab, uint8_t *active, float *centroids,
                               uint32_t *counts, uint32_t *changed, uint32_t *halt, uint32_t *iters, uint32_t *done_blocks,
                               uint32_t *chg_scratch, hipStream_t stream);
// centroids[s][j] = X[rows[s*k+j]][s*sd ..]
int launch_gather_rows(const float *X, uint32_t d, uint32_t m, uint32_t k, uint32_t sd,
                       const uint64_t *rows, float *centroids, hipStream_t stream);

// sharded init: bits of the owned rows among global ids `rows`, zero words elsewhere
int launch_gather_rows_owned(const float *X, uint32_t d, uint32_t m, uint32_t k, uint32_t sd, const uint64_t *rows,
                             uint64_t row_offset, uint64_t n_local, uint32_t *out_bits, hipStream_t stream);

// ---- RCCL (comm.hip): the exchange step of row-sharded training --------------------------
struct Comm;
int comm_unique_id(uint8_t *id128);
int comm_create(const uint8_t *id128, int world, int rank, Comm **out);  // id128 == NULL: one rank, no RCCL
int comm_adopt(void *nccl_comm, Comm **out);
void comm_info(const Comm *c, int *world, int *rank);
int comm_destroy(Comm *c);
int comm_allreduce_f64(Comm *c, double *buf, size_t count, hipStream_t stream);
int comm_allreduce_u32(Comm *c, uint32_t *buf, size_t count, hipStream_t stream);
// the ranks of one process (a host thread per GPU): a direct fixed-order exchange through peer access (comm.hip)
struct LocalGroup;
int local_group_create(int world, LocalGroup **out);
void local_group_destroy(LocalGroup *g);
int comm_create_local(LocalGroup *g, int rank, Comm **out);  // collective over the group's ranks, each on its own thread
void comm_abort(Comm *c, const char *text);  // poison an in-process group: blocked peers return at once (no-op otherwise)
void comm_abort_rccl(Comm *c);                 // ncclCommAbort on an owned communicator (one-process RCCL team's failure path)
int comm_kind(const Comm *c);                                // 0 identity, 1 RCCL, 2 in-process exchange

// ---- TSVQ -----------------------------------------------------------------------------
// build on a device-resident matrix; outputs are HOST arrays in pre-order (see vqhip.h)
// what k_fs_policy found out about a data set's columns (which blocks of 32 may take a sampled binade guess): a property
// of the rows, kept with a library-owned (immutable) data set from its first build on -- later builds skip the kernel
// and the host knows which of the two mean-pass chains have columns to work on
struct TsvqPolicyCache {
    std::mutex mu;
    bool valid = false;
    bool no_speculation = false;  // a build found levels mixing long and short nodes: launch both column-sum paths at once
    uint32_t n_cblk = 0;
    DevBuf dev;
    std::vector<uint32_t> host;
};
int tsvq_build_device(const float *X, uint64_t n, uint32_t d, uint32_t max_depth, uint32_t cap,
                      float *centroids_out, int32_t *left_out, int32_t *right_out, int32_t *n_nodes_out,
                      hipStream_t stream, TsvqPolicyCache *policy_cache = nullptr);
// latency path for a handful of rows (k_small.hip): rows / outputs are device-visible pinned host pointers
int launch_pq_encode_small(const float *rows_dev, uint32_t n, uint32_t d, uint32_t m, uint32_t k, uint32_t sd, int metric,
                           const float *cb, const float *cnsqrt, uint8_t *codes_dev, uint16_t *f16_dev,
                           hipStream_t stream);
// one Lloyd iteration of a small problem in two launches (k_lloyd_small.hip)
bool lloyd_small_supported(uint64_t n, uint32_t m, uint32_t k, uint32_t sd);
size_t lloyd_small_workspace(uint64_t n, uint32_t m, uint32_t k, uint32_t sd, size_t *cnt_bytes, size_t *flag_bytes);
int launch_lloyd_small(const float *X, uint64_t n, uint32_t d, uint32_t m, uint32_t k, uint32_t sd, float *cb, uint8_t *codes,
                       float *psum, uint32_t *pcnt, uint32_t *counts, uint32_t *changed, const uint8_t *active, uint32_t *run_flags,
                       uint32_t *run_iters, uint32_t it, hipStream_t stream);
void lloyd_small_run_result(uint32_t m, const uint8_t *start_active, const uint32_t *flags, const uint32_t *iters, bool *paused,
                            uint8_t *active_out, uint32_t *changed_out);
int launch_lloyd_small_slab(const float *X, uint64_t n, uint32_t d, uint32_t m, uint32_t k, uint32_t sd, const float *cb, uint8_t *codes,
                            float *psum, uint32_t *pcnt, const uint8_t *active, const uint32_t *gate_halt, uint32_t *changed, double *slab,
                            hipStream_t stream);
bool tsvq_small_supported(uint32_t d);
int launch_tsvq_encode_small(const float *rows_dev, uint32_t n, uint32_t d, int metric, const float *centroids,
                             const float *cnorm, const int32_t *left, const int32_t *right, int32_t *leaf_dev,
                             uint16_t *f16_dev, hipStream_t stream);

// asymmetric-distance search over stored codes (k_adc.hip)
int launch_adc_search(const float *cb, uint32_t m, uint32_t k, uint32_t sd, int metric, const uint8_t *codes, uint64_t n,
                      const float *queries_dev, uint32_t nq, uint32_t topk, float *lut_ws, float *dist_ws,
                      void *state_ws, unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev,
                      hipStream_t stream, uint32_t qgroup, const uint32_t *mask = nullptr);
uint32_t adc_query_batch();
uint32_t adc_query_group(uint64_t n, uint32_t nq);  // queries that go through one set of launches (a multiple of the batch, all nq, or fewer where 4 n passes 1 GB)
size_t adc_state_bytes(uint32_t qgroup);
// the selection stage's workspaces for a batch of qb queries (topk.hpp): its state hist | sel | cand_n, which every family's
// state workspace ends in (the IVF search's is nothing else), and the candidate words [qb][kAdcCand] of every search
size_t topk_state_bytes(uint32_t qb);
size_t topk_cand_bytes(uint32_t qb);
// VQHIP_ERR_UNSUPPORTED for a table above the LDS plan's limit (m * k > kAdcMaxTable, adc_plan.hpp): both schedules refuse it
int fail_adc_table(uint32_t m, uint32_t k);
// the threshold pass (one scan of the codes, candidates only): all queries in one set of launches; redo_dev[q] = 1 where
// query q has to be repeated through launch_adc_search
bool adc_fast_eligible(uint32_t m, uint32_t k, uint64_t n, uint32_t topk);
size_t adc_fast_lut_bytes(uint32_t m, uint32_t k, uint32_t nq);
size_t adc_fast_state_bytes(uint32_t m, uint32_t k, uint32_t nq);
size_t adc_fast_cand_bytes(uint32_t m, uint32_t k, uint32_t nq);
int launch_adc_search_fast(const float *cb, uint32_t m, uint32_t k, uint32_t sd, int metric, const uint8_t *codes, uint64_t n,
                           const float *queries_dev, uint32_t nq, uint32_t topk, float *lut_ws, void *state_ws,
                           unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *redo_dev,
                           hipStream_t stream);

// the ADC tables alone, k_adc_lut over nq queries (k_adc.hip): lut [nq][m][k], bounds [nq][2] scratch
int launch_adc_lut(const float *queries_dev, uint32_t nq, uint32_t m, uint32_t k, uint32_t sd, const float *cb, int metric,
                   float *lut, float *bounds, hipStream_t stream);
// inverted-file search over list-ordered PQ codes (k_ivf.hip): one batch of nb queries whose probe lists and tables are on
// the device; W [nb][wstride] (wstride >= every query's |S(q)|), pref [nb][nprobe + 1], seg [nb][nprobe], bounds [nb][2],
// state >= topk_state_bytes(nb), cand >= topk_cand_bytes(nb)
uint32_t ivf_chunk(uint64_t expected_positions);
int launch_ivf_search(const uint8_t *codes, const uint32_t *ids, const uint32_t *off, uint32_t nlist, uint32_t m, uint32_t k, int metric,
                      const float *lut, const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk,
                      uint64_t wstride, float *W, uint32_t *pref, uint32_t *seg, float *bounds, void *state,
                      unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream,
                      const uint32_t *pick = nullptr);
// the same over residual lists (a row of list l encodes x - C[l]): the tables per (query, probe slot) are built here from
// the queries, coarse [nlist][dim] and cb [m][k][sd]; tabs [nb][nprobe][m][k], mm [nb][nprobe][2]
size_t ivf_rtab_bytes(uint32_t qb, uint32_t nprobe, uint32_t m, uint32_t k);
size_t ivf_rmm_bytes(uint32_t qb, uint32_t nprobe);
uint32_t ivf_rchunk(uint64_t expected_positions, uint32_t k);
int launch_ivf_rsearch(const uint8_t *codes, const uint32_t *ids, const uint32_t *off, const float *coarse, uint32_t nlist,
                       const float *cb, uint32_t m, uint32_t k, uint32_t sd, int metric, const float *queries,
                       const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk, uint64_t wstride,
                       float *tabs, float *mm, float *W, uint32_t *pref, uint32_t *seg, float *bounds, void *state,
                       unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream,
                       const uint32_t *pick = nullptr);
// Inverted-file search over list-ordered rows, SQ codes or packed BQ words (k_ivfflat.hip, k_ivfsq.hip, k_ivfbin.hip).
// One batch of nb <= 1024 queries whose probe lists are on the device, as every stage of it sees it:
struct IvfBatchView {
    // the index in list order: list l holds the rows ids[off[l] .. off[l + 1]); n rows in all, max_list in the largest list
    const uint32_t *ids;
    uint64_t n;
    const uint32_t *off;
    uint32_t nlist;
    uint64_t max_list;
    // the batch: probe [nb][nprobe] (launch_knn_search), positions per item of the scan kernels, floats of W per query
    const uint32_t *probe;
    uint32_t nb, nprobe, chunk;
    uint64_t wstride;
    // its workspaces: W [nb][wstride] (wstride >= every query's |S(q)|), pref [nb][nprobe + 1], seg and inv [nb][nprobe],
    // lists >= ivfflat_lists_bytes(nlist), state >= knn_state_bytes(nb)
    float *W;
    uint32_t *pref, *seg, *inv, *lists;
    void *state;
    // a filtered call (ivf_view.hpp): ids and off above are the view's (the allowed rows only), and row j of the view is
    // row pick[j] of the payload in list order; NULL: every row, the payload as it lies.  Read by the distance passes of
    // the flat, the scalar and the binary index
    const uint32_t *pick = nullptr;
};
// The view of a filtered call on an inverted file: the inverted file of the allowed rows, built once per call on the
// device (ivf_view.hpp, instantiated in k_ivfflat.hip).  allowed: the call's row mask, ceil(n / 32) words; ids / off: the
// index in list order; pick / aids [n], aoff [nlist + 1], ws >= ivf_view_ws_bytes(n).  No atomics: the same call gives
// the same arrays on every run.  Enqueued on stream, no host round trip.
size_t ivf_view_ws_bytes(uint64_t n);
int launch_ivf_view(const uint32_t *allowed, const uint32_t *ids, uint64_t n, const uint32_t *off, uint32_t nlist, void *ws,
                    uint32_t *pick, uint32_t *aids, uint32_t *aoff, hipStream_t stream);
size_t ivfflat_lists_bytes(uint32_t nlist);
// The stages of a batch around its distance passes (k_ivfflat.hip), the same for the three indexes: plan = the batch's
// checks, the zeroed state, k_ivff_plan / _lists / _invert (topk: the selection's, 1 in front of a range stage); select
// = k_ivff_hist and the selection stage, results [nb][topk] on the device, cand >= topk_cand_bytes(nb).
// IvffPlan: the per-list counts and starts (in lists), the key range (in state) and the tile kernel's grid.
struct IvffPlan {
    const uint32_t *cnt, *lstart, *tstart;
    uint32_t *kmin, *kmax;
    void *topk_ws;             // the selection stage's state, behind kmin / kmax
    uint64_t tiles_max, cols;  // query tiles the batch can have; columns of row tiles per query tile (0: no tile kernel)
};
int launch_ivff_plan(const IvfBatchView &v, uint32_t topk, IvffPlan *p, hipStream_t stream);
int launch_ivff_select(const IvffPlan &p, const IvfBatchView &v, uint32_t topk, unsigned long long *cand, uint32_t *idx_out,
                       float *dist_out, hipStream_t stream);
// The two distance passes of a batch behind its plan, what an index has of its own: every D(q, i) of the probed lists
// into v.W, the key range into p.  queries [nb][d] f32, qnorm [nb] under the cosines; rows in list order:
//   ivfflat  X [n][d] f32 (dtype 0) or f16 bits (dtype 1), rnorm [n] under the cosines
//   ivfsq    C [n][d] u8, v(c) = mn + (float)c * step decoded on the fly, rnorm [n] from launch_sq_norms over C
//   ivfbin   P [n][bin_words(d)] and the batch's queries packed the same way (Q [nb][bin_words(d)], launch_bq_pack);
//            D = S[H], its root under VQHIP_EUCLIDEAN, S [d + 1] binary_table's on the device
int launch_ivfflat_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const void *X, int dtype, uint32_t d,
                             const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream);
int launch_ivfsq_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint8_t *C, uint32_t d, float mn, float step,
                           const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream);
//   ivfsq4   words [n][sq4_words(d)] u32, eight 4-bit codes a word (k_sq4index.hip's layout, pad nibbles zero), decoded as
//            ivfsq's; rnorm [n] from launch_sq4_norms over the words (k_ivfsq4.hip)
int launch_ivfsq4_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint32_t *words, uint32_t d, float mn,
                            float step, const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream);
int bin_load_width(const uint32_t *P, uint32_t W);
int launch_ivfbin_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint32_t *P, uint32_t d, const float *S,
                            const uint32_t *Q, hipStream_t stream);
// exact k-NN search over resident rows and exact rerank of candidate lists (k_knn.hip); X [n][d] f32 (dtype 0) or f16
// bits (dtype 1), rnorm [n] the rows' norms (cosine only, else unused)
// mask_dev (search and range, here and over SQ codes): the row mask of a filtered call on the device -- ceil(n / 32)
// words, row i allowed iff bit i & 31 of word i >> 5 is set -- or NULL for the unmasked kernels.
int launch_knn_norms(const void *X, int dtype, uint64_t n, uint32_t d, float *out, hipStream_t stream);
uint32_t knn_query_batch(uint64_t n, uint32_t nq);
size_t knn_state_bytes(uint32_t qb);
int launch_knn_search(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                      unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                      hipStream_t stream);
int launch_knn_rerank(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c, uint32_t topk,
                      uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream);

// exact range search (range.hpp behind k_knn.hip and k_sqindex.hip): per query every row with D <= its radius, in
// ascending row id.  The result, on the device: lims [nq + 1] u64 (lims[0] = 0), idx / dist [total] with room for cap.
struct RangeOut {
    DevBuf lims, idx, dist;
    uint32_t nq = 0;
    uint64_t total = 0, cap = 0;
};
// workspace of the range stage for batches of knn_query_batch(n, nq) queries
size_t range_ws_bytes(uint64_t n, uint32_t nq);
// an empty result for nq queries (range.hpp's range_begin): lims[0] = 0, room for min(kRangeInitCap, max_results) hits
int launch_range_begin(RangeOut *out, uint32_t nq, uint64_t max_results, hipStream_t stream);
// launch_knn_search's arguments with radii_dev [nq] f32 and max_results >= 1 in place of topk, range_ws >=
// range_ws_bytes(n, nq) in place of the candidates; state_ws is written (kmin / kmax) and not read.  Waits for the
// stream once per batch and once at the end: *out is complete on return.  More than max_results hits:
// VQHIP_ERR_UNSUPPORTED.
int launch_knn_range(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                     const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results, float *dist_ws,
                     void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream);
int launch_sq_range(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                    const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                    float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream);

// exact range search over the probed lists (ivf_range.hpp behind k_ivfflat.hip): the range stage in place of the
// selection behind a batch's distance passes, radii [nb] on the device (for the binary index the reported distance of each
// query's Hamming radius).  The batch's hits go into *out (begun by launch_range_begin) as queries q0 .. q0 + nb, in
// ascending row id per query; range_ws >= ivff_range_ws_bytes(wstride, nb); *stage: the staging areas, grown as needed.
// Waits for the stream once per batch.  More than max_results hits: VQHIP_ERR_UNSUPPORTED.
size_t ivff_range_ws_bytes(uint64_t wstride, uint32_t nb);
int launch_ivff_range(const IvfBatchView &v, uint32_t q0, const float *radii, void *range_ws, DevBuf *stage, uint64_t max_results,
                      RangeOut *out, hipStream_t stream);

// exact search and rerank over resident SQ codes (k_sqindex.hip): C [n][d] u8, v(c) = mn + (float)c * step decoded on
// the fly, rnorm [n] the decoded rows' norms (cosine only).  Batches and workspaces as launch_knn_search / _rerank; the
// query norms come from launch_knn_norms.
int launch_sq_norms(const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, float *out, hipStream_t stream);
int launch_sq_search(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                     unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                     hipStream_t stream);
int launch_sq_rerank(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                     uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream);

// exact search, range search and rerank of f32 queries over resident packed BQ bits (k_abin.hip): P [n][bin_words(d)]
// u32 in the binary index's layout, v(bit) = bit ? hi : lo decoded on the fly (lo / hi: the quantizer's low / high as
// floats), rnorm [n] the decoded rows' norms (cosine only).  Batches and workspaces as launch_knn_search / _range /
// _rerank; the query norms come from launch_knn_norms.
int launch_abin_norms(const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, float *out, hipStream_t stream);
int launch_abin_search(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                       const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                       unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                       hipStream_t stream);
int launch_abin_range(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                      float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream);
int launch_abin_rerank(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                       const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                       uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream);

// exact search, range search and rerank of f32 queries over resident 4-bit SQ codes (k_sq4index.hip): P [n][sq4_words(d)]
// u32, dimension t of a row in bits 4 (t % 8) .. + 3 of its word t / 8, v(c) = mn + (float)c * step decoded on the fly,
// rnorm [n] the decoded rows' norms (cosine only).  Batches and workspaces as launch_knn_search / _range / _rerank; the
// query norms come from launch_knn_norms.
uint32_t sq4_words(uint32_t d);
// C [n][d] u8 codes -> out [n][sq4_words(d)], pad nibbles zero; *bad |= 1 where a code is above 15 (the caller zeroes it)
int launch_sq4_pack(const uint8_t *C, uint64_t n, uint32_t d, uint32_t *out, uint32_t *bad, hipStream_t stream);
// *bad |= 1 where a packed row has a pad nibble set (the caller zeroes it first)
int launch_sq4_padcheck(const uint32_t *P, uint64_t n, uint32_t d, uint32_t *bad, hipStream_t stream);
int launch_sq4_norms(const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, float *out, hipStream_t stream);
int launch_sq4_search(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                      unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                      hipStream_t stream);
int launch_sq4_range(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                     float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream);
int launch_sq4_rerank(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                      uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream);

// prepared per-node data of the screened squared-L2 / Euclidean descent (k_tsvq_screen.hip)
struct TsvqScreen {
    const float *w = nullptr;     // [n_int][d]  c_left - c_right of every two-child node; cosine: [n_int][2][d] unit vectors of the children
    const int4 *info = nullptr;   // [n_int]     {code_l, code_r, bits(b), bits(|w|)}; code >= 0 slot, < 0 leaf -1-code; cosine: {.., .., bits(margin M, NaN = exact-only), 0}
    const int32_t *slot_node = nullptr;  // [n_int] node index of a slot
    const int32_t *node_slot = nullptr;  // [n_nodes] slot of a two-child node, -1 otherwise (the continuation's re-screen)
    int32_t start_slot = 0;       // slot the root resolves to
    const float *mu = nullptr;    // [d]         root centroid
    uint32_t n_int = 0, n_nodes = 0;  // n_int: slots resident in LDS (the levels nearest the root)
    uint32_t n_slots = 0;         // all two-child nodes of the tree (>= n_int; more: the deeper ones are read from L2)
    float R = 0.0f;               // >= max_node |c - mu|
    float coef_a = 0.0f, coef_b = 0.0f;
    uint2 *wl = nullptr;          // [n] undecided (row, node)
    // two counters used in turn: a call appends under wl_count[turn] and its continuation kernel, which is the last to
    // read it, clears the OTHER one for the next call -- the memset in front of every call was one launch in four
    uint32_t *wl_count = nullptr;
    mutable uint32_t turn = 0;    // counter of the next call (flipped by launch_tsvq_screen_encode, under the handle's lock)
};
size_t tsvq_screen_lds_bytes(uint32_t n_int, uint32_t nv, uint32_t d);
uint32_t tsvq_screen_width(uint32_t d);  // instantiated width serving d (zero padding for other multiples of 4), 0 = none
bool tsvq_screen_supported(uint32_t n_int, uint32_t n_nodes, uint32_t d, int metric);
int launch_tsvq_screen_encode(const float *X, uint64_t n, uint32_t d, const float *centroids, const float *cnorm,
                              const int32_t *left, const int32_t *right, int metric, const TsvqScreen &s, int32_t *leaf,
                              hipStream_t stream, const uint16_t *table16 = nullptr, uint16_t *f16_out = nullptr,
                              LaunchStage *stage = nullptr);  // stage: events for the call's kernels to carry (the last keeps the stop)
int launch_tsvq_gather_f16(const float *centroids, uint32_t d, const int32_t *leaf, uint64_t n, uint16_t *f16_out,
                           hipStream_t stream);
int launch_tsvq_node_norms(const float *centroids, uint32_t n_nodes, uint32_t d, float *cnorm, hipStream_t stream);
int launch_tsvq_encode(const float *X, uint64_t n, uint32_t d, const float *centroids, const float *cnorm,
                       const int32_t *left, const int32_t *right, int metric, int32_t *leaf, hipStream_t stream);
int launch_tsvq_table_f16(const float *centroids, uint32_t n_nodes, uint32_t d, uint16_t *table, hipStream_t stream);
int launch_tsvq_gather_table(const uint16_t *table, uint32_t d, const int32_t *leaf, uint64_t n, uint16_t *f16_out,
                             hipStream_t stream);

// ---- outputs / misc ---------------------------------------------------------------
int launch_gather_f16(const CodebookView &cb, const uint8_t *codes, uint64_t n, uint16_t *f16_out,
                      hipStream_t stream);
int launch_decode_f32(const CodebookView &cb, const uint8_t *codes, uint64_t n, float *out,
                      hipStream_t stream);
int launch_dequant_f16(const uint16_t *in, uint64_t count, float *out, hipStream_t stream);
// binary index: BQ bits packed 32 to a word, exact Hamming top-k (k_binary.hip).  x [n][d] f32 (kind VQHIP_BINARY_F32:
// bit = x >= thr) or u8 codes (VQHIP_BINARY_U8: bit = c >= high) -> out [n][bin_words(d)], pad bits zero.
struct BinSel {
    uint32_t hstar, less, need, heavy;  // the cut, rows below it, rows at it that belong to the result, cut too dense
};
uint32_t bin_words(uint32_t d);
// S [d + 1]: S[0] = +0.0, S[j] = S[j - 1] + t in sequential f32, t = a * a (squared / Euclidean) or a (Manhattan)
int binary_table(uint32_t d, uint32_t low, uint32_t high, int metric, float *S);
int launch_bq_pack(const void *x, int kind, uint64_t n, uint32_t d, float thr, uint32_t high, uint32_t *out, hipStream_t stream);
// *bad |= 1 where a packed row has a pad bit set (the caller zeroes it first)
int launch_bin_padcheck(const uint32_t *P, uint64_t n, uint32_t d, uint32_t *bad, hipStream_t stream);
size_t binary_hist_bytes(uint32_t qb, uint32_t d);
// Q [nb][W] packed queries, nb <= 1024; workspaces hist >= binary_hist_bytes(nb, d), sel [nb], adc_sel [2 nb], cnt [nb],
// cand >= topk_cand_bytes(nb); results [nb][topk] on the device.  mask (here and in launch_binary_range): the row mask of
// a filtered call on the device, ceil(n / 32) words, 4-byte aligned -- the masked kernels, which
// select among the allowed rows and pad a query with fewer than topk of them; NULL: the unmasked kernels as they are.
int launch_binary_search(const uint32_t *P, uint64_t n, uint32_t d, int metric, const float *S, const uint32_t *Q, uint32_t nb,
                         uint32_t topk, uint32_t *hist, BinSel *sel, uint32_t *adc_sel, uint32_t *cnt,
                         unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream,
                         const uint32_t *mask = nullptr);
// rows per scan workgroup of a filtered search over n rows and `groups` query groups: a multiple of 64, at most 65472
uint64_t binary_masked_slice(uint64_t n, uint32_t groups);
// Hamming-radius range search over the same rows: queries_dev [nq][d] f32 are packed a batch at a
// time (binary_range_batch queries) into qw [batch][W]; hcut [nq + 32] on the device, the radii clamped to d with 32
// entries of padding behind them; range_ws >= binary_range_ws_bytes(n, d, nq).  Row i is a hit of query q iff H <= hcut[q];
// *out as launch_knn_range leaves it, complete on return.  More than max_results hits: VQHIP_ERR_UNSUPPORTED.
uint32_t binary_range_batch(uint64_t n, uint32_t d, uint32_t nq);
size_t binary_range_ws_bytes(uint64_t n, uint32_t d, uint32_t nq);
int launch_binary_range(const uint32_t *P, uint64_t n, uint32_t d, int metric, const float *S, const float *queries_dev, float thr,
                        uint32_t high, uint32_t nq, const uint32_t *hcut, uint64_t max_results, uint32_t *qw, void *range_ws,
                        RangeOut *out, hipStream_t stream, const uint32_t *mask = nullptr);

int launch_synth_uniform(float *X, uint64_t n, uint32_t d, uint64_t seed, uint64_t row_offset,
                         hipStream_t stream);
void synth_uniform_host(float *out, uint64_t n, uint32_t d, uint64_t seed, uint64_t row_offset);

// ---- ScalarQuantizer / BinaryQuantizer (k_sqbq.hip) --------------------------------
// Parameters travel by value as kernel arguments; the tables are built on the host with the reference's arithmetic.
enum { SQBQ_TABLE = 0, SQBQ_DIRECT = 1, SQBQ_BINARY = 2 };
constexpr uint32_t kSqTable = 257;  // b[0] = -inf, b[1..levels-1] thresholds, b[levels] = NaN
struct SqbqEncodeOp {
    int mode = SQBQ_DIRECT;
    float mn = 0, mx = 0, step = 0, inv = 0;  // SQ
    uint32_t top = 0;                         // SQ: levels - 1
    float thr = 0;                            // BQ
    uint32_t low = 0, high = 0;               // BQ
    float b[kSqTable] = {};                   // SQ, SQBQ_TABLE: b[i] = smallest f32 whose code is >= i
};
struct SqbqDecodeLut {
    float lut[256];  // the reference's dequantize of each code byte
};
// validation in the reference's order; the texts are its `Display` ("Invalid parameter '<p>': <reason>")
int sq_check(float mn, float mx, uint32_t levels, float *step);
int bq_check(float threshold, uint32_t low, uint32_t high);
// b[0..levels): b[0] = -inf, b[i] = the smallest f32 whose code is >= i (NaN if none); parameters already checked
void sq_thresholds(float mn, float mx, uint32_t levels, float step, float *b);
int sq_encode_op(float mn, float mx, uint32_t levels, SqbqEncodeOp *p);
int bq_encode_op(float threshold, uint32_t low, uint32_t high, SqbqEncodeOp *p);
int sq_decode_lut(float mn, float mx, uint32_t levels, SqbqDecodeLut *p);
int bq_decode_lut(float threshold, uint32_t low, uint32_t high, SqbqDecodeLut *p);
// any alignment of x (4 bytes) / codes (1 byte), any count
int launch_sqbq_encode(const SqbqEncodeOp &p, const float *x, uint64_t count, uint8_t *codes, hipStream_t stream);
int launch_sqbq_decode(const SqbqDecodeLut &p, const uint8_t *codes, uint64_t count, float *out, hipStream_t stream);

// stable compaction of n rows of rb bytes under a remove mask on the device (k_compact.hip, compact.hpp): ceil(n / 32)
// words, row i removed iff bit i & 31 of word i >> 5 is set.  launch_compact_plan counts and scans into ws (>=
// compact_ws_bytes(n)) and leaves the number of survivors at compact_survivors(ws, n); launch_compact_move, once per
// payload of the index, copies the survivors of src to dst (na * rb bytes, no overlap with src) in their old order.
size_t compact_ws_bytes(uint64_t n);
const uint32_t *compact_survivors(const void *ws, uint64_t n);
int launch_compact_plan(const uint32_t *remove_dev, uint64_t n, void *ws, hipStream_t stream);
int launch_compact_move(const uint32_t *remove_dev, uint64_t n, const void *ws, const void *src, void *dst, uint64_t rb,
                        hipStream_t stream);

// removing rows from an inverted file on the device (k_ivf_remove.hip, ivf_remove.hpp), behind launch_ivf_view over the
// mask of the rows that stay: launch_ivf_take copies row pick[j] of src (rb bytes a row) to row j of dst for j < na (no
// overlap); launch_ivf_renumber writes ids[j] = aids[j] - (the removed rows under aids[j]), `allowed` the view's mask and
// prefix[w] the removed rows below row 32 w.  Enqueued on stream.
int launch_ivf_take(const uint32_t *pick, uint64_t na, const void *src, void *dst, uint64_t rb, hipStream_t stream);
int launch_ivf_renumber(const uint32_t *aids, uint64_t na, const uint32_t *allowed, const uint32_t *prefix, uint32_t *ids,
                        hipStream_t stream);

}  // namespace vqhip
