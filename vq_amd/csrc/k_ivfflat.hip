// Inverted-file search over the rows themselves (include/vqhip.h, vqhip_ivfflat_*).  The index keeps
// its rows in list order: list l holds the rows ids[off[l] .. off[l + 1]) (ascending) as one contiguous run of X, and
// their norms under the cosines.  Per query:
//   P(q)    = the nprobe lists the flat search over the coarse centroids returns (launch_knn_search, k_knn.hip),
//   S(q)    = the rows of those lists as ONE sequence of positions: probe slot 0's list, then slot 1's, ... (ivf_plan.hpp),
//   D(q, i) = the flat index's distance (knn_tile.hpp: knn_step from -0.0 over ascending dimensions, knn_finish),
//   result  = the topk rows of S(q) by (adc_key(D), row id) ascending; Euclidean ordered by the reported root; padding
//             (|S(q)| < topk) idx 0xFFFFFFFF, dist +inf.
// Schedule of one batch (launch_ivff_plan, launch_ivfflat_distances, launch_ivff_select):
//   k_ivff_plan    each query's prefix over its probed lists' lengths; cnt[l] = the batch's queries that probe list l
//   k_ivff_lists   prefix sums over the lists: lstart[l] (the list's run of the inverted table) and tstart[l] (its query
//                  tiles; none for a list probed by fewer than kIvffTileMin queries)
//   k_ivff_invert  the inverted probe table: inv[lstart[l] ..] = the (query, slot) pairs that probe l, in any order
//   k_ivff_tile    work item = one list x one tile of 128 of its queries x a column of tiles of 64 of its rows: k_knn_dist's
//                  8 x 4 register block over 32-dimension LDS chunks (knn_tile_pass), the queries gathered through inv,
//                  every D written to W[q][pref[q][slot] + r]; a list's rows are read once per query tile
//   k_ivff_scan    the lists probed by fewer than kIvffTileMin queries: work item = one query x one chunk of its positions,
//                  the query in LDS, one position per lane, the same per-pair operation order
//   k_ivff_hist    the key-space histogram of W[q][0 .. |S(q)|) over the range the two kernels found (integer atomics)
//   launch_topk_select over IvffSource: IvffRows' positions and ids (ivf_plan.hpp), KnnSource's bins.
// Which kernel computes a pair depends on the batch; both run one pair's operations in one order, so the bits do not.
// A range search runs the plan and the two distance kernels as they are and then the range stage over W
// (launch_ivff_range: ivf_range.hpp) in place of the histogram and the selection.
// The two distance kernels and ivff_distances live in ivf_tile.hpp, templated on the row source, and serve the SQ codes
// of k_ivfsq.hip too; this file instantiates them over dense f32 / f16 rows and holds the stages every inverted-file
// search over W shares (plan, lists, inverted table, histogram, selection, range).
// A filtered call first builds the inverted file of its allowed rows (launch_ivf_view: ivf_view.hpp)
// and runs this schedule over it: v.off / v.ids are the view's, and the two distance kernels are instantiated over
// PickedRows (ivf_tile.hpp), which reads row v.pick[j] of X for row j of the view.  No other stage knows.
#include "common.hpp"
#include "ivf_plan.hpp"
#include "ivf_range.hpp"
#include "ivf_tile.hpp"
#include "ivf_view.hpp"
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "topk.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

__device__ __forceinline__ bool ivff_real(uint32_t l, uint32_t nlist, const uint32_t *__restrict__ off) {
    return l < nlist && off[l + 1] > off[l];
}

// block = query (1024 threads): pref / seg as k_ivf_plan; cnt[l] += 1 for every non-empty list the query probes
__global__ __launch_bounds__(1024) void k_ivff_plan(const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                    const uint32_t *__restrict__ off, uint32_t *__restrict__ pref,
                                                    uint32_t *__restrict__ seg, uint32_t *__restrict__ cnt) {
    const uint32_t len = ivf_plan_prefix(probe, nprobe, nlist, off, pref, seg);
    if (threadIdx.x < nprobe && len > 0) atomicAdd(&cnt[probe[(size_t)blockIdx.x * nprobe + threadIdx.x]], 1u);
}

__device__ __forceinline__ uint32_t ivff_tiles(uint32_t c) { return c >= kIvffTileMin ? (c + kKnnTQ - 1) / kKnnTQ : 0u; }

// one block of 1024 threads: exclusive prefix sums of cnt[l] and of the lists' query tiles; lstart / tstart [nlist + 1]
__global__ __launch_bounds__(1024) void k_ivff_lists(const uint32_t *__restrict__ cnt, uint32_t nlist, uint32_t *__restrict__ lstart,
                                                     uint32_t *__restrict__ tstart) {
    __shared__ uint32_t s_c[1024], s_t[1024];
    const uint32_t t = threadIdx.x, per = (nlist + 1023) / 1024;
    const uint32_t a = min(nlist, t * per), b = min(nlist, a + per);
    uint32_t c = 0, tl = 0;
    for (uint32_t l = a; l < b; ++l) {
        c += cnt[l];
        tl += ivff_tiles(cnt[l]);
    }
    s_c[t] = c;
    s_t[t] = tl;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan
        const uint32_t vc = t >= d ? s_c[t - d] : 0u, vt = t >= d ? s_t[t - d] : 0u;
        __syncthreads();
        s_c[t] += vc;
        s_t[t] += vt;
        __syncthreads();
    }
    c = s_c[t] - c;
    tl = s_t[t] - tl;
    for (uint32_t l = a; l < b; ++l) {
        lstart[l] = c;
        tstart[l] = tl;
        c += cnt[l];
        tl += ivff_tiles(cnt[l]);
    }
    if (t == 1023) {
        lstart[nlist] = s_c[1023];
        tstart[nlist] = s_t[1023];
    }
}

// block = query: inv[lstart[l] + (a slot of the list's run, taken in any order)] = q * nprobe + slot
__global__ __launch_bounds__(1024) void k_ivff_invert(const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                      const uint32_t *__restrict__ off, const uint32_t *__restrict__ lstart,
                                                      uint32_t *__restrict__ fill, uint32_t *__restrict__ inv) {
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    if (t >= nprobe) return;
    const uint32_t l = probe[(size_t)q * nprobe + t];
    if (!ivff_real(l, nlist, off)) return;
    const uint32_t at = atomicAdd(&fill[l], 1u);
    if (at < lstart[l + 1] - lstart[l]) inv[lstart[l] + at] = q * nprobe + t;  // (always: fill counts what cnt counted)
}

// k_knn_hist over the positions of S(q): hist[q][bin] += 1 (integer atomics: the counts do not depend on their order)
__global__ __launch_bounds__(256) void k_ivff_hist(const float *__restrict__ W, uint64_t wstride, const uint32_t *__restrict__ pref,
                                                   uint32_t nprobe, const uint32_t *__restrict__ kmin,
                                                   const uint32_t *__restrict__ kmax, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[kAdcBins];
    const uint32_t q = blockIdx.y, lo = kmin[q], hi = kmax[q];
    const uint32_t total = (uint32_t)min((uint64_t)pref[(size_t)q * (nprobe + 1) + nprobe], wstride);
    if ((uint64_t)blockIdx.x * 256 >= total) return;  // (uniform)
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256) h[e] = 0u;
    __syncthreads();
    const float *wq = W + (size_t)q * wstride;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256)
        atomicAdd(&h[knn_bin(adc_key(wq[i]), lo, hi)], 1u);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256)
        if (h[e]) atomicAdd(&hist[(size_t)q * kAdcBins + e], h[e]);
}

// the two kernels' output as a source of the selection stage (topk.hpp): IvffRows' positions and row ids (ivf_plan.hpp),
// KnnSource's key bins over [kmin[q], kmax[q]] (knn_tile.hpp)
struct IvffSource : IvffRows {
    const uint32_t *kmin, *kmax;
    uint32_t lo = 0, hi = 0;  // (device: of the opened query)
    __device__ void open(uint32_t q) {
        IvffRows::open(q);
        lo = kmin[q];
        hi = kmax[q];
    }
    __device__ uint32_t bin(float dval) const { return knn_bin(adc_key(dval), lo, hi); }
    uint32_t blocks() const { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((wstride + 255) / 256, 1), 64); }
};

}  // namespace

// cnt | fill | lstart | tstart of a batch: [nlist] + [nlist] + [nlist + 1] + [nlist + 1] words (cnt and fill zeroed per batch)
size_t ivfflat_lists_bytes(uint32_t nlist) { return ((size_t)4 * nlist + 2) * 4; }

// The stages of a batch before its distance passes, the same for the three indexes: the batch's checks, the zeroed state,
// then k_ivff_plan, k_ivff_lists and k_ivff_invert.  *p: where the distance passes find cnt / lstart / tstart and the key
// range, and the grid of the tile kernel.
int launch_ivff_plan(const IvfBatchView &v, uint32_t topk, IvffPlan *p, hipStream_t stream) {
    const uint32_t nb = v.nb, nprobe = v.nprobe, nlist = v.nlist;
    *p = IvffPlan{};
    if (nb == 0) return VQHIP_OK;  // (no tiles: the distance passes and the stages behind them have nothing to do either)
    if (nb > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "a batch holds at most 1024 queries");
    if (nprobe == 0 || nprobe > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "nprobe must be in [1, 1024]");
    if (topk == 0 || topk > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, 1024]");
    uint32_t *cnt = v.lists, *fill = cnt + nlist, *lstart = fill + nlist, *tstart = lstart + nlist + 1;
    uint32_t *kmin = reinterpret_cast<uint32_t *>(v.state), *kmax = kmin + nb;
    VQ_HIP(hipMemsetAsync(cnt, 0, (size_t)2 * nlist * 4, stream));
    VQ_HIP(hipMemsetAsync(kmin, 0xFF, (size_t)nb * 4, stream));
    VQ_HIP(hipMemsetAsync(kmax, 0, knn_state_bytes(nb) - (size_t)nb * 4, stream));
    hipLaunchKernelGGL(k_ivff_plan, dim3(nb), dim3(1024), 0, stream, v.probe, nprobe, nlist, v.off, v.pref, v.seg, cnt);
    VQ_LAUNCH_CHECK("k_ivff_plan");
    hipLaunchKernelGGL(k_ivff_lists, dim3(1), dim3(1024), 0, stream, cnt, nlist, lstart, tstart);
    VQ_LAUNCH_CHECK("k_ivff_lists");
    hipLaunchKernelGGL(k_ivff_invert, dim3(nb), dim3(1024), 0, stream, v.probe, nprobe, nlist, v.off, lstart, fill, v.inv);
    VQ_LAUNCH_CHECK("k_ivff_invert");
    // the tiles the batch can have: a list with tiles has at least kIvffTileMin pairs and one partial tile
    const uint64_t pairs = (uint64_t)nb * nprobe;
    const uint64_t tiles_max = std::min<uint64_t>(nlist, pairs / kIvffTileMin) + pairs / kKnnTQ;
    // about eight workgroups per CU in all: columns of row tiles per query tile, at most the largest list's
    const uint64_t nrt = std::max<uint64_t>(1, (v.max_list + kKnnTR - 1) / kKnnTR);
    const uint64_t cols = tiles_max ? std::min<uint64_t>({nrt, 64, ((uint64_t)num_cus() * 8 + tiles_max - 1) / tiles_max}) : 0;
    *p = IvffPlan{cnt, lstart, tstart, kmin, kmax, kmax + nb, tiles_max, cols};
    return VQHIP_OK;
}

// The stages behind the distance passes: k_ivff_hist over W and the selection stage over IvffSource.
int launch_ivff_select(const IvffPlan &p, const IvfBatchView &v, uint32_t topk, unsigned long long *cand, uint32_t *idx_out,
                       float *dist_out, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    const TopkState st = topk_state(p.topk_ws, v.nb);
    const IvffSource src{{v.W, v.wstride, v.pref, v.seg, v.ids, v.nprobe}, p.kmin, p.kmax};
    hipLaunchKernelGGL(k_ivff_hist, dim3(src.blocks(), v.nb), dim3(256), 0, stream, v.W, v.wstride, v.pref, v.nprobe, p.kmin, p.kmax,
                       st.hist);
    VQ_LAUNCH_CHECK("k_ivff_hist");
    return launch_topk_select(src, v.nb, topk, 0, st, cand, idx_out, dist_out, stream);
}

// The range stage behind the distance passes (ivf_range.hpp).  The key range the distance passes write into state is not
// read.
size_t ivff_range_ws_bytes(uint64_t wstride, uint32_t nb) { return range_ws_size(wstride, nb); }
int launch_ivff_range(const IvfBatchView &v, uint32_t q0, const float *radii, void *range_ws, DevBuf *stage, uint64_t max_results,
                      RangeOut *out, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    return ivfr_batch(v, q0, radii, range_ws, stage, max_results, out, stream);
}

// The view of a filtered call (ivf_view.hpp): count, scan, fill and the lists' offsets, enqueued on stream.
size_t ivf_view_ws_bytes(uint64_t n) { return ivfv_ws_bytes(n); }
int launch_ivf_view(const uint32_t *allowed, const uint32_t *ids, uint64_t n, const uint32_t *off, uint32_t nlist, void *ws,
                    uint32_t *pick, uint32_t *aids, uint32_t *aoff, hipStream_t stream) {
    return ivfv_build(allowed, ids, n, off, nlist, ws, pick, aids, aoff, stream);
}

// The distance passes of a batch over dense f32 / f16 rows (v.pick: over the view of a filtered call).
int launch_ivfflat_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const void *X, int dtype, uint32_t d,
                             const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    return knn_dense_rows(X, dtype, d, [&](auto rows) { return ivff_distances(p, v, metric, rows, rnorm, queries, qnorm, stream); });
}

}  // namespace vqhip
