// Inverted-file search over SQ codes (include/vqhip.h, vqhip_ivfsq_*): k_ivfflat.hip's search with the
// row side read as one byte per dimension and decoded where it leaves global memory, as k_sqindex.hip decodes it:
//   v(c)    = mn + (float)c * step for every byte value c (sq_decode.hpp: two roundings, never fused),
//   D(q, i) = the flat index's distance over the decoded row (knn_tile.hpp: knn_step from -0.0 over ascending
//             dimensions, knn_finish), so every result equals IVFFlatIndex over the dequantized rows in the same lists.
// The index keeps its codes in list order: list l is the run C[off[l] * d .. off[l + 1] * d) of one buffer the index owns,
// so with d % 16 == 0 (d % 4 == 0) every row of every list starts on a 16-byte (4-byte) boundary.
// Schedule of one batch (launch_ivfsq_search): section 14's, step for step --
//   launch_ivff_plan    k_ivff_plan, k_ivff_lists, k_ivff_invert (k_ivfflat.hip): pref / seg, cnt, the inverted probe table
//   ivff_distances      k_ivff_tile and k_ivff_scan (ivf_tile.hpp) instantiated with the row source SqRows (sq_decode.hpp):
//                       the row chunk loaded as codes, 16, 4 or 1 byte per load; the row walked as dwords or bytes
//   launch_ivff_select  k_ivff_hist and the selection stage over IvffSource (k_ivfflat.hip)
// Which kernel computes a pair depends on the batch; both run one pair's operations in one order, so the bits do not.
// A range search (launch_ivfsq_range) puts the range stage (launch_ivff_range) behind the same
// plan and distance passes.
#include "common.hpp"
#include "ivf_tile.hpp"
#include "kernels.hpp"
#include "sq_decode.hpp"

#pragma clang fp contract(off)

namespace vqhip {

// One batch of nb <= 1024 queries (queries [nb][d] f32, qnorm [nb] under the cosines) whose probe lists
// (probe [nb][nprobe], launch_knn_search) are on the device.  C / rnorm / ids / off: the index in list order, C [n][d]
// u8 with v(c) = mn + (float)c * step, rnorm from launch_sq_norms over C.  The workspaces are launch_ivfflat_search's.
// Results [nb][topk] on the device.
int launch_ivfsq_search(int metric, const uint8_t *C, uint32_t d, float mn, float step, const float *rnorm, const uint32_t *ids,
                        const uint32_t *off, uint32_t nlist, uint64_t max_list, const float *queries, const float *qnorm,
                        const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk, uint64_t wstride,
                        float *W, uint32_t *pref, uint32_t *seg, uint32_t *inv, uint32_t *lists, void *state,
                        unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream) {
    if (nb == 0) return VQHIP_OK;
    IvffPlan p;
    VQ_TRY(launch_ivff_plan(off, nlist, max_list, probe, nb, nprobe, topk, pref, seg, inv, lists, state, &p, stream));
    VQ_TRY(sq_rows(C, d, mn, step, [&](auto rows) {
        return ivff_distances(p, metric, rows, rnorm, off, nlist, queries, qnorm, probe, nb, nprobe, chunk, wstride, W, pref, seg, inv,
                              stream);
    }));
    return launch_ivff_select(p, W, wstride, pref, seg, ids, nb, nprobe, topk, cand, idx_out, dist_out, stream);
}

// launch_ivfsq_search's batch with the range stage behind the distances (launch_ivff_range, k_ivfflat.hip): the arguments
// of launch_ivfflat_range with the rows as SQ codes.
int launch_ivfsq_range(int metric, const uint8_t *C, uint32_t d, float mn, float step, const float *rnorm, const uint32_t *ids, uint64_t n,
                       const uint32_t *off, uint32_t nlist, uint64_t max_list, const float *queries, const float *qnorm,
                       const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t chunk, uint64_t wstride, float *W, uint32_t *pref,
                       uint32_t *seg, uint32_t *inv, uint32_t *lists, void *state, uint32_t q0, const float *radii, void *range_ws,
                       DevBuf *stage, uint64_t max_results, RangeOut *out, hipStream_t stream) {
    if (nb == 0) return VQHIP_OK;
    IvffPlan p;
    VQ_TRY(launch_ivff_plan(off, nlist, max_list, probe, nb, nprobe, 1, pref, seg, inv, lists, state, &p, stream));
    VQ_TRY(sq_rows(C, d, mn, step, [&](auto rows) {
        return ivff_distances(p, metric, rows, rnorm, off, nlist, queries, qnorm, probe, nb, nprobe, chunk, wstride, W, pref, seg, inv,
                              stream);
    }));
    return launch_ivff_range(W, wstride, pref, seg, ids, n, nb, nprobe, q0, radii, range_ws, stage, max_results, out, stream);
}

}  // namespace vqhip
