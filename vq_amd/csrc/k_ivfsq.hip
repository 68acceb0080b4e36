// Inverted-file search over SQ codes (include/vqhip.h, vqhip_ivfsq_*): k_ivfflat.hip's search with the
// row side read as one byte per dimension and decoded where it leaves global memory, as k_sqindex.hip decodes it:
//   v(c)    = mn + (float)c * step for every byte value c (sq_decode.hpp: two roundings, never fused),
//   D(q, i) = the flat index's distance over the decoded row (knn_tile.hpp: knn_step from -0.0 over ascending
//             dimensions, knn_finish), so every result equals IVFFlatIndex over the dequantized rows in the same lists.
// The index keeps its codes in list order: list l is the run C[off[l] * d .. off[l + 1] * d) of one buffer the index owns,
// so with d % 16 == 0 (d % 4 == 0) every row of every list starts on a 16-byte (4-byte) boundary.
// Schedule of one batch: section 14's, step for step, with launch_ivfsq_distances as its distance passes --
//   launch_ivff_plan    k_ivff_plan, k_ivff_lists, k_ivff_invert (k_ivfflat.hip): pref / seg, cnt, the inverted probe table
//   ivff_distances      k_ivff_tile and k_ivff_scan (ivf_tile.hpp) instantiated with the row source SqRows (sq_decode.hpp):
//                       the row chunk loaded as codes, 16, 4 or 1 byte per load; the row walked as dwords or bytes
//   launch_ivff_select  k_ivff_hist and the selection stage over IvffSource (k_ivfflat.hip)
// Which kernel computes a pair depends on the batch; both run one pair's operations in one order, so the bits do not.
// A range search puts the range stage (launch_ivff_range) behind the same plan and distance
// passes.
// A filtered call runs the same passes over the view of its allowed rows: v.pick set, the kernels
// instantiated over PickedRows<SqRows<LW>> (ivf_tile.hpp), whose alignment conditions are SqRows' own.
#include "common.hpp"
#include "ivf_tile.hpp"
#include "kernels.hpp"
#include "sq_decode.hpp"

#pragma clang fp contract(off)

namespace vqhip {

// The distance passes of a batch (kernels.hpp): ivff_distances over the row source SqRows.
int launch_ivfsq_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint8_t *C, uint32_t d, float mn, float step,
                           const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    return sq_rows(C, d, mn, step, [&](auto rows) { return ivff_distances(p, v, metric, rows, rnorm, queries, qnorm, stream); });
}

}  // namespace vqhip
