// k_sqindex.hip -- exact top-k search and exact rerank over ScalarQuantizer codes resident on the device, one byte per
// dimension, against f32 queries (never quantized).  No reference counterpart; the semantics are include/vqhip.h's:
//   v(c)    = min + (float)c * step for every byte value c (the SQ decode rule, un-fused; codes >= levels included)
//   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit: the arithmetic, its order and the two norms of k_knn.hip over
//             the decoded row, so every result equals the flat index over the dequantized rows, indices and distance bits
// The kernels, schedules and host drivers are k_knn.hip's (knn_tile.hpp), instantiated here with the row source SqRows
// (sq_decode.hpp): a byte is decoded where it leaves global memory -- on its way into the transposed LDS tile
// (k_knn_dist) or in registers (k_knn_rerank, k_knn_norms) -- by the formula itself (-ffp-contract=off and the file
// pragma keep the multiply and the add apart; f32 subnormals are not flushed).  That is three VALU operations per byte and
// no LDS traffic; the 256-entry table of sq_decode_lut costs a shift, a mask and a scattered ds_read per byte for the
// same bits.  The row side of a chunk is 2 KB of codes instead of 8 KB of floats.
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "sq_decode.hpp"

#pragma clang fp contract(off)

namespace vqhip {

// sqrtf(sum_t v(c_t)^2) per row, sequential from -0.0f (the row-norm chain of exact_distance_rt over the decoded row)
int launch_sq_norms(const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, float *out, hipStream_t stream) {
    return sq_rows(C, d, mn, step, [&](auto rows) { return knn_norms_rows(rows, n, out, stream); });
}

// codes [n][d] u8 on the device, rnorm [n] (cosine; launch_sq_norms), queries_dev [nq][d] f32, qnorm_dev [nq] (cosine;
// launch_knn_norms); the batches and workspaces are launch_knn_search's
int launch_sq_search(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                     unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                      hipStream_t stream) {
    return sq_rows(C, d, mn, step, [&](auto rows) {
        return knn_search_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, topk, dist_ws, state_ws, cand_ws, idx_out_dev,
                               dist_out_dev, mask_dev, stream);
    });
}

// launch_sq_search with the range stage behind the distances (launch_knn_range); range_ws >= range_ws_bytes(n, nq)
int launch_sq_range(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                    const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                    float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev,
                     hipStream_t stream) {
    return sq_rows(C, d, mn, step, [&](auto rows) {
        return knn_range_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, radii_dev, max_results, dist_ws, state_ws, range_ws,
                              out, mask_dev, stream);
    });
}

// launch_knn_rerank with the candidate's row read as codes and decoded in registers
int launch_sq_rerank(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                     uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    return sq_rows(C, d, mn, step, [&](auto rows) {
        return knn_rerank_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, cand_dev, c, topk, idx_out_dev, dist_out_dev,
                               err_dev, stream);
    });
}

}  // namespace vqhip
