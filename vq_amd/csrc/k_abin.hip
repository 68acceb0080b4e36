// k_abin.hip -- exact top-k search, range search and rerank of f32 queries (never quantized) over BinaryQuantizer bits
// resident on the device, packed 32 to a word.  No reference counterpart; the semantics are include/vqhip.h's:
//   v(bit)  = bit ? (float)high : (float)low (the BQ decode rule)
//   D(q, i) = Distance::compute(q, v(bits[i])) bit for bit: the arithmetic, its order and the two norms of k_knn.hip over
//             the decoded row, so every result equals the flat index over the dequantized rows, and the scalar index over
//             the bits as 0/1 bytes under ScalarQuantizer(low, high, 2), indices and distance bits
// The kernels, schedules and host drivers are k_knn.hip's (knn_tile.hpp), instantiated here with the row source BitRows
// (bit_decode.hpp): a chunk of the tile is one word per row, expanded where it leaves global memory -- into the
// transposed LDS tile (k_knn_dist) or in registers (k_knn_rerank, k_knn_norms).  A shift, a mask and a select per
// dimension; the row side of a chunk is 256 bytes of bits instead of 8 KB of floats.
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "bit_decode.hpp"

#pragma clang fp contract(off)

namespace vqhip {

static BitRows bit_rows(const uint32_t *P, uint32_t d, float lo, float hi) { return BitRows{P, d, {lo, hi}}; }

// sqrtf(sum_t v(bit_t)^2) per row, sequential from -0.0f (the row-norm chain of exact_distance_rt over the decoded row)
int launch_abin_norms(const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, float *out, hipStream_t stream) {
    return knn_norms_rows(bit_rows(P, d, lo, hi), n, out, stream);
}

// P [n][bin_words(d)] on the device, rnorm [n] (cosine; launch_abin_norms), queries_dev [nq][d] f32, qnorm_dev [nq] (cosine;
// launch_knn_norms); the batches and workspaces are launch_knn_search's
int launch_abin_search(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                       const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                       unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                       hipStream_t stream) {
    return knn_search_rows(metric, bit_rows(P, d, lo, hi), n, rnorm, queries_dev, qnorm_dev, nq, topk, dist_ws, state_ws, cand_ws,
                           idx_out_dev, dist_out_dev, mask_dev, stream);
}

// launch_abin_search with the range stage behind the distances (launch_knn_range); range_ws >= range_ws_bytes(n, nq)
int launch_abin_range(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                      float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream) {
    return knn_range_rows(metric, bit_rows(P, d, lo, hi), n, rnorm, queries_dev, qnorm_dev, nq, radii_dev, max_results, dist_ws,
                          state_ws, range_ws, out, mask_dev, stream);
}

// launch_knn_rerank with the candidate's row read as words and decoded in registers
int launch_abin_rerank(int metric, const uint32_t *P, uint64_t n, uint32_t d, float lo, float hi, const float *rnorm,
                       const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                       uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    return knn_rerank_rows(metric, bit_rows(P, d, lo, hi), n, rnorm, queries_dev, qnorm_dev, nq, cand_dev, c, topk, idx_out_dev,
                           dist_out_dev, err_dev, stream);
}

}  // namespace vqhip
