// k_knn.hip -- exact k-nearest-neighbour search over rows resident on the device, and exact rerank of candidate lists.
// No reference counterpart (the crate has no search function); the semantics are the ones include/vqhip.h states:
//   D(q, i) = Distance::compute(q, row_i) bit for bit (vqhip_distance_batch): every pair summed sequentially over
//             t = 0 .. d-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean = sqrtf of the sum;
//             cosine = vq_cosine_finish(dot, |q|, |row_i|) with the two norms computed once (a norm depends on its own
//             vector only, so hoisting it changes no bit).
//   result  = the topk rows per query by (adc_key(D), row) ascending: NaN last, ties to the lower row.
// The kernels and the batched host drivers live in knn_tile.hpp, templated on the row source, and serve the scalar
// index too (k_sqindex.hip); this file instantiates them over dense f32 / f16 rows (DenseRows).
// Schedule of one search (launch_knn_search), per batch of queries whose [batch][n] f32 distances stay under 1 GB:
//   k_knn_dist     tiles of 128 queries x 64 rows per workgroup: the tile's query and row elements pass through LDS 32
//                  dimensions at a time, every lane advances an 8 x 4 block of (query, row) pairs by one chunk in
//                  register; writes every D and the per-query range [min, max] of the non-NaN keys
//   k_knn_hist     a 512-bin histogram per query, bins linear in KEY space over that range (monotone in D whatever the
//                  values: +-inf, NaN, huge ranges), NaN alone in the last bin
//   launch_topk_select   the shared selection stage (topk.hpp) over those distances and bins
// A range search (launch_knn_range) runs k_knn_dist over the same batches and then the range stage (range.hpp; DESIGN.md
// 15) in place of the histogram and the selection.
// A filtered search or range search (mask_dev: one row mask per call) runs k_knn_dist_masked, which leaves a
// row tile without an allowed row after its two mask words, and stages that read a row's mask bit before its distance.
// Roofline: VALU.  Squared L2 / Euclidean cost 3 unfused operations per (query, row, dimension), L1 2 (sub, then an add
// that takes |.| as a source modifier), cosine 2 (mul, add).
#include "kernels.hpp"
#include "knn_tile.hpp"

#pragma clang fp contract(off)

namespace vqhip {

int launch_knn_norms(const void *X, int dtype, uint64_t n, uint32_t d, float *out, hipStream_t stream) {
    return knn_dense_rows(X, dtype, d, [&](auto rows) { return knn_norms_rows(rows, n, out, stream); });
}

// queries per batch: their [batch][n] distances under 1 GB, whole query tiles where that allows, at most 1024
uint32_t knn_query_batch(uint64_t n, uint32_t nq) {
    uint64_t g = (1ull << 30) / std::max<uint64_t>(4 * n, 1);
    g = std::min<uint64_t>(std::max<uint64_t>(g, 1), 1024);
    if (g >= kKnnTQ) g = g / kKnnTQ * kKnnTQ;
    return (uint32_t)std::min<uint64_t>(g, std::max<uint32_t>(nq, 1));
}
// per query of a batch: kmin | kmax | the selection's state (topk.hpp)
size_t knn_state_bytes(uint32_t qb) { return (size_t)qb * 2 * 4 + topk_state_bytes(qb); }

size_t range_ws_bytes(uint64_t n, uint32_t nq) { return range_ws_size(n, knn_query_batch(n, nq)); }
int launch_range_begin(RangeOut *out, uint32_t nq, uint64_t max_results, hipStream_t stream) {
    return range_begin(out, nq, max_results, stream);
}

int launch_knn_search(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                      unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                      hipStream_t stream) {
    return knn_dense_rows(X, dtype, d, [&](auto rows) {
        return knn_search_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, topk, dist_ws, state_ws, cand_ws, idx_out_dev,
                               dist_out_dev, mask_dev, stream);
    });
}

int launch_knn_range(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                     const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results, float *dist_ws,
                     void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev,
                     hipStream_t stream) {
    return knn_dense_rows(X, dtype, d, [&](auto rows) {
        return knn_range_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, radii_dev, max_results, dist_ws, state_ws, range_ws,
                              out, mask_dev, stream);
    });
}

int launch_knn_rerank(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c, uint32_t topk,
                      uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    return knn_dense_rows(X, dtype, d, [&](auto rows) {
        return knn_rerank_rows(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, cand_dev, c, topk, idx_out_dev, dist_out_dev,
                               err_dev, stream);
    });
}

}  // namespace vqhip
