// k_sq4index.hip -- exact top-k search, range search and rerank of f32 queries over ScalarQuantizer codes of at most 16
// levels resident on the device, packed eight to a word.  No reference counterpart; the semantics are include/vqhip.h's:
//   v(c)    = mn + (float)c * step for every nibble value 0 .. 15 (the SQ decode rule, two roundings)
//   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit: the arithmetic, its order and the two norms of k_knn.hip over
//             the decoded row, so every result equals the scalar index over the same codes as bytes and the flat index
//             over the dequantized rows, indices and distance bits
// The kernels, schedules and host drivers are k_knn.hip's (knn_tile.hpp), instantiated here with the row source
// NibbleRows (nibble_decode.hpp): a chunk of the tile is four words per row, expanded where it leaves global memory --
// into the transposed LDS tile (k_knn_dist) or in registers (k_knn_rerank, k_knn_norms).  The row side of a chunk is 1 KB
// of codes instead of 2 KB of bytes or 8 KB of floats.  The pack kernel (u8 codes -> words) and the pad check of packed
// device words are here too.
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "nibble_decode.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// One lane per word: eight codes of one row -> word g = row * W + w, dimensions past d as zero nibbles.  VEC (d % 8 == 0
// and C 8-byte aligned): the eight bytes in one load.  *bad |= 1 where a code is above 15 (the word then holds its low
// four bits; the caller drops the rows).
template <bool VEC>
__global__ __launch_bounds__(256) void k_sq4_pack(const uint8_t *__restrict__ C, uint64_t n, uint32_t d, uint32_t W,
                                                  uint32_t *__restrict__ out, uint32_t *__restrict__ bad) {
    const uint64_t total = n * W;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        const uint64_t row = g / W;
        const uint32_t t0 = (uint32_t)(g % W) * 8;
        const uint8_t *c = C + row * d + t0;
        uint32_t word = 0, over = 0;
        if constexpr (VEC) {
            const uint2 v = *reinterpret_cast<const uint2 *>(c);
            over = (v.x | v.y) & 0xF0F0F0F0u;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                word |= ((v.x >> (8 * j)) & 15u) << (4 * j);
                word |= ((v.y >> (8 * j)) & 15u) << (4 * (j + 4));
            }
        } else {
            const uint32_t m = min(8u, d - t0);
            for (uint32_t j = 0; j < m; ++j) {
                const uint32_t b = c[j];
                over |= b & 0xF0u;
                word |= (b & 15u) << (4 * j);
            }
        }
        out[g] = word;
        if (over) atomicOr(bad, 1u);
    }
}

// *bad |= 1 where a pad nibble (dimension >= d) of a packed row is set; keep: the bits of the last word's dimensions
__global__ __launch_bounds__(256) void k_sq4_padcheck(const uint32_t *__restrict__ P, uint64_t n, uint32_t W, uint32_t keep,
                                                      uint32_t *__restrict__ bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (P[i * W + (W - 1)] & ~keep) atomicOr(bad, 1u);
}

NibbleRows nib_rows(const uint32_t *P, uint32_t d, float mn, float step) { return NibbleRows{P, d, {mn, step}}; }

}  // namespace

uint32_t sq4_words(uint32_t d) { return nib_row_words(d); }

int launch_sq4_pack(const uint8_t *C, uint64_t n, uint32_t d, uint32_t *out, uint32_t *bad, hipStream_t stream) {
    if (n == 0) return VQHIP_OK;
    const uint32_t W = nib_row_words(d);
    const uint64_t blocks = std::min<uint64_t>((n * W + 255) / 256, 8192);
    if (d % 8 == 0 && (reinterpret_cast<uintptr_t>(C) & 7) == 0)
        hipLaunchKernelGGL(k_sq4_pack<true>, dim3((uint32_t)blocks), dim3(256), 0, stream, C, n, d, W, out, bad);
    else
        hipLaunchKernelGGL(k_sq4_pack<false>, dim3((uint32_t)blocks), dim3(256), 0, stream, C, n, d, W, out, bad);
    VQ_LAUNCH_CHECK("k_sq4_pack");
    return VQHIP_OK;
}

int launch_sq4_padcheck(const uint32_t *P, uint64_t n, uint32_t d, uint32_t *bad, hipStream_t stream) {
    if (d % 8 == 0 || n == 0) return VQHIP_OK;
    const uint32_t W = nib_row_words(d), keep = (1u << (4 * (d % 8))) - 1u;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_sq4_padcheck, dim3((uint32_t)blocks), dim3(256), 0, stream, P, n, W, keep, bad);
    VQ_LAUNCH_CHECK("k_sq4_padcheck");
    return VQHIP_OK;
}

// sqrtf(sum_t v(c_t)^2) per row, sequential from -0.0f (the row-norm chain of exact_distance_rt over the decoded row)
int launch_sq4_norms(const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, float *out, hipStream_t stream) {
    return knn_norms_rows(nib_rows(P, d, mn, step), n, out, stream);
}

// P [n][sq4_words(d)] on the device, rnorm [n] (cosine; launch_sq4_norms), queries_dev [nq][d] f32, qnorm_dev [nq] (cosine;
// launch_knn_norms); the batches and workspaces are launch_knn_search's
int launch_sq4_search(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                      unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, const uint32_t *mask_dev,
                      hipStream_t stream) {
    return knn_search_rows(metric, nib_rows(P, d, mn, step), n, rnorm, queries_dev, qnorm_dev, nq, topk, dist_ws, state_ws, cand_ws,
                           idx_out_dev, dist_out_dev, mask_dev, stream);
}

// launch_sq4_search with the range stage behind the distances (launch_knn_range); range_ws >= range_ws_bytes(n, nq)
int launch_sq4_range(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                     float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, const uint32_t *mask_dev, hipStream_t stream) {
    return knn_range_rows(metric, nib_rows(P, d, mn, step), n, rnorm, queries_dev, qnorm_dev, nq, radii_dev, max_results, dist_ws,
                          state_ws, range_ws, out, mask_dev, stream);
}

// launch_knn_rerank with the candidate's row read as words and decoded in registers
int launch_sq4_rerank(int metric, const uint32_t *P, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                      const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                      uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    return knn_rerank_rows(metric, nib_rows(P, d, mn, step), n, rnorm, queries_dev, qnorm_dev, nq, cand_dev, c, topk, idx_out_dev,
                           dist_out_dev, err_dev, stream);
}

}  // namespace vqhip
