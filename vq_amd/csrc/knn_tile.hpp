// knn_tile.hpp -- what the exact distance passes over resident rows share: the f32 rows of k_knn.hip and the u8 SQ codes
// of k_sqindex.hip.  The tile shape, one pair's arithmetic (the operation order of Distance::compute), the key-space
// histogram over the distances and the source it makes of them for the selection stage (topk.hpp).  Every including
// file gets its own copy of the kernel (an anonymous namespace: no relocatable device code).
#pragma once
#include "kernels.hpp"
#include "topk.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

constexpr uint32_t kKnnRQ = 8, kKnnRR = 4;                  // (query, row) pairs per lane
constexpr uint32_t kKnnTQ = 16 * kKnnRQ, kKnnTR = 16 * kKnnRR; // tile: 16 query groups x 16 row groups = 256 lanes
constexpr uint32_t kKnnKC = 32;                              // dimensions per LDS chunk
constexpr uint32_t kKnnRerankMax = 4096;                     // candidates per query of a rerank

// one pair's running sum advanced by one element
template <int METRIC>
__device__ __forceinline__ float knn_step(float acc, float q, float r) {
    if constexpr (METRIC == VQHIP_SQUARED_EUCLIDEAN || METRIC == VQHIP_EUCLIDEAN) {
        const float diff = q - r;
        const float sq = diff * diff;
        return acc + sq;
    } else if constexpr (METRIC == VQHIP_MANHATTAN) {
        const float diff = q - r;
        return acc + fabsf(diff);
    } else {
        const float p = q * r;
        return acc + p;
    }
}

template <int METRIC>
__device__ __forceinline__ float knn_finish(float acc, float qn, float rn) {
    if constexpr (METRIC == VQHIP_EUCLIDEAN) return sqrtf(acc);
    else if constexpr (vq_is_cos(METRIC)) return vq_cosine_finish(METRIC, acc, qn, rn);
    else return acc;
}

// monotone bin of a key: non-NaN keys (all within [lo, hi]) linearly over bins 0 .. kAdcBins-2, NaN in the last bin
__device__ __forceinline__ uint32_t knn_bin(uint32_t key, uint32_t lo, uint32_t hi) {
    if (key > hi) return kAdcBins - 1;
    if (key <= lo) return 0;
    return (uint32_t)(((uint64_t)(key - lo) * (kAdcBins - 1)) / ((uint64_t)(hi - lo) + 1));
}

__attribute__((unused)) __global__ __launch_bounds__(256) void k_knn_hist(const float *__restrict__ dist, uint64_t n, const uint32_t *__restrict__ kmin,
                                                  const uint32_t *__restrict__ kmax, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[kAdcBins];
    const uint32_t q = blockIdx.y, lo = kmin[q], hi = kmax[q];
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256) h[e] = 0u;
    __syncthreads();
    const float *dq = dist + (size_t)q * n;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        atomicAdd(&h[knn_bin(adc_key(dq[i]), lo, hi)], 1u);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256)
        if (h[e]) atomicAdd(&hist[(size_t)q * kAdcBins + e], h[e]);
}

// the search as a source of the selection stage (topk.hpp): dense rows, k_knn_hist's key bins over [kmin[q], kmax[q]]
struct KnnSource : TopkRows {
    const uint32_t *kmin, *kmax;
    uint32_t lo = 0, hi = 0;  // (device: of the opened query)
    __device__ void open(uint32_t q) {
        TopkRows::open(q);
        lo = kmin[q];
        hi = kmax[q];
    }
    __device__ uint32_t bin(float dval) const { return knn_bin(adc_key(dval), lo, hi); }
    uint32_t blocks() const { return (uint32_t)std::min<uint64_t>((n + 255) / 256, 64); }
};

inline uint32_t knn_grid(uint64_t items, uint32_t per_cu) {
    const uint64_t cap = (uint64_t)num_cus() * per_cu;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, cap));
}

}  // namespace
}  // namespace vqhip
