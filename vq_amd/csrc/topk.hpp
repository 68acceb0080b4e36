// topk.hpp -- exact per-query top-k over f32 distances, shared by the ADC search (k_adc.hip) and the exact
// k-NN search (k_knn.hip).  Device code only; every including file gets its own copy of the kernels.
//   adc_key / adc_unkey : the order-preserving key of a distance (NaN sorts last, reported back as 0x7FC00000)
//   k_adc_pick_bin      : the histogram bin that holds the topk-th smallest value
//   k_adc_sort_out      : the candidates of a query sorted by (key, row) in LDS, the first topk out
//   k_adc_topk          : exact radix select where the candidate cut was too dense
//   adc_terms / adc_row : D(q, i) of one row from ADC tables in LDS, subspace 0 first -- the one operation order of the ADC
//                         scans (k_adc.hip) and the IVF scan (k_ivf.hip)
#pragma once
#include "adc_plan.hpp"
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

__device__ __forceinline__ uint32_t adc_key(float f) {  // order-preserving; NaN sorts last
    const uint32_t b = __float_as_uint(f);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float adc_unkey(uint32_t k) {
    if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// QL consecutive table entries (QL queries' terms of one (subspace, code)) from float offset `at`
template <uint32_t QL>
__device__ __forceinline__ void adc_terms(const float *__restrict__ lds, uint32_t at, float (&v)[QL]) {
    if constexpr (QL == 1) {
        v[0] = lds[at];
    } else if constexpr (QL == 2) {
        const float2 a = *reinterpret_cast<const float2 *>(lds + at);
        v[0] = a.x, v[1] = a.y;
    } else {
#pragma unroll
        for (uint32_t h = 0; h < QL / 4; ++h) {
            const float4 a = *reinterpret_cast<const float4 *>(lds + at + 4 * h);
            v[4 * h] = a.x, v[4 * h + 1] = a.y, v[4 * h + 2] = a.z, v[4 * h + 3] = a.w;
        }
    }
}

// D(q, i) of QL of the batch's qb queries (those from `first` on) for row i, subspace 0 first (the order of k_adc_scan and
// of the oracle)
template <uint32_t QL>
__device__ __forceinline__ void adc_row(const uint8_t *__restrict__ codes, uint64_t i, uint32_t m, uint32_t k, bool words,
                                        const float *__restrict__ lds, uint32_t qb, uint32_t first, float (&acc)[QL]) {
    float v[QL];
    if (words) {  // one-byte codes, rows of whole 8-byte words
        for (uint32_t s8 = 0; s8 < m; s8 += 8) {
            const uint2 w = *reinterpret_cast<const uint2 *>(codes + i * m + s8);
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b) {
                const uint32_t s = s8 + b;
                adc_terms<QL>(lds, (s * k + (((b < 4 ? w.x : w.y) >> (8 * (b & 3))) & 255u)) * qb + first, v);
#pragma unroll
                for (uint32_t qq = 0; qq < QL; ++qq) acc[qq] = (s == 0) ? v[qq] : acc[qq] + v[qq];
            }
        }
    } else {
        for (uint32_t s = 0; s < m; ++s) {
            adc_terms<QL>(lds, (s * k + load_code(codes, i * m + s, k)) * qb + first, v);
#pragma unroll
            for (uint32_t qq = 0; qq < QL; ++qq) acc[qq] = (s == 0) ? v[qq] : acc[qq] + v[qq];
        }
    }
}

// (kAdcBins, the histogram bins of the candidate filter: adc_plan.hpp)
constexpr uint32_t kAdcCand = 8192; // candidates the fast top-k path sorts in LDS

// fast top-k, step 1: the bin that holds the k-th smallest value; sel[q] = {bin, candidates up to it}
__attribute__((unused)) __global__ __launch_bounds__(64) void k_adc_pick_bin(const uint32_t *__restrict__ hist, uint32_t topk,
                                                     uint32_t *__restrict__ sel) {
    const uint32_t q = blockIdx.x;
    if (threadIdx.x != 0) return;
    uint32_t cum = 0, b = 0;
    for (; b < kAdcBins; ++b) {
        cum += hist[q * kAdcBins + b];
        if (cum >= topk) break;
    }
    sel[2 * q + 0] = b;
    sel[2 * q + 1] = cum;
}

// step 3: sort the candidates by (key, row) in LDS, emit the first topk
__attribute__((unused)) __global__ __launch_bounds__(1024) void k_adc_sort_out(const unsigned long long *__restrict__ cand,
                                                       const uint32_t *__restrict__ sel, uint32_t topk, int take_sqrt,
                                                       uint32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
    extern __shared__ unsigned long long sort_buf[];  // [kAdcCand]
    const uint32_t q = blockIdx.x, cnt = sel[2 * q + 1];
    if (cnt > kAdcCand) return;  // handled by k_adc_topk
    uint32_t len = 1024;
    while (len < cnt) len <<= 1;
    for (uint32_t e = threadIdx.x; e < len; e += 1024) sort_buf[e] = (e < cnt) ? cand[(size_t)q * kAdcCand + e] : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= len; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < len; t += 1024) {
                const uint32_t partner = t ^ stride;
                if (partner > t) {
                    const bool up = (t & size) == 0;
                    const unsigned long long a = sort_buf[t], b = sort_buf[partner];
                    if ((a > b) == up) {
                        sort_buf[t] = b;
                        sort_buf[partner] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x < topk) {
        const unsigned long long w = sort_buf[threadIdx.x];
        float dv = adc_unkey((uint32_t)(w >> 32));
        if (take_sqrt) dv = sqrtf(dv);
        idx_out[(size_t)q * topk + threadIdx.x] = (uint32_t)w;
        dist_out[(size_t)q * topk + threadIdx.x] = dv;
    }
}

// exact top-k of one query's distances: radix select of the k-th key, ordered collection (ties by
// row index), bitonic sort of the <= 1024 winners by (key, index)
__attribute__((unused)) __global__ __launch_bounds__(1024) void k_adc_topk(const float *__restrict__ dist, uint64_t n, uint32_t topk, int take_sqrt,
                                                   const uint32_t *__restrict__ sel, uint32_t *__restrict__ idx_out,
                                                   float *__restrict__ dist_out) {
    __shared__ uint32_t hist[256];
    if (sel && sel[2 * blockIdx.x + 1] <= kAdcCand) return;  // the candidate path produced this query's result
    __shared__ uint32_t s_prefix, s_rank, s_count;
    __shared__ uint32_t wsum[16];
    __shared__ unsigned long long win[1024];
    const float *dq = dist + (size_t)blockIdx.x * n;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_prefix = 0;
        s_rank = topk - 1;
    }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix, himask = (shift == 24) ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (uint64_t i = tid; i < n; i += 1024) {
            const uint32_t key = adc_key(dq[i]);
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rank = s_rank, b = 0;
            for (; b < 255; ++b) {
                if (rank < hist[b]) break;
                rank -= hist[b];
            }
            s_rank = rank;
            s_prefix = prefix | (b << shift);
        }
        __syncthreads();
    }
    const uint32_t T = s_prefix;         // the k-th smallest key
    const uint32_t need_eq = s_rank + 1;  // how many keys == T belong to the result (lowest row indices)
    if (tid == 0) s_count = 0;
    __syncthreads();
    // ordered collection: chunks of 1024 rows, block prefix sums keep row order
    uint32_t eq_taken = 0;  // replicated in every thread (uniform updates)
    for (uint64_t base = 0; base < n; base += 1024) {
        const uint64_t i = base + tid;
        uint32_t key = 0xFFFFFFFFu;
        bool less = false, eq = false;
        if (i < n) {
            key = adc_key(dq[i]);
            less = key < T;
            eq = key == T;
        }
        // ranks among this chunk's `eq` rows and among its selected rows (wave scan + wave sums)
        const uint64_t eqm = __ballot(eq);
        const uint32_t lane = tid & 63, wv = tid >> 6;
        const uint32_t eq_before_w = __popcll(eqm & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(eqm);
        __syncthreads();
        uint32_t eq_before = eq_before_w, eq_total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wv) eq_before += wsum[w];
            eq_total += wsum[w];
        }
        __syncthreads();
        const bool take = less || (eq && (eq_taken + eq_before < need_eq));
        const uint64_t tm = __ballot(take);
        const uint32_t t_before_w = __popcll(tm & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(tm);
        __syncthreads();
        uint32_t t_before = t_before_w, t_total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wv) t_before += wsum[w];
            t_total += wsum[w];
        }
        const uint32_t pos = s_count + t_before;
        if (take && pos < 1024) win[pos] = ((unsigned long long)key << 32) | (uint32_t)i;
        __syncthreads();
        if (tid == 0) s_count += t_total;
        {
            const uint32_t remaining = need_eq - eq_taken;  // eq_taken <= need_eq always
            eq_taken += eq_total < remaining ? eq_total : remaining;
        }
        __syncthreads();
        if (s_count >= topk) break;  // uniform
    }
    const uint32_t got = s_count < topk ? s_count : topk;
    for (uint32_t e = tid; e < 1024; e += 1024)
        if (e >= got) win[e] = ~0ull;
    __syncthreads();
    // bitonic sort of 1024 (key, index) pairs
    for (uint32_t size = 2; size <= 1024; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            const uint32_t partner = tid ^ stride;
            if (partner > tid) {
                const bool up = (tid & size) == 0;
                const unsigned long long a = win[tid], b = win[partner];
                if ((a > b) == up) {
                    win[tid] = b;
                    win[partner] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid < topk) {
        const unsigned long long w = win[tid];
        const bool valid = tid < got;
        float dv = adc_unkey((uint32_t)(w >> 32));
        if (take_sqrt) dv = sqrtf(dv);
        idx_out[(size_t)blockIdx.x * topk + tid] = valid ? (uint32_t)w : 0xFFFFFFFFu;
        dist_out[(size_t)blockIdx.x * topk + tid] = valid ? dv : __uint_as_float(0x7FC00000u);
    }
}

}  // namespace
}  // namespace vqhip
