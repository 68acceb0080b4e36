// k_knn.hip -- exact k-nearest-neighbour search over rows resident on the device, and exact rerank of candidate lists.
// No reference counterpart (the crate has no search function); the semantics are the ones include/vqhip.h states:
//   D(q, i) = Distance::compute(q, row_i) bit for bit (vqhip_distance_batch): every pair summed sequentially over
//             t = 0 .. d-1 from -0.0f, one rounding per operation, no fused multiply-add; Euclidean = sqrtf of the sum;
//             cosine = vq_cosine_finish(dot, |q|, |row_i|) with the two norms computed once (a norm depends on its own
//             vector only, so hoisting it changes no bit).
//   result  = the topk rows per query by (adc_key(D), row) ascending: NaN last, ties to the lower row.
// Schedule of one search (launch_knn_search), per batch of queries whose [batch][n] f32 distances stay under 1 GB:
//   k_knn_dist     tiles of 128 queries x 64 rows per workgroup: the tile's query and row elements pass through LDS 32
//                  dimensions at a time, every lane advances an 8 x 4 block of (query, row) pairs by one chunk in
//                  register; writes every D and the per-query range [min, max] of the non-NaN keys
//   k_knn_hist     a 512-bin histogram per query, bins linear in KEY space over that range (monotone in D whatever the
//                  values: +-inf, NaN, huge ranges), NaN alone in the last bin
//   launch_topk_select   the shared selection stage (topk.hpp) over those distances and bins
// A range search (launch_knn_range) runs k_knn_dist over the same batches and then the range stage (range.hpp; DESIGN.md
// 15) in place of the histogram and the selection.
// Roofline: VALU.  Squared L2 / Euclidean cost 3 unfused operations per (query, row, dimension), L1 2 (sub, then an add
// that takes |.| as a source modifier), cosine 2 (mul, add).
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "range.hpp"
#include "topk.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

template <typename RT>
__device__ __forceinline__ float knn_widen(RT v) {
    if constexpr (std::is_same<RT, uint16_t>::value) return (float)__builtin_bit_cast(_Float16, v);  // exact
    else return v;
}

// sqrtf(sum_t x_t^2) per vector, sequential from -0.0f (the norm chains of exact_distance_rt)
template <typename RT>
__global__ __launch_bounds__(256) void k_knn_norms(const RT *__restrict__ X, uint64_t n, uint32_t d, float *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const RT *x = X + i * d;
        float s = -0.0f;
        for (uint32_t t = 0; t < d; ++t) {
            const float v = knn_widen(x[t]);
            const float p = v * v;
            s = s + p;
        }
        out[i] = sqrtf(s);
    }
}

// dist[q][i] for the batch's nq queries.  Workgroup b owns query tile b % nqt and strides over the row tiles
// b / nqt, b / nqt + gridDim.x / nqt, ... (gridDim.x is a multiple of nqt): the workgroups in flight at one time share
// row tiles, so the rows come from HBM about once per call and from L2 for the other query tiles.
// kmin / kmax [nq]: the range of the non-NaN keys of each query (atomics, once per workgroup and query).
template <int METRIC, typename RT>
__global__ __launch_bounds__(256) void k_knn_dist(const float *__restrict__ Q, uint32_t nq, const RT *__restrict__ X, uint64_t n,
                                                  uint32_t d, const float *__restrict__ qnorm, const float *__restrict__ rnorm,
                                                  uint32_t nqt, uint64_t nrt, float *__restrict__ dist, uint32_t *__restrict__ kmin,
                                                  uint32_t *__restrict__ kmax) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, KC = kKnnKC;
    // transposed: lane (qg, rg) reads its 8 query and 4 row elements of dimension t as two + one 16-byte LDS reads
    // (+4: the loaders' column-major writes spread over the banks)
    __shared__ __attribute__((aligned(16))) float qs[KC][TQ + 4];
    __shared__ __attribute__((aligned(16))) float rs[KC][TR + 4];
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4;
    const uint32_t q0 = (blockIdx.x % nqt) * TQ;
    const uint64_t rstep = gridDim.x / nqt;
    float qn[RQ];
    uint32_t lo[RQ], hi[RQ];
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
        const uint32_t q = q0 + qg * RQ + a;
        qn[a] = (vq_is_cos(METRIC) && q < nq) ? qnorm[q] : 1.0f;
        lo[a] = 0xFFFFFFFFu;
        hi[a] = 0u;
    }
    for (uint64_t rt = blockIdx.x / nqt; rt < nrt; rt += rstep) {
        const uint64_t row0 = rt * TR;
        float acc[RQ][RR];
#pragma unroll
        for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
            for (uint32_t b = 0; b < RR; ++b) acc[a][b] = -0.0f;
        for (uint32_t t0 = 0; t0 < d; t0 += KC) {
            const uint32_t tc = min(KC, d - t0);
            __syncthreads();  // the previous chunk's readers are done
#pragma unroll
            for (uint32_t e = 0; e < TQ * KC / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / KC, c = idx % KC;
                const uint32_t q = q0 + r;
                qs[c][r] = (q < nq && c < tc) ? Q[(size_t)q * d + t0 + c] : 0.0f;
            }
#pragma unroll
            for (uint32_t e = 0; e < TR * KC / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / KC, c = idx % KC;
                const uint64_t row = row0 + r;
                rs[c][r] = (row < n && c < tc) ? knn_widen(X[row * d + t0 + c]) : 0.0f;
            }
            __syncthreads();
            auto advance = [&](uint32_t t) {
                const float4 qa = *reinterpret_cast<const float4 *>(&qs[t][qg * RQ]);
                const float4 qb = *reinterpret_cast<const float4 *>(&qs[t][qg * RQ + 4]);
                const float4 rv = *reinterpret_cast<const float4 *>(&rs[t][rg * RR]);
                const float qv[RQ] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                const float rr[RR] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
                    for (uint32_t b = 0; b < RR; ++b) acc[a][b] = knn_step<METRIC>(acc[a][b], qv[a], rr[b]);
            };
            if (tc == KC) {  // whole chunk: no per-dimension test (unrolled by 8: fully, the LDS reads of all 32 dimensions
                             // were hoisted into 338 VGPRs -- one wave per SIMD)
#pragma unroll 8
                for (uint32_t t = 0; t < KC; ++t) advance(t);
            } else {         // the last chunk of a d that is not a multiple of 32
                for (uint32_t t = 0; t < tc; ++t) advance(t);
            }
        }
        float rn[RR];
#pragma unroll
        for (uint32_t b = 0; b < RR; ++b) {
            const uint64_t row = row0 + rg * RR + b;
            rn[b] = (vq_is_cos(METRIC) && row < n) ? rnorm[row] : 1.0f;
        }
        const uint64_t rbase = row0 + rg * RR;
        const bool vec = ((n & 3u) == 0) && rbase + RR <= n;
#pragma unroll
        for (uint32_t a = 0; a < RQ; ++a) {
            const uint32_t q = q0 + qg * RQ + a;
            float dv[RR];
#pragma unroll
            for (uint32_t b = 0; b < RR; ++b) {
                dv[b] = knn_finish<METRIC>(acc[a][b], qn[a], rn[b]);
                const uint32_t key = adc_key(dv[b]);
                if (rbase + b < n && key != 0xFFFFFFFFu) {
                    lo[a] = min(lo[a], key);
                    hi[a] = max(hi[a], key);
                }
            }
            if (q >= nq) continue;
            float *dq = dist + (size_t)q * n;
            if (vec) {
                *reinterpret_cast<float4 *>(dq + rbase) = make_float4(dv[0], dv[1], dv[2], dv[3]);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < RR; ++b)
                    if (rbase + b < n) dq[rbase + b] = dv[b];
            }
        }
    }
    // the 16 lanes of a query group (lane bits 0-3) hold all of the workgroup's rows for its 8 queries
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
#pragma unroll
        for (uint32_t off = 1; off < 16; off <<= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], (int)off));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], (int)off));
        }
        const uint32_t q = q0 + qg * RQ + a;
        if (rg == 0 && q < nq && lo[a] <= hi[a]) {
            atomicMin(&kmin[q], lo[a]);
            atomicMax(&kmax[q], hi[a]);
        }
    }
}

// rerank: one workgroup per query computes D for its c candidates (the row of each gathered from the index), sorts the
// (key, row) pairs in LDS and writes the first topk.  An id >= n reads nothing: it sets *err and sorts last.
template <int METRIC, typename RT>
__global__ __launch_bounds__(1024) void k_knn_rerank(const float *__restrict__ Q, const RT *__restrict__ X, uint64_t n, uint32_t d,
                                                     const float *__restrict__ qnorm, const float *__restrict__ rnorm,
                                                     const uint32_t *__restrict__ cand, uint32_t c, uint32_t topk,
                                                     uint32_t *__restrict__ idx_out, float *__restrict__ dist_out,
                                                     uint32_t *__restrict__ err) {
    __shared__ unsigned long long buf[kKnnRerankMax];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const float *x = Q + (size_t)q * d;
    const float qn = vq_is_cos(METRIC) ? qnorm[q] : 1.0f;
    uint32_t len = 2;
    while (len < c) len <<= 1;
    for (uint32_t e = tid; e < len; e += 1024) {
        unsigned long long w = ~0ull;
        if (e < c) {
            const uint32_t id = cand[(size_t)q * c + e];
            if (id >= n) {
                atomicOr(err, 1u);
            } else {
                const RT *r = X + (size_t)id * d;
                float acc = -0.0f;
                for (uint32_t t = 0; t < d; ++t) acc = knn_step<METRIC>(acc, x[t], knn_widen(r[t]));
                const float dv = knn_finish<METRIC>(acc, qn, vq_is_cos(METRIC) ? rnorm[id] : 1.0f);
                w = ((unsigned long long)adc_key(dv) << 32) | id;
            }
        }
        buf[e] = w;
    }
    adc_bitonic<1024>(buf, len);
    for (uint32_t e = tid; e < topk; e += 1024) adc_emit(buf[e], true, 0, idx_out + (size_t)q * topk + e, dist_out + (size_t)q * topk + e);
}

template <int METRIC, typename RT>
int knn_dist_launch(const float *Q, uint32_t nq, const RT *X, uint64_t n, uint32_t d, const float *qnorm, const float *rnorm,
                    float *dist, uint32_t *kmin, uint32_t *kmax, hipStream_t stream) {
    const uint32_t nqt = (nq + kKnnTQ - 1) / kKnnTQ;
    const uint64_t nrt = (n + kKnnTR - 1) / kKnnTR;
    // about eight workgroups per CU in all, each a column of row tiles for one query tile
    const uint64_t per_qt = std::max<uint64_t>(1, std::min<uint64_t>(nrt, ((uint64_t)num_cus() * 8 + nqt - 1) / nqt));
    hipLaunchKernelGGL((k_knn_dist<METRIC, RT>), dim3((uint32_t)(per_qt * nqt)), dim3(256), 0, stream, Q, nq, X, n, d, qnorm,
                       rnorm, nqt, nrt, dist, kmin, kmax);
    VQ_LAUNCH_CHECK("k_knn_dist");
    return VQHIP_OK;
}

template <int METRIC, typename RT>
int knn_rerank_launch(const float *Q, uint32_t nq, const RT *X, uint64_t n, uint32_t d, const float *qnorm, const float *rnorm,
                      const uint32_t *cand, uint32_t c, uint32_t topk, uint32_t *idx_out, float *dist_out, uint32_t *err,
                      hipStream_t stream) {
    hipLaunchKernelGGL((k_knn_rerank<METRIC, RT>), dim3(nq), dim3(1024), 0, stream, Q, X, n, d, qnorm, rnorm, cand, c, topk,
                       idx_out, dist_out, err);
    VQ_LAUNCH_CHECK("k_knn_rerank");
    return VQHIP_OK;
}

// METRIC and the row type as template arguments of F (a generic lambda called with two tags)
template <class F>
int knn_dispatch(int metric, int dtype, F &&f) {
    auto by_type = [&](auto mtag) -> int {
        if (dtype == 1) return f(mtag, (const uint16_t *)nullptr);
        return f(mtag, (const float *)nullptr);
    };
    switch (metric) {
        case VQHIP_SQUARED_EUCLIDEAN: return by_type(std::integral_constant<int, VQHIP_SQUARED_EUCLIDEAN>());
        case VQHIP_EUCLIDEAN: return by_type(std::integral_constant<int, VQHIP_EUCLIDEAN>());
        case VQHIP_MANHATTAN: return by_type(std::integral_constant<int, VQHIP_MANHATTAN>());
        case VQHIP_COSINE: return by_type(std::integral_constant<int, VQHIP_COSINE>());
        case VQHIP_COSINE_UNCLAMPED: return by_type(std::integral_constant<int, VQHIP_COSINE_UNCLAMPED>());
    }
    return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
}

}  // namespace

int launch_knn_norms(const void *X, int dtype, uint64_t n, uint32_t d, float *out, hipStream_t stream) {
    if (n == 0) return VQHIP_OK;
    if (dtype == 1)
        hipLaunchKernelGGL(k_knn_norms<uint16_t>, dim3(knn_grid(n, 8)), dim3(256), 0, stream, (const uint16_t *)X, n, d, out);
    else
        hipLaunchKernelGGL(k_knn_norms<float>, dim3(knn_grid(n, 8)), dim3(256), 0, stream, (const float *)X, n, d, out);
    VQ_LAUNCH_CHECK("k_knn_norms");
    return VQHIP_OK;
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

// queries_dev [nq][d] f32, qnorm_dev [nq] (cosine; launch_knn_norms), workspaces sized for knn_query_batch(n, nq) queries:
// dist_ws >= qb * n floats, state_ws >= knn_state_bytes(qb), cand_ws >= topk_cand_bytes(qb); outputs [nq][topk] on the device
int launch_knn_search(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                      unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, hipStream_t stream) {
    if (topk == 0 || topk > 1024 || topk > n) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, min(n, 1024)]");
    const uint32_t qb = knn_query_batch(n, nq);
    uint32_t *kmin = reinterpret_cast<uint32_t *>(state_ws);
    uint32_t *kmax = kmin + qb;
    const TopkState st = topk_state(kmax + qb, qb);
    const KnnSource src{{dist_ws, n}, kmin, kmax};
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0);
        const float *Qb = queries_dev + (size_t)q0 * d;
        const float *qn = qnorm_dev ? qnorm_dev + q0 : nullptr;
        VQ_HIP(hipMemsetAsync(kmin, 0xFF, (size_t)qb * 4, stream));
        VQ_HIP(hipMemsetAsync(kmax, 0, knn_state_bytes(qb) - (size_t)qb * 4, stream));
        VQ_TRY(knn_dispatch(metric, dtype, [&](auto mtag, auto rtag) -> int {
            using RT = std::remove_const_t<std::remove_pointer_t<decltype(rtag)>>;
            return knn_dist_launch<decltype(mtag)::value, RT>(Qb, nb, reinterpret_cast<const RT *>(X), n, d, qn, rnorm, dist_ws,
                                                             kmin, kmax, stream);
        }));
        hipLaunchKernelGGL(k_knn_hist, dim3(src.blocks(), nb), dim3(256), 0, stream, dist_ws, n, kmin, kmax, st.hist);
        VQ_LAUNCH_CHECK("k_knn_hist");
        VQ_TRY(launch_topk_select(src, nb, topk, 0, st, cand_ws, idx_out_dev + (size_t)q0 * topk, dist_out_dev + (size_t)q0 * topk,
                                  stream));
    }
    return VQHIP_OK;
}

size_t range_ws_bytes(uint64_t n, uint32_t nq) { return range_ws_size(n, knn_query_batch(n, nq)); }

// launch_knn_search with the range stage behind the distances: per batch k_knn_dist, then count -> scan -> (host: total,
// cap, room) -> fill (range.hpp).  radii_dev [nq]; *out is complete when this returns.
int launch_knn_range(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                     const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results, float *dist_ws,
                     void *state_ws, void *range_ws, RangeOut *out, hipStream_t stream) {
    if (max_results == 0) return fail(VQHIP_ERR_INVALID_INPUT, "max_results must be at least 1");
    const uint32_t qb = knn_query_batch(n, nq);
    uint32_t *kmin = reinterpret_cast<uint32_t *>(state_ws);  // written by k_knn_dist, not read here
    uint32_t *kmax = kmin + qb;
    VQ_TRY(range_begin(out, nq, max_results, stream));
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0);
        const float *Qb = queries_dev + (size_t)q0 * d;
        const float *qn = qnorm_dev ? qnorm_dev + q0 : nullptr;
        VQ_TRY(knn_dispatch(metric, dtype, [&](auto mtag, auto rtag) -> int {
            using RT = std::remove_const_t<std::remove_pointer_t<decltype(rtag)>>;
            return knn_dist_launch<decltype(mtag)::value, RT>(Qb, nb, reinterpret_cast<const RT *>(X), n, d, qn, rnorm, dist_ws,
                                                             kmin, kmax, stream);
        }));
        VQ_TRY(range_batch(dist_ws, n, nb, q0, radii_dev + q0, range_ws, max_results, out, stream));
    }
    VQ_HIP(hipStreamSynchronize(stream));
    return VQHIP_OK;
}

// cand_dev [nq][c] row ids, 1 <= c <= 4096, topk <= c; *err_dev |= 1 where an id is >= n (the caller zeroes it first)
int launch_knn_rerank(int metric, const void *X, int dtype, uint64_t n, uint32_t d, const float *rnorm, const float *queries_dev,
                      const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c, uint32_t topk,
                      uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    if (c == 0 || c > kKnnRerankMax) return fail(VQHIP_ERR_INVALID_INPUT, "candidates per query must be in [1, %u]", kKnnRerankMax);
    if (topk == 0 || topk > c) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, candidates]");
    if (nq == 0) return VQHIP_OK;
    return knn_dispatch(metric, dtype, [&](auto mtag, auto rtag) -> int {
        using RT = std::remove_const_t<std::remove_pointer_t<decltype(rtag)>>;
        return knn_rerank_launch<decltype(mtag)::value, RT>(queries_dev, nq, reinterpret_cast<const RT *>(X), n, d, qnorm_dev,
                                                           rnorm, cand_dev, c, topk, idx_out_dev, dist_out_dev, err_dev, stream);
    });
}

}  // namespace vqhip
