// k_sqindex.hip -- exact top-k search and exact rerank over ScalarQuantizer codes resident on the device, one byte per
// dimension, against f32 queries (never quantized).  No reference counterpart; the semantics are include/vqhip.h's:
//   v(c)    = min + (float)c * step for every byte value c (the SQ decode rule, un-fused; codes >= levels included)
//   D(q, i) = Distance::compute(q, v(codes[i])) bit for bit: the arithmetic, its order and the two norms of k_knn.hip over
//             the decoded row, so every result equals the flat index over the dequantized rows, indices and distance bits
// A byte is decoded where it leaves global memory -- on its way into the transposed LDS tile (k_sq_dist) or in registers
// (k_sq_rerank, k_sq_norms) -- by the formula itself: v_cvt_f32_ubyteN takes byte N of a loaded dword straight to f32,
// then one multiply and one add (-ffp-contract=off and the file pragma keep them apart; f32 subnormals are not flushed).
// That is three VALU operations per byte and no LDS traffic; the 256-entry table of sq_decode_lut costs a shift, a mask
// and a scattered ds_read per byte for the same bits.
// Schedule of one search (launch_sq_search), per batch of queries whose [batch][n] f32 distances stay under 1 GB:
//   k_sq_dist      k_knn_dist's tiles (128 queries x 64 rows, 32 dimensions per LDS chunk, an 8 x 4 block of pairs per
//                  lane); the row side of a chunk is 2 KB of codes instead of 8 KB of floats
//   k_knn_hist     the 512-bin key-space histogram per query (knn_tile.hpp)
//   launch_topk_select   the shared selection stage (topk.hpp)
// A range search (launch_sq_range) runs k_sq_dist over the same batches and then the range stage (range.hpp).
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "range.hpp"
#include "sq_decode.hpp"
#include "topk.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// sqrtf(sum_t v(c_t)^2) per row, sequential from -0.0f (the row-norm chain of exact_distance_rt over the decoded row)
template <bool W4>
__global__ __launch_bounds__(256) void k_sq_norms(const uint8_t *__restrict__ C, uint64_t n, uint32_t d, float mn, float step,
                                                  float *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        float s = -0.0f;
        sq_row_walk<W4>(C + i * d, d, mn, step, [&](uint32_t, float v) {
            const float p = v * v;
            s = s + p;
        });
        out[i] = sqrtf(s);
    }
}

// dist[q][i] for the batch's nq queries: k_knn_dist with the rows read as codes.  LW = bytes per load of the row
// loader: 16 (d % 16 == 0 and a 16-byte aligned base), 4 (d % 4 == 0, 4-byte aligned) or 1.  A chunk of a row starts at
// byte row * d + t0 with t0 a multiple of 32, so those conditions align every load; a row's last chunk holds tc < 32
// dimensions, a multiple of LW, and a load is issued only where its first dimension is below tc and its row below n.
// Padded rows and dimensions become 0.0f in the tile and never reach a result: a padded dimension is not summed (the
// loops stop at tc), a padded row's distance is not written, nor does it enter the key range.
template <int METRIC, int LW>
__global__ __launch_bounds__(256) void k_sq_dist(const float *__restrict__ Q, uint32_t nq, const uint8_t *__restrict__ C, uint64_t n,
                                                 uint32_t d, float mn, float step, const float *__restrict__ qnorm,
                                                 const float *__restrict__ rnorm, uint32_t nqt, uint64_t nrt, float *__restrict__ dist,
                                                 uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, KC = kKnnKC;
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
            if constexpr (LW == 16) {  // 64 rows x two 16-byte halves: the first 128 lanes
                if (tid < TR * KC / 16) {
                    const uint32_t r = tid >> 1, c0 = (tid & 1u) * 16;
                    const uint64_t row = row0 + r;
                    const bool ok = row < n && c0 < tc;
                    uint4 w = make_uint4(0, 0, 0, 0);
                    if (ok) w = *reinterpret_cast<const uint4 *>(C + row * d + t0 + c0);
                    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (uint32_t j = 0; j < 16; ++j)
                        rs[c0 + j][r] = ok ? sq_val((ws[j >> 2] >> (8 * (j & 3))) & 0xffu, mn, step) : 0.0f;
                }
            } else if constexpr (LW == 4) {  // 64 rows x eight dwords: two per lane
#pragma unroll
                for (uint32_t e = 0; e < TR * KC / 4 / 256; ++e) {
                    const uint32_t idx = tid + 256 * e, r = idx / (KC / 4), c0 = (idx % (KC / 4)) * 4;
                    const uint64_t row = row0 + r;
                    const bool ok = row < n && c0 < tc;
                    uint32_t w = 0;
                    if (ok) w = *reinterpret_cast<const uint32_t *>(C + row * d + t0 + c0);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) rs[c0 + j][r] = ok ? sq_val((w >> (8 * j)) & 0xffu, mn, step) : 0.0f;
                }
            } else {
#pragma unroll
                for (uint32_t e = 0; e < TR * KC / 256; ++e) {
                    const uint32_t idx = tid + 256 * e, r = idx / KC, c = idx % KC;
                    const uint64_t row = row0 + r;
                    rs[c][r] = (row < n && c < tc) ? sq_val(C[row * d + t0 + c], mn, step) : 0.0f;
                }
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
            if (tc == KC) {  // whole chunk: no per-dimension test (unrolled by 8, as k_knn_dist: two waves per SIMD)
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

// rerank: k_knn_rerank with the candidate's row read as codes and decoded in registers.  One workgroup per query, one
// candidate per lane and pass; an id >= n reads nothing: it sets *err and sorts last.
template <int METRIC, bool W4>
__global__ __launch_bounds__(1024) void k_sq_rerank(const float *__restrict__ Q, const uint8_t *__restrict__ C, uint64_t n, uint32_t d,
                                                    float mn, float step, const float *__restrict__ qnorm,
                                                    const float *__restrict__ rnorm, const uint32_t *__restrict__ cand, uint32_t c,
                                                    uint32_t topk, uint32_t *__restrict__ idx_out, float *__restrict__ dist_out,
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
                float acc = -0.0f;
                sq_row_walk<W4>(C + (size_t)id * d, d, mn, step, [&](uint32_t t, float v) { acc = knn_step<METRIC>(acc, x[t], v); });
                const float dv = knn_finish<METRIC>(acc, qn, vq_is_cos(METRIC) ? rnorm[id] : 1.0f);
                w = ((unsigned long long)adc_key(dv) << 32) | id;
            }
        }
        buf[e] = w;
    }
    adc_bitonic<1024>(buf, len);
    for (uint32_t e = tid; e < topk; e += 1024) adc_emit(buf[e], true, 0, idx_out + (size_t)q * topk + e, dist_out + (size_t)q * topk + e);
}

// METRIC as a template argument of F (a generic lambda called with a tag)
template <class F>
int sq_dispatch(int metric, F &&f) {
    switch (metric) {
        case VQHIP_SQUARED_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_SQUARED_EUCLIDEAN>());
        case VQHIP_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_EUCLIDEAN>());
        case VQHIP_MANHATTAN: return f(std::integral_constant<int, VQHIP_MANHATTAN>());
        case VQHIP_COSINE: return f(std::integral_constant<int, VQHIP_COSINE>());
        case VQHIP_COSINE_UNCLAMPED: return f(std::integral_constant<int, VQHIP_COSINE_UNCLAMPED>());
    }
    return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
}

template <int METRIC, int LW>
int sq_dist_launch(const float *Q, uint32_t nq, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *qnorm,
                   const float *rnorm, float *dist, uint32_t *kmin, uint32_t *kmax, hipStream_t stream) {
    const uint32_t nqt = (nq + kKnnTQ - 1) / kKnnTQ;
    const uint64_t nrt = (n + kKnnTR - 1) / kKnnTR;
    // about eight workgroups per CU in all, each a column of row tiles for one query tile (knn_dist_launch)
    const uint64_t per_qt = std::max<uint64_t>(1, std::min<uint64_t>(nrt, ((uint64_t)num_cus() * 8 + nqt - 1) / nqt));
    hipLaunchKernelGGL((k_sq_dist<METRIC, LW>), dim3((uint32_t)(per_qt * nqt)), dim3(256), 0, stream, Q, nq, C, n, d, mn, step, qnorm,
                       rnorm, nqt, nrt, dist, kmin, kmax);
    VQ_LAUNCH_CHECK("k_sq_dist");
    return VQHIP_OK;
}

}  // namespace

int launch_sq_norms(const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, float *out, hipStream_t stream) {
    if (n == 0) return VQHIP_OK;
    if (sq_load_width(C, d) >= 4)
        hipLaunchKernelGGL(k_sq_norms<true>, dim3(knn_grid(n, 8)), dim3(256), 0, stream, C, n, d, mn, step, out);
    else
        hipLaunchKernelGGL(k_sq_norms<false>, dim3(knn_grid(n, 8)), dim3(256), 0, stream, C, n, d, mn, step, out);
    VQ_LAUNCH_CHECK("k_sq_norms");
    return VQHIP_OK;
}

// codes [n][d] u8 on the device, rnorm [n] (cosine; launch_sq_norms), queries_dev [nq][d] f32, qnorm_dev [nq] (cosine;
// launch_knn_norms); the batches and workspaces are launch_knn_search's: dist_ws >= qb * n floats, state_ws >=
// knn_state_bytes(qb), cand_ws >= topk_cand_bytes(qb) for qb = knn_query_batch(n, nq); outputs [nq][topk] on the device
int launch_sq_search(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws,
                     unsigned long long *cand_ws, uint32_t *idx_out_dev, float *dist_out_dev, hipStream_t stream) {
    if (topk == 0 || topk > 1024 || topk > n) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, min(n, 1024)]");
    const uint32_t qb = knn_query_batch(n, nq);
    uint32_t *kmin = reinterpret_cast<uint32_t *>(state_ws);
    uint32_t *kmax = kmin + qb;
    const TopkState st = topk_state(kmax + qb, qb);
    const KnnSource src{{dist_ws, n}, kmin, kmax};
    const int lw = sq_load_width(C, d);
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0);
        const float *Qb = queries_dev + (size_t)q0 * d;
        const float *qn = qnorm_dev ? qnorm_dev + q0 : nullptr;
        VQ_HIP(hipMemsetAsync(kmin, 0xFF, (size_t)qb * 4, stream));
        VQ_HIP(hipMemsetAsync(kmax, 0, knn_state_bytes(qb) - (size_t)qb * 4, stream));
        VQ_TRY(sq_dispatch(metric, [&](auto mtag) -> int {
            constexpr int M = decltype(mtag)::value;
            if (lw == 16) return sq_dist_launch<M, 16>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
            if (lw == 4) return sq_dist_launch<M, 4>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
            return sq_dist_launch<M, 1>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
        }));
        hipLaunchKernelGGL(k_knn_hist, dim3(src.blocks(), nb), dim3(256), 0, stream, dist_ws, n, kmin, kmax, st.hist);
        VQ_LAUNCH_CHECK("k_knn_hist");
        VQ_TRY(launch_topk_select(src, nb, topk, 0, st, cand_ws, idx_out_dev + (size_t)q0 * topk, dist_out_dev + (size_t)q0 * topk,
                                  stream));
    }
    return VQHIP_OK;
}

// launch_sq_search with the range stage behind the distances (launch_knn_range): per batch k_sq_dist, then count -> scan
// -> (host: total, cap, room) -> fill (range.hpp).  range_ws >= range_ws_bytes(n, nq); *out is complete on return.
int launch_sq_range(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                    const float *queries_dev, const float *qnorm_dev, uint32_t nq, const float *radii_dev, uint64_t max_results,
                    float *dist_ws, void *state_ws, void *range_ws, RangeOut *out, hipStream_t stream) {
    if (max_results == 0) return fail(VQHIP_ERR_INVALID_INPUT, "max_results must be at least 1");
    const uint32_t qb = knn_query_batch(n, nq);
    uint32_t *kmin = reinterpret_cast<uint32_t *>(state_ws);  // written by k_sq_dist, not read here
    uint32_t *kmax = kmin + qb;
    const int lw = sq_load_width(C, d);
    VQ_TRY(range_begin(out, nq, max_results, stream));
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0);
        const float *Qb = queries_dev + (size_t)q0 * d;
        const float *qn = qnorm_dev ? qnorm_dev + q0 : nullptr;
        VQ_TRY(sq_dispatch(metric, [&](auto mtag) -> int {
            constexpr int M = decltype(mtag)::value;
            if (lw == 16) return sq_dist_launch<M, 16>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
            if (lw == 4) return sq_dist_launch<M, 4>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
            return sq_dist_launch<M, 1>(Qb, nb, C, n, d, mn, step, qn, rnorm, dist_ws, kmin, kmax, stream);
        }));
        VQ_TRY(range_batch(dist_ws, n, nb, q0, radii_dev + q0, range_ws, max_results, out, stream));
    }
    VQ_HIP(hipStreamSynchronize(stream));
    return VQHIP_OK;
}

// cand_dev [nq][c] row ids, 1 <= c <= 4096, topk <= c; *err_dev |= 1 where an id is >= n (the caller zeroes it first)
int launch_sq_rerank(int metric, const uint8_t *C, uint64_t n, uint32_t d, float mn, float step, const float *rnorm,
                     const float *queries_dev, const float *qnorm_dev, uint32_t nq, const uint32_t *cand_dev, uint32_t c,
                     uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev, uint32_t *err_dev, hipStream_t stream) {
    if (c == 0 || c > kKnnRerankMax) return fail(VQHIP_ERR_INVALID_INPUT, "candidates per query must be in [1, %u]", kKnnRerankMax);
    if (topk == 0 || topk > c) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, candidates]");
    if (nq == 0) return VQHIP_OK;
    const bool w4 = sq_load_width(C, d) >= 4;
    return sq_dispatch(metric, [&](auto mtag) -> int {
        constexpr int M = decltype(mtag)::value;
        if (w4)
            hipLaunchKernelGGL((k_sq_rerank<M, true>), dim3(nq), dim3(1024), 0, stream, queries_dev, C, n, d, mn, step, qnorm_dev, rnorm,
                               cand_dev, c, topk, idx_out_dev, dist_out_dev, err_dev);
        else
            hipLaunchKernelGGL((k_sq_rerank<M, false>), dim3(nq), dim3(1024), 0, stream, queries_dev, C, n, d, mn, step, qnorm_dev, rnorm,
                               cand_dev, c, topk, idx_out_dev, dist_out_dev, err_dev);
        VQ_LAUNCH_CHECK("k_sq_rerank");
        return VQHIP_OK;
    });
}

}  // namespace vqhip
