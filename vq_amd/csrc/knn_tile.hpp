// knn_tile.hpp -- the exact distance passes over resident rows, each written once: dense f32 / f16 rows (k_knn.hip) and
// u8 SQ codes (k_sqindex.hip; SqRows of sq_decode.hpp) go through the same kernels, and the inverted-file tiles
// (ivf_tile.hpp) through the same tile pass.  The tile shape, one pair's arithmetic (the operation order of
// Distance::compute), the row source of dense rows, the tile pass and the key range behind it, the three kernels
// (k_knn_dist, k_knn_rerank, k_knn_norms) with their batched host drivers, the key-space histogram over the distances and
// the source it makes of them for the selection stage (topk.hpp).
// A row source ROWS is the only code that knows how a row leaves global memory.  It holds {X, d, sc} (Elem *, the
// dimensions, Scale: what a kernel takes beside the pointer) and offers two operations:
//   fill(rs, row0, nvalid, t0, tc)   dimensions [t0, t0 + tc) of rows row0 .. row0 + 63 into the transposed LDS chunk; a
//                                    load is issued only where its row is below nvalid and its first dimension below tc,
//                                    everything else becomes 0.0f
//   walk(row, t0, tc, vec, f)        f(t, value) for t = t0 .. t0 + tc - 1 ascending
//   row(j)                           the row of X behind row j of the source: j itself, but for a picked source
//   fill_rows(rs, row_of, ...)       fill with tile row r read from row row_of(r) of X: the loader itself, written once
// ROWS::Walk is the type the one-row-per-lane kernels are instantiated with (a source whose walk is the same code).
// Every including file gets its own copy of the kernels (an anonymous namespace: no relocatable device code); each .hip
// instantiates what it launches.
#pragma once
#include "kernels.hpp"
#include "range.hpp"
#include "topk.hpp"

#include <algorithm>
#include <type_traits>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

constexpr uint32_t kKnnRQ = 8, kKnnRR = 4;                  // (query, row) pairs per lane
constexpr uint32_t kKnnTQ = 16 * kKnnRQ, kKnnTR = 16 * kKnnRR; // tile: 16 query groups x 16 row groups = 256 lanes
constexpr uint32_t kKnnKC = 32;                              // dimensions per LDS chunk
constexpr uint32_t kKnnRerankMax = 4096;                     // candidates per query of a rerank
constexpr uint32_t kKnnNone = 0xFFFFFFFFu;                   // the query of a tile slot that has none

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

template <typename RT>
__device__ __forceinline__ float knn_widen(RT v) {
    if constexpr (std::is_same<RT, uint16_t>::value) return (float)__builtin_bit_cast(_Float16, v);  // exact
    else return v;
}

// the row source of dense rows X [n][d], RT = float or the bits of an f16 (widened exactly)
template <typename RT>
struct DenseRows {
    using Elem = RT;
    using Walk = DenseRows;
    struct Scale {};
    const RT *X;
    uint32_t d;
    Scale sc;

    // fill with tile row r read from row row_of(r) of X (asked only for r < nvalid): the one loader behind fill and the
    // picked form of the source (PickedRows, ivf_tile.hpp)
    template <class RF>
    __device__ __forceinline__ void fill_rows(float (&rs)[kKnnKC][kKnnTR + 4], RF &&row_of, uint32_t nvalid, uint32_t t0,
                                              uint32_t tc) const {
#pragma unroll
        for (uint32_t e = 0; e < kKnnTR * kKnnKC / 256; ++e) {
            const uint32_t idx = threadIdx.x + 256 * e, r = idx / kKnnKC, c = idx % kKnnKC;
            rs[c][r] = (r < nvalid && c < tc) ? knn_widen(X[row_of(r) * d + t0 + c]) : 0.0f;
        }
    }
    __device__ __forceinline__ void fill(float (&rs)[kKnnKC][kKnnTR + 4], uint64_t row0, uint32_t nvalid, uint32_t t0,
                                         uint32_t tc) const {
        fill_rows(rs, [&](uint32_t r) { return row0 + r; }, nvalid, t0, tc);
    }
    // the row of X behind row j of the source (what a kernel indexes the rows' norms with)
    __device__ __forceinline__ uint64_t row(uint64_t j) const { return j; }
    // vec: four elements per load (8 or 16 bytes); d, t0 and tc are multiples of 4 then
    template <class F>
    __device__ __forceinline__ void walk(uint64_t row, uint32_t t0, uint32_t tc, bool vec, F &&f) const {
        const RT *r = X + row * d + t0;
        if (vec) {
            for (uint32_t t = 0; t < tc; t += 4) {
                float v[4];
                if constexpr (std::is_same<RT, uint16_t>::value) {
                    const uint2 w = *reinterpret_cast<const uint2 *>(r + t);
                    v[0] = knn_widen((uint16_t)(w.x & 0xFFFFu)), v[1] = knn_widen((uint16_t)(w.x >> 16));
                    v[2] = knn_widen((uint16_t)(w.y & 0xFFFFu)), v[3] = knn_widen((uint16_t)(w.y >> 16));
                } else {
                    const float4 w = *reinterpret_cast<const float4 *>(r + t);
                    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) f(t0 + t + j, v[j]);
            }
        } else {
            for (uint32_t t = 0; t < tc; ++t) f(t0 + t, knn_widen(r[t]));
        }
    }
};

// The tile pass: acc[a][b] = the running sum of the pair (query slot qg * 8 + a, row row0 + rg * 4 + b) over all d
// dimensions, from -0.0f, ascending, one unfused knn_step per dimension.  The tile's query and row elements pass through
// LDS 32 dimensions at a time (transposed: lane (qg, rg) reads its 8 query and 4 row elements of dimension t as two +
// one 16-byte LDS reads; +4: the loaders' column-major writes spread over the banks).  query_of(slot) is the query of
// tile slot 0 .. 127 or kKnnNone.  Padded queries, rows and dimensions are 0.0f in the tile; a padded dimension is not
// summed (the loops stop at tc), what a padded query or row sums is for the caller to drop.
template <int METRIC, class ROWS, class QF>
__device__ __forceinline__ void knn_tile_pass(float (&acc)[kKnnRQ][kKnnRR], float (&qs)[kKnnKC][kKnnTQ + 4],
                                              float (&rs)[kKnnKC][kKnnTR + 4], const float *__restrict__ Q, QF &&query_of,
                                              const ROWS &rows, uint64_t row0, uint32_t nvalid) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, KC = kKnnKC;
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4, d = rows.d;
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
        for (uint32_t b = 0; b < RR; ++b) acc[a][b] = -0.0f;
    for (uint32_t t0 = 0; t0 < d; t0 += KC) {
        const uint32_t tc = min(KC, d - t0);
        __syncthreads();  // the previous chunk's readers are done
        // a lane loads dimension c of the tile slots tid / KC + 8 e.  Said per lane, not per load from tid + 256 e: that
        // form kept 16 addresses alive across the pair loop and cost the 16-byte SQ tiles their third wave
        const uint32_t c = tid % KC;
        const float *qc = Q + t0 + c;
#pragma unroll
        for (uint32_t e = 0; e < TQ * KC / 256; ++e) {
            const uint32_t r = tid / KC + (256 / KC) * e, q = query_of(r);
            qs[c][r] = (q != kKnnNone && c < tc) ? qc[(size_t)q * d] : 0.0f;
        }
        rows.fill(rs, row0, nvalid, t0, tc);
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
}

// The key range behind a tile kernel: the 16 lanes of a query group (lane bits 0-3) hold all of the workgroup's rows for
// its 8 queries query(a) (kKnnNone: none); lo / hi [a] the range of the non-NaN keys the lane saw.  Two atomics per
// workgroup and query.
template <class QA>
__device__ __forceinline__ void knn_key_range(uint32_t (&lo)[kKnnRQ], uint32_t (&hi)[kKnnRQ], QA &&query, uint32_t *__restrict__ kmin,
                                              uint32_t *__restrict__ kmax) {
#pragma unroll
    for (uint32_t a = 0; a < kKnnRQ; ++a) {
#pragma unroll
        for (uint32_t off = 1; off < 16; off <<= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], (int)off));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], (int)off));
        }
        const uint32_t q = query(a);
        if ((threadIdx.x & 15u) == 0 && q != kKnnNone && lo[a] <= hi[a]) {
            atomicMin(&kmin[q], lo[a]);
            atomicMax(&kmax[q], hi[a]);
        }
    }
}

// sqrtf(sum_t x_t^2) per row, sequential from -0.0f (the norm chains of exact_distance_rt)
template <class ROWS>
__global__ __launch_bounds__(256) void k_knn_norms(const typename ROWS::Elem *__restrict__ X, uint64_t n, uint32_t d,
                                                   typename ROWS::Scale sc, float *__restrict__ out) {
    const ROWS rows{X, d, sc};
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        float s = -0.0f;
        rows.walk(i, 0, d, false, [&](uint32_t, float v) {
            const float p = v * v;
            s = s + p;
        });
        out[i] = sqrtf(s);
    }
}

// The row mask of row tile rt (rows rt * 64 .. + nvalid) as two words, bits at or past nvalid cleared.  The mask has
// ceil(n / 32) words and is 4-byte aligned: two u32 reads, and the second only where the tile reaches past 32 rows (for
// n = 33, 65 or 96 the last tile's second word does not exist).  Workgroup-uniform.
__device__ __forceinline__ void knn_tile_mask(const uint32_t *__restrict__ mask, uint64_t rt, uint32_t nvalid, uint32_t &w0,
                                              uint32_t &w1) {
    w0 = mask[2 * rt];
    w1 = nvalid > 32 ? mask[2 * rt + 1] : 0u;
    if (nvalid < 32) w0 &= (1u << nvalid) - 1u;
    else if (nvalid > 32 && nvalid < 64) w1 &= (1u << (nvalid - 32)) - 1u;
}

// dist[q][i] for the batch's nq queries.  Workgroup b owns query tile b % nqt and strides over the row tiles
// b / nqt, b / nqt + gridDim.x / nqt, ... (gridDim.x is a multiple of nqt): the workgroups in flight at one time share
// row tiles, so the rows come from HBM about once per call and from L2 for the other query tiles.  A padded row's
// distance is not written, nor does it enter the key range.
// kmin / kmax [nq]: the range of the non-NaN keys of each query (atomics, once per workgroup and query).
// MASKED (k_knn_dist_masked; mask: the call's row mask): a tile reads its two mask words first and, with no allowed row
// below n, is left at once -- no tile pass, no rnorm, no store: its slots of dist keep what an earlier batch or call left
// there, which is why everything behind a masked kernel reads the mask before a distance.  A tile with an allowed row is
// computed and stored whole; only allowed rows enter the key range.
template <int METRIC, class ROWS, bool MASKED>
__device__ __forceinline__ void knn_dist_body(const float *__restrict__ Q, uint32_t nq, const typename ROWS::Elem *__restrict__ X,
                                              uint64_t n, uint32_t d, typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                              const float *__restrict__ rnorm, uint32_t nqt, uint64_t nrt, float *__restrict__ dist,
                                              uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax,
                                              const uint32_t *__restrict__ mask) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, KC = kKnnKC;
    __shared__ __attribute__((aligned(16))) float qs[KC][TQ + 4];
    __shared__ __attribute__((aligned(16))) float rs[KC][TR + 4];
    const ROWS rows{X, d, sc};
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4;
    const uint32_t q0 = (blockIdx.x % nqt) * TQ;
    const uint64_t rstep = gridDim.x / nqt;
    auto query_of = [&](uint32_t slot) { return q0 + slot < nq ? q0 + slot : kKnnNone; };
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
        const uint32_t nvalid = (uint32_t)min((uint64_t)TR, n - row0);
        uint32_t ok = 0xFu;  // MASKED: the mask bits of this lane's four rows
        if constexpr (MASKED) {
            uint32_t w0, w1;
            knn_tile_mask(mask, rt, nvalid, w0, w1);
            if ((w0 | w1) == 0u) continue;  // (uniform) nothing allowed in this tile
            ok = ((rg < 8 ? w0 : w1) >> ((rg & 7u) * 4)) & 0xFu;
        }
        float acc[RQ][RR];
        knn_tile_pass<METRIC>(acc, qs, rs, Q, query_of, rows, row0, nvalid);
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
                bool in = rbase + b < n && key != 0xFFFFFFFFu;
                if constexpr (MASKED) in = in && ((ok >> b) & 1u);
                if (in) {
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
    knn_key_range(lo, hi, [&](uint32_t a) { return query_of(qg * RQ + a); }, kmin, kmax);
}

template <int METRIC, class ROWS>
__global__ __launch_bounds__(256) void k_knn_dist(const float *__restrict__ Q, uint32_t nq, const typename ROWS::Elem *__restrict__ X,
                                                  uint64_t n, uint32_t d, typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                                  const float *__restrict__ rnorm, uint32_t nqt, uint64_t nrt, float *__restrict__ dist,
                                                  uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    knn_dist_body<METRIC, ROWS, false>(Q, nq, X, n, d, sc, qnorm, rnorm, nqt, nrt, dist, kmin, kmax, nullptr);
}

template <int METRIC, class ROWS>
__global__ __launch_bounds__(256) void k_knn_dist_masked(const float *__restrict__ Q, uint32_t nq,
                                                         const typename ROWS::Elem *__restrict__ X, uint64_t n, uint32_t d,
                                                         typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                                         const float *__restrict__ rnorm, uint32_t nqt, uint64_t nrt,
                                                         float *__restrict__ dist, uint32_t *__restrict__ kmin,
                                                         uint32_t *__restrict__ kmax, const uint32_t *__restrict__ mask) {
    knn_dist_body<METRIC, ROWS, true>(Q, nq, X, n, d, sc, qnorm, rnorm, nqt, nrt, dist, kmin, kmax, mask);
}

// rerank: one workgroup per query computes D for its c candidates (the row of each gathered from the index, one
// candidate per lane and pass), sorts the (key, row) pairs in LDS and writes the first topk.  An id >= n reads nothing:
// it sets *err and sorts last.
template <int METRIC, class ROWS>
__global__ __launch_bounds__(1024) void k_knn_rerank(const float *__restrict__ Q, const typename ROWS::Elem *__restrict__ X, uint64_t n,
                                                     uint32_t d, typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                                     const float *__restrict__ rnorm, const uint32_t *__restrict__ cand, uint32_t c,
                                                     uint32_t topk, uint32_t *__restrict__ idx_out, float *__restrict__ dist_out,
                                                     uint32_t *__restrict__ err) {
    __shared__ unsigned long long buf[kKnnRerankMax];
    const ROWS rows{X, d, sc};
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
                rows.walk(id, 0, d, false, [&](uint32_t t, float v) { acc = knn_step<METRIC>(acc, x[t], v); });
                const float dv = knn_finish<METRIC>(acc, qn, vq_is_cos(METRIC) ? rnorm[id] : 1.0f);
                w = ((unsigned long long)adc_key(dv) << 32) | id;
            }
        }
        buf[e] = w;
    }
    adc_bitonic<1024>(buf, len);
    for (uint32_t e = tid; e < topk; e += 1024) adc_emit(buf[e], true, 0, idx_out + (size_t)q * topk + e, dist_out + (size_t)q * topk + e);
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

// k_knn_hist over the allowed rows only, four consecutive rows per lane: their mask bits are read first, and the distances
// of a group without an allowed row not at all
__attribute__((unused)) __global__ __launch_bounds__(256) void k_knn_hist_masked(const float *__restrict__ dist, uint64_t n,
                                                                                 const uint32_t *__restrict__ kmin,
                                                                                 const uint32_t *__restrict__ kmax,
                                                                                 const uint32_t *__restrict__ mask,
                                                                                 uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[kAdcBins];
    const uint32_t q = blockIdx.y, lo = kmin[q], hi = kmax[q];
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256) h[e] = 0u;
    __syncthreads();
    const float *dq = dist + (size_t)q * n;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (uint64_t)gridDim.x * 1024) {
        const uint32_t ok = (mask[i0 >> 5] >> (uint32_t)(i0 & 31u)) & 0xFu;
        if (ok == 0) continue;
        float v[4];
        masked_load4(dq, n, i0, ok, v);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (((ok >> j) & 1u) && i0 + j < n) atomicAdd(&h[knn_bin(adc_key(v[j]), lo, hi)], 1u);
    }
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

// KnnSource under a row mask: the allowed rows only (MaskedRows, topk.hpp)
struct MaskedKnnSource : MaskedRows {
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

// METRIC as a template argument of F (a generic lambda called with a tag)
template <class F>
int knn_metric_dispatch(int metric, F &&f) {
    switch (metric) {
        case VQHIP_SQUARED_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_SQUARED_EUCLIDEAN>());
        case VQHIP_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_EUCLIDEAN>());
        case VQHIP_MANHATTAN: return f(std::integral_constant<int, VQHIP_MANHATTAN>());
        case VQHIP_COSINE: return f(std::integral_constant<int, VQHIP_COSINE>());
        case VQHIP_COSINE_UNCLAMPED: return f(std::integral_constant<int, VQHIP_COSINE_UNCLAMPED>());
    }
    return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
}

// f(the row source of X [.][d], dtype 0: f32, 1: f16 bits)
template <class F>
int knn_dense_rows(const void *X, int dtype, uint32_t d, F &&f) {
    if (dtype == 1) return f(DenseRows<uint16_t>{(const uint16_t *)X, d, {}});
    return f(DenseRows<float>{(const float *)X, d, {}});
}

template <class ROWS>
int knn_norms_rows(const ROWS &rows, uint64_t n, float *out, hipStream_t stream) {
    if (n == 0) return VQHIP_OK;
    hipLaunchKernelGGL(k_knn_norms<typename ROWS::Walk>, dim3(knn_grid(n, 8)), dim3(256), 0, stream, rows.X, n, rows.d, rows.sc, out);
    VQ_LAUNCH_CHECK("k_knn_norms");
    return VQHIP_OK;
}

// The batched driver of a search over resident rows: per batch of knn_query_batch(n, nq) queries (their [batch][n] f32
// distances under 1 GB) k_knn_dist into dist_ws, the key range into kmin | kmax at the head of state_ws (reset first
// where the stage reads it), then stage(q0, nb, kmin, kmax).  mask: the row mask of a filtered call on the device (ceil(n /
// 32) words; k_knn_dist_masked), NULL for every row (k_knn_dist).
template <class ROWS, class STAGE>
int knn_batches(int metric, const ROWS &rows, uint64_t n, const float *rnorm, const float *queries_dev, const float *qnorm_dev,
                uint32_t nq, float *dist_ws, void *state_ws, bool reset, const uint32_t *mask, hipStream_t stream, STAGE &&stage) {
    const uint32_t qb = knn_query_batch(n, nq), d = rows.d;
    uint32_t *kmin = reinterpret_cast<uint32_t *>(state_ws);
    uint32_t *kmax = kmin + qb;
    const uint64_t nrt = (n + kKnnTR - 1) / kKnnTR;
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0), nqt = (nb + kKnnTQ - 1) / kKnnTQ;
        const float *Qb = queries_dev + (size_t)q0 * d;
        const float *qn = qnorm_dev ? qnorm_dev + q0 : nullptr;
        if (reset) {
            VQ_HIP(hipMemsetAsync(kmin, 0xFF, (size_t)qb * 4, stream));
            VQ_HIP(hipMemsetAsync(kmax, 0, knn_state_bytes(qb) - (size_t)qb * 4, stream));
        }
        // about eight workgroups per CU in all, each a column of row tiles for one query tile
        const uint64_t per_qt = std::max<uint64_t>(1, std::min<uint64_t>(nrt, ((uint64_t)num_cus() * 8 + nqt - 1) / nqt));
        VQ_TRY(knn_metric_dispatch(metric, [&](auto mtag) -> int {
            if (mask)
                hipLaunchKernelGGL((k_knn_dist_masked<decltype(mtag)::value, ROWS>), dim3((uint32_t)(per_qt * nqt)), dim3(256), 0, stream,
                                   Qb, nb, rows.X, n, d, rows.sc, qn, rnorm, nqt, nrt, dist_ws, kmin, kmax, mask);
            else
                hipLaunchKernelGGL((k_knn_dist<decltype(mtag)::value, ROWS>), dim3((uint32_t)(per_qt * nqt)), dim3(256), 0, stream, Qb, nb,
                                   rows.X, n, d, rows.sc, qn, rnorm, nqt, nrt, dist_ws, kmin, kmax);
            VQ_LAUNCH_CHECK("k_knn_dist");
            return VQHIP_OK;
        }));
        VQ_TRY(stage(q0, nb, kmin, kmax));
    }
    return VQHIP_OK;
}

// queries_dev [nq][d] f32, qnorm_dev [nq] (cosine; launch_knn_norms), workspaces sized for knn_query_batch(n, nq) queries:
// dist_ws >= qb * n floats, state_ws >= knn_state_bytes(qb), cand_ws >= topk_cand_bytes(qb); outputs [nq][topk] on the device.
// mask_dev: the row mask of a filtered search (the allowed rows only, padding behind fewer than topk of them) or NULL.
template <class ROWS>
int knn_search_rows(int metric, const ROWS &rows, uint64_t n, const float *rnorm, const float *queries_dev, const float *qnorm_dev,
                    uint32_t nq, uint32_t topk, float *dist_ws, void *state_ws, unsigned long long *cand_ws, uint32_t *idx_out_dev,
                    float *dist_out_dev, const uint32_t *mask_dev, hipStream_t stream) {
    if (topk == 0 || topk > 1024 || topk > n) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, min(n, 1024)]");
    const uint32_t qb = knn_query_batch(n, nq);
    return knn_batches(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, dist_ws, state_ws, true, mask_dev, stream,
                       [&](uint32_t q0, uint32_t nb, uint32_t *kmin, uint32_t *kmax) -> int {
        const TopkState st = topk_state(kmax + qb, qb);
        if (mask_dev) {
            const MaskedKnnSource src{{{dist_ws, n}, mask_dev}, kmin, kmax};
            hipLaunchKernelGGL(k_knn_hist_masked, dim3(src.blocks(), nb), dim3(256), 0, stream, dist_ws, n, kmin, kmax, mask_dev, st.hist);
            VQ_LAUNCH_CHECK("k_knn_hist_masked");
            return launch_topk_select(src, nb, topk, 0, st, cand_ws, idx_out_dev + (size_t)q0 * topk, dist_out_dev + (size_t)q0 * topk,
                                      stream);
        }
        const KnnSource src{{dist_ws, n}, kmin, kmax};
        hipLaunchKernelGGL(k_knn_hist, dim3(src.blocks(), nb), dim3(256), 0, stream, dist_ws, n, kmin, kmax, st.hist);
        VQ_LAUNCH_CHECK("k_knn_hist");
        return launch_topk_select(src, nb, topk, 0, st, cand_ws, idx_out_dev + (size_t)q0 * topk, dist_out_dev + (size_t)q0 * topk,
                                  stream);
    });
}

// knn_search_rows with the range stage behind the distances: per batch k_knn_dist, then count -> scan -> (host: total,
// cap, room) -> fill (range.hpp).  radii_dev [nq]; the kmin / kmax k_knn_dist writes are not read; *out is complete when
// this returns.  mask_dev: the row mask of a filtered call (only allowed rows hit) or NULL.
template <class ROWS>
int knn_range_rows(int metric, const ROWS &rows, uint64_t n, const float *rnorm, const float *queries_dev, const float *qnorm_dev,
                   uint32_t nq, const float *radii_dev, uint64_t max_results, float *dist_ws, void *state_ws, void *range_ws,
                   RangeOut *out, const uint32_t *mask_dev, hipStream_t stream) {
    if (max_results == 0) return fail(VQHIP_ERR_INVALID_INPUT, "max_results must be at least 1");
    VQ_TRY(range_begin(out, nq, max_results, stream));
    VQ_TRY(knn_batches(metric, rows, n, rnorm, queries_dev, qnorm_dev, nq, dist_ws, state_ws, false, mask_dev, stream,
                       [&](uint32_t q0, uint32_t nb, uint32_t *, uint32_t *) -> int {
        return range_batch(dist_ws, n, nb, q0, radii_dev + q0, range_ws, max_results, out, stream, mask_dev);
    }));
    VQ_HIP(hipStreamSynchronize(stream));
    return VQHIP_OK;
}

// cand_dev [nq][c] row ids, 1 <= c <= 4096, topk <= c; *err_dev |= 1 where an id is >= n (the caller zeroes it first)
template <class ROWS>
int knn_rerank_rows(int metric, const ROWS &rows, uint64_t n, const float *rnorm, const float *queries_dev, const float *qnorm_dev,
                    uint32_t nq, const uint32_t *cand_dev, uint32_t c, uint32_t topk, uint32_t *idx_out_dev, float *dist_out_dev,
                    uint32_t *err_dev, hipStream_t stream) {
    if (c == 0 || c > kKnnRerankMax) return fail(VQHIP_ERR_INVALID_INPUT, "candidates per query must be in [1, %u]", kKnnRerankMax);
    if (topk == 0 || topk > c) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, candidates]");
    if (nq == 0) return VQHIP_OK;
    return knn_metric_dispatch(metric, [&](auto mtag) -> int {
        hipLaunchKernelGGL((k_knn_rerank<decltype(mtag)::value, typename ROWS::Walk>), dim3(nq), dim3(1024), 0, stream, queries_dev,
                           rows.X, n, rows.d, rows.sc, qnorm_dev, rnorm, cand_dev, c, topk, idx_out_dev, dist_out_dev, err_dev);
        VQ_LAUNCH_CHECK("k_knn_rerank");
        return VQHIP_OK;
    });
}

}  // namespace
}  // namespace vqhip
