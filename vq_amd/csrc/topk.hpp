// topk.hpp -- the one exact top-k selection stage behind the ADC full pass (k_adc.hip), the exact k-NN search (k_knn.hip),
// the inverted-file search (k_ivf.hip) and, from the sort on, the binary index (k_binary.hip).  Every including file gets
// its own copy of the kernels (an anonymous namespace: no relocatable device code).
// A scan leaves one f32 distance per (query, position) and a histogram of them, hist[q][kAdcBins].  The result of a query
// is the first topk words (adc_key(D) << 32) | row id, ascending: NaN last, ties to the lower row id, whatever the bins.
//   source              : what a family hands the stage, a small struct passed by value to the kernels:
//                           Pos          the type of a position (uint64_t for dense rows, uint32_t for probed lists)
//                           open(q)      turns the kernel's copy into the view of query q of the batch
//                           count()      the query's positions;  at(pos) the distance;  id(pos) the row id behind it
//                           bin(d)       the histogram bin of a distance (the bin the scan filled hist with)
//                           blocks()     (host) the collect kernel's workgroups per query
//                         TopkRows is the dense part (dist[q][n], id = position) of the ADC and k-NN sources
//                         a masked source (MaskedRows: kMasked, allowed(pos), allowed4(p0), row()) counts only the positions its row mask
//                         allows; the kernels skip the others before they read a distance, so what a disallowed
//                         position's slot holds never matters.  Its dense ties go through k_adc_topk, whose select over
//                         (key, id) words gives ties to the lowest allowed rows
//   adc_key / adc_unkey : the order-preserving key of a distance (NaN sorts last, reported back as 0x7FC00000)
//   adc_scale / adc_bin : the float histogram bin of the ADC and IVF scans
//   adc_bitonic         : the bitonic sort of (key, id) words in LDS;  adc_emit: one result slot from a word
//   TopkState           : hist | sel | cand_n of a batch, carved from a workspace by topk_state
//   launch_topk_select  : k_adc_pick_bin (the bin of the topk-th smallest value) -> k_adc_collect (the positions at or
//                         below it as words) -> k_adc_sort_out (sorted in LDS, the first topk out, padding past a short
//                         query's rows) -> k_adc_topk (exact radix select over (key, id) where the cut held more than
//                         kAdcCand positions; k_adc_topk_rows for the sources built on TopkRows, chosen from the type)
//   adc_terms / adc_row : D(q, i) of one row from ADC tables in LDS, subspace 0 first -- the one operation order of the ADC
//                         scans (k_adc.hip) and the IVF scan (k_ivf.hip)
#pragma once
#include "adc_plan.hpp"
#include "common.hpp"
#include "kernels.hpp"

#include <type_traits>

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

// monotone (non-decreasing in d) bin of a distance over the range [lo, hi] of a query, scale = adc_scale(lo, hi); NaN and
// out-of-range values go to the last bin
__device__ __forceinline__ float adc_scale(float lo, float hi) { return (hi > lo) ? (float)kAdcBins / (hi - lo) : 0.0f; }
__device__ __forceinline__ uint32_t adc_bin(float dval, float lo, float scale) {
    const float t = (dval - lo) * scale;
    return (t >= 0.0f && t < (float)(kAdcBins - 1)) ? (uint32_t)t : ((t < 0.0f) ? 0u : kAdcBins - 1);
}

// the dense part of a source: dist[q][n], the row id is the position (offsets q * n + pos stay 64-bit)
struct TopkRows {
    using Pos = uint64_t;
    static constexpr bool kRagged = false;  // (range.hpp) every position of a query's row counts
    const float *dist;
    uint64_t n;
    // (range.hpp) from the range kernels' arguments: a dense source has no plan and no ids
    static __device__ TopkRows rows(const float *dist, uint64_t n, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t) {
        return {dist, n};
    }
    __device__ void open(uint32_t q) { dist += (size_t)q * n; }
    __device__ Pos count() const { return n; }
    __device__ const float *row() const { return dist; }
    __device__ float at(Pos pos) const { return dist[pos]; }
    __device__ uint32_t id(Pos pos) const { return (uint32_t)pos; }
};

// The dense source under a row mask (include/vqhip.h: row i is allowed iff bit i & 31 of word i >> 5 is set; ceil(n / 32)
// words, 4-byte aligned): only allowed positions count.  allowed4(r0): the bits of positions r0 .. r0 + 3, r0 a multiple
// of 4 below n (bits at or past n are the caller's to drop).
struct MaskedRows : TopkRows {
    static constexpr bool kMasked = true;
    const uint32_t *mask;
    // (range.hpp) the mask travels in the range kernels' `ids` argument: a dense source has no ids of its own
    static __device__ MaskedRows rows(const float *dist, uint64_t n, const uint32_t *, const uint32_t *, const uint32_t *ids, uint32_t) {
        return {{dist, n}, ids};
    }
    __device__ bool allowed(Pos pos) const { return (mask[pos >> 5] >> (uint32_t)(pos & 31u)) & 1u; }
    __device__ uint32_t allowed4(Pos r0) const { return (mask[r0 >> 5] >> (uint32_t)(r0 & 31u)) & 0xFu; }
};

// the distances of positions p0 .. p0 + 3 of a query's row dq[0 .. n), p0 a multiple of 4 below n: one float4 where n % 4 ==
// 0 (then every row of the [q][n] workspace starts 16-byte aligned), else the positions below n whose bit of `ok` is set
__device__ __forceinline__ void masked_load4(const float *__restrict__ dq, uint64_t n, uint64_t p0, uint32_t ok, float (&v)[4]) {
    if ((n & 3u) == 0) {
        const float4 a = *reinterpret_cast<const float4 *>(dq + p0);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) v[j] = (((ok >> j) & 1u) && p0 + j < n) ? dq[p0 + j] : 0.0f;
    }
}

// whether a source has positions that do not count (kMasked); the sources without the member compile to what they were
template <class Src, class = void>
struct topk_masked : std::false_type {};
template <class Src>
struct topk_masked<Src, std::enable_if_t<Src::kMasked>> : std::true_type {};

// per query of a batch of qb: hist [kAdcBins] | sel [2] = {bin of the cut, positions up to it} | cand_n, in this order
// (topk_state_bytes(qb), kernels.hpp; a family's own prefix -- ADC's bounds, k-NN's kmin / kmax -- sits in front)
struct TopkState {
    uint32_t *hist, *sel, *cand_n;
};
inline TopkState topk_state(void *ws, uint32_t qb) {
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws);
    return {hist, hist + (size_t)qb * kAdcBins, hist + (size_t)qb * (kAdcBins + 2)};
}

// ascending bitonic sort of buf[0 .. len) in LDS by a workgroup of NT threads, len a power of two; a barrier in front
// (the buffer's writers) and behind
template <uint32_t NT>
__device__ __forceinline__ void adc_bitonic(unsigned long long *buf, uint32_t len) {
    __syncthreads();
    for (uint32_t size = 2; size <= len; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < len; t += NT) {
                const uint32_t partner = t ^ stride;
                if (partner > t) {
                    const bool up = (t & size) == 0;
                    const unsigned long long a = buf[t], b = buf[partner];
                    if ((a > b) == up) {
                        buf[t] = b;
                        buf[partner] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// one result slot from a word: the row id and the distance behind the key (sqrtf for Euclidean); !real: padding
__device__ __forceinline__ void adc_emit(unsigned long long w, bool real, int take_sqrt, uint32_t *idx, float *dist) {
    if (!real) {
        *idx = 0xFFFFFFFFu;
        *dist = __builtin_inff();
        return;
    }
    float dv = adc_unkey((uint32_t)(w >> 32));
    if (take_sqrt) dv = sqrtf(dv);
    *idx = (uint32_t)w;
    *dist = dv;
}

// step 1: the bin that holds the k-th smallest value; sel[q] = {bin, candidates up to it} ({kAdcBins, all of them} for a
// query with fewer than topk positions)
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

// step 2: every position whose bin is <= the selected one becomes a candidate word; any order (the sort orders them)
template <class Src>
__global__ __launch_bounds__(256) void k_adc_collect(Src src, const uint32_t *__restrict__ sel,
                                                     unsigned long long *__restrict__ cand, uint32_t *__restrict__ cand_n) {
    using Pos = typename Src::Pos;
    const uint32_t q = blockIdx.y;
    if (sel[2 * q + 1] > kAdcCand) return;  // too dense: k_adc_topk
    src.open(q);
    const uint32_t bmax = sel[2 * q];
    const Pos total = src.count();
    if constexpr (topk_masked<Src>::value) {
        // four consecutive positions per lane: one mask read for the four, and no distance read without an allowed one
        for (Pos p0 = ((Pos)blockIdx.x * 256 + threadIdx.x) * 4; p0 < total; p0 += (Pos)gridDim.x * 1024) {
            const uint32_t ok = src.allowed4(p0);
            if (ok == 0) continue;
            float v[4];
            masked_load4(src.row(), total, p0, ok, v);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (((ok >> j) & 1u) && p0 + j < total && src.bin(v[j]) <= bmax) {
                    const uint32_t at = atomicAdd(&cand_n[q], 1u);
                    if (at < kAdcCand) cand[(size_t)q * kAdcCand + at] = ((unsigned long long)adc_key(v[j]) << 32) | src.id(p0 + j);
                }
        }
    } else {
        for (Pos pos = (Pos)blockIdx.x * 256 + threadIdx.x; pos < total; pos += (Pos)gridDim.x * 256) {
            const float dv = src.at(pos);
            if (src.bin(dv) <= bmax) {
                const uint32_t at = atomicAdd(&cand_n[q], 1u);
                if (at < kAdcCand) cand[(size_t)q * kAdcCand + at] = ((unsigned long long)adc_key(dv) << 32) | src.id(pos);
            }
        }
    }
}

// step 3: the candidates sorted in LDS, the first topk out; slots at or past the candidate count (a query with fewer
// than topk positions) are padding
__attribute__((unused)) __global__ __launch_bounds__(1024) void k_adc_sort_out(const unsigned long long *__restrict__ cand,
                                                       const uint32_t *__restrict__ sel, uint32_t topk, int take_sqrt,
                                                       uint32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sort_buf[];  // [kAdcCand]
    const uint32_t q = blockIdx.x, cnt = sel[2 * q + 1];
    if (cnt > kAdcCand) return;  // k_adc_topk
    uint32_t len = 1024;
    while (len < cnt) len <<= 1;
    for (uint32_t e = threadIdx.x; e < len; e += 1024) sort_buf[e] = (e < cnt) ? cand[(size_t)q * kAdcCand + e] : ~0ull;
    adc_bitonic<1024>(sort_buf, len);
    if (threadIdx.x < topk)
        adc_emit(sort_buf[threadIdx.x], threadIdx.x < cnt, take_sqrt, idx_out + (size_t)q * topk + threadIdx.x,
                 dist_out + (size_t)q * topk + threadIdx.x);
}

// step 4, a query whose cut held more than kAdcCand positions (ties piled on one value): exact radix select of the
// topk-th smallest word -- the key's four bytes over all positions, then the row id's four over the positions of that
// key -- and the topk words at or below it, sorted.  More than kAdcCand >= topk positions here: no padding.
template <class Src>
__global__ __launch_bounds__(1024) void k_adc_topk(Src src, uint32_t topk, int take_sqrt, const uint32_t *__restrict__ sel,
                                                   uint32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
    using Pos = typename Src::Pos;
    const uint32_t q = blockIdx.x;
    if (sel[2 * q + 1] <= kAdcCand) return;  // the candidate sort produced this query's result
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_rank, s_count;
    __shared__ unsigned long long win[1024];
    src.open(q);
    const Pos total = src.count();
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_prefix = 0;
        s_rank = topk - 1;
    }
    __syncthreads();
    // pass 0 finds the key T of the topk-th word and its rank among the words of key T; pass 1 the row id R of that rank
    uint32_t T = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const uint32_t prefix = s_prefix, himask = (shift == 24) ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (Pos pos = tid; pos < total; pos += 1024) {
                if constexpr (topk_masked<Src>::value)
                    if (!src.allowed(pos)) continue;
                const uint32_t key = adc_key(src.at(pos));
                uint32_t v = key;
                if (pass == 1) {
                    if (key != T) continue;
                    v = src.id(pos);
                }
                if ((v & himask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
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
        if (pass == 0) {
            T = s_prefix;
            __syncthreads();
            if (tid == 0) s_prefix = 0;  // (s_rank: the rank among the words of key T, carried into pass 1)
            __syncthreads();
        }
    }
    const unsigned long long cut = ((unsigned long long)T << 32) | s_prefix;  // the topk-th smallest word
    if (tid == 0) s_count = 0;
    win[tid] = ~0ull;
    __syncthreads();
    for (Pos pos = tid; pos < total; pos += 1024) {
        if constexpr (topk_masked<Src>::value)
            if (!src.allowed(pos)) continue;
        const uint32_t key = adc_key(src.at(pos));
        if (key > T) continue;
        const unsigned long long w = ((unsigned long long)key << 32) | src.id(pos);
        if (w <= cut) {
            const uint32_t at = atomicAdd(&s_count, 1u);
            if (at < 1024) win[at] = w;  // (exactly topk words pass)
        }
    }
    adc_bitonic<1024>(win, 1024);
    if (tid < topk) adc_emit(win[tid], true, take_sqrt, idx_out + (size_t)q * topk + tid, dist_out + (size_t)q * topk + tid);
}

// step 4 for dense rows (TopkRows: the row id is the position): the key's four bytes as above, then an ORDERED collection
// in chunks of 1024 rows (block prefix sums keep row order) that ends at the topk-th word -- ties go to the lowest rows
// without the four passes over the row id.  Kept beside k_adc_topk because it is faster there: 3.2 against 5.3 ms (ADC)
// and 2.7 against 4.6 ms (k-NN) for 64 queries over 1M rows with 62500 ties at the cut (profiles/topk/ab.json).
__attribute__((unused)) __global__ __launch_bounds__(1024) void k_adc_topk_rows(TopkRows src, uint32_t topk, int take_sqrt,
                                                        const uint32_t *__restrict__ sel, uint32_t *__restrict__ idx_out,
                                                        float *__restrict__ dist_out) {
    if (sel[2 * blockIdx.x + 1] <= kAdcCand) return;  // the candidate sort produced this query's result
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_rank, s_count;
    __shared__ uint32_t wsum[16];
    __shared__ unsigned long long win[1024];
    src.open(blockIdx.x);
    const float *dq = src.dist;
    const uint64_t n = src.n;
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
    if (tid >= topk) win[tid] = ~0ull;  // (exactly topk words were taken)
    adc_bitonic<1024>(win, 1024);
    if (tid < topk)
        adc_emit(win[tid], true, take_sqrt, idx_out + (size_t)blockIdx.x * topk + tid, dist_out + (size_t)blockIdx.x * topk + tid);
}

// the dynamic LDS of k_adc_sort_out (this file's copy), once per device
inline int topk_sort_attr() {
    static PerDeviceOnce attr;
    if (attr.needed()) {
        VQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_adc_sort_out), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(kAdcCand * 8)));
        attr.done();
    }
    return VQHIP_OK;
}

// The selection of one batch of nb queries whose scan has filled st.hist (st zeroed before the scan): results
// [nb][topk] on the device.  cand >= topk_cand_bytes(nb).
template <class Src>
int launch_topk_select(const Src &src, uint32_t nb, uint32_t topk, int take_sqrt, const TopkState &st, unsigned long long *cand,
                       uint32_t *idx_out, float *dist_out, hipStream_t stream) {
    VQ_TRY(topk_sort_attr());
    hipLaunchKernelGGL(k_adc_pick_bin, dim3(nb), dim3(64), 0, stream, st.hist, topk, st.sel);
    VQ_LAUNCH_CHECK("k_adc_pick_bin");
    hipLaunchKernelGGL(k_adc_collect<Src>, dim3(src.blocks(), nb), dim3(256), 0, stream, src, st.sel, cand, st.cand_n);
    VQ_LAUNCH_CHECK("k_adc_collect");
    hipLaunchKernelGGL(k_adc_sort_out, dim3(nb), dim3(1024), (size_t)kAdcCand * 8, stream, cand, st.sel, topk, take_sqrt, idx_out,
                       dist_out);
    VQ_LAUNCH_CHECK("k_adc_sort_out");
    if constexpr (std::is_base_of<TopkRows, Src>::value && !topk_masked<Src>::value)
        hipLaunchKernelGGL(k_adc_topk_rows, dim3(nb), dim3(1024), 0, stream, src, topk, take_sqrt, st.sel, idx_out, dist_out);
    else
        hipLaunchKernelGGL(k_adc_topk<Src>, dim3(nb), dim3(1024), 0, stream, src, topk, take_sqrt, st.sel, idx_out, dist_out);
    VQ_LAUNCH_CHECK("k_adc_topk");
    return VQHIP_OK;
}

}  // namespace
}  // namespace vqhip
