// k_binary.hip -- the binary index: BQ bits packed 32 to a word, exact Hamming top-k over them.
// No reference counterpart (the crate has no search function); the semantics are the ones include/vqhip.h states:
//   bits    = x >= threshold for f32 (NaN -> 0, -0.0 == 0.0), c >= high for u8 codes (the BQ encode / decode rules)
//   layout  = row i, dimension t in word i * W + t / 32, bit t % 32, W = ceil(d / 32), pad bits zero
//   D(q, i) = S[H] (sqrtf(S[H]) for Euclidean), H = popcount(bits(q) xor bits(row_i)), S the host's sequential f32 table;
//             S is strictly increasing, so (H, row) orders like (D, row) and the scans select on the integer H.
// Schedule of one search (launch_binary_search), per batch of <= 1024 packed queries:
//   k_bin_scan<HIST>     workgroup = (a slice of <= 65535 rows) x (a group of QG queries, their words in LDS); every lane
//                        takes two rows at a time, XORs their words against each query's and counts bits; per query an
//                        LDS histogram of H in 16-bit halves (a slice cannot carry a half past 65535), added to the
//                        batch's global [q][d + 1] histogram at the end, non-zero bins only
//   k_bin_pick           per query the cut H* (the smallest H whose cumulative count reaches topk), the rows below it and
//                        the rows at it
//   k_bin_scan<COLLECT>  the same scan again: rows with H < H*, and those with H == H* unless the cut is heavy, into the
//                        query's candidate list (key adc_key(S[H]), row)
//   k_bin_ties           heavy cut (more than 8192 candidates): the lowest need = topk - less row ids with H == H*, found
//                        by an ordered scan over the rows that stops once it has them
//   k_adc_sort_out       (topk.hpp) the candidates sorted by (key, row) in LDS, the first topk out,
//                        sqrtf for Euclidean
// A filtered call (a row mask) runs the masked twins of the scans, the pick and the ties: the 64 rows a
// wave takes at one (step, j) are two mask words (bin_mask64), a wave without an allowed row among them skips the step, and
// the histogram, the cut and the candidates hold allowed rows only.  mask == NULL launches the kernels above as they are.
// Roofline: VALU, 2 operations (v_xor, v_bcnt with accumulate) per 32 dimensions per (query, row) pair and scan.
#include "kernels.hpp"
#include "range.hpp"
#include "topk.hpp"

#include <algorithm>
#include <vector>

namespace vqhip {
namespace {

constexpr uint32_t kPackBlock = 256;
constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanRR = 2;                 // rows per lane and step of the scan
constexpr uint64_t kSliceMax = 65535;           // rows per scan workgroup: a 16-bit histogram half never carries
constexpr uint32_t kTiesBlock = 1024;

enum { BIN_HIST = 0, BIN_COLLECT = 1 };

__device__ __forceinline__ bool bq_bit(float v, float thr, uint32_t) { return v >= thr; }
__device__ __forceinline__ bool bq_bit(uint8_t v, float, uint32_t high) { return (uint32_t)v >= high; }

// bit i of the byte b -> bit 4 i
__device__ __forceinline__ uint32_t spread4(uint32_t b) {
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    b = (b | (b << 3)) & 0x11111111u;
    return b;
}

// One wave per row (grid-stride over rows).  VEC (d % 4 == 0, x 4-element aligned): windows of 256 elements, four per
// lane in one load, four ballots; lane j < 8 assembles word j of the window from byte j of each.  Otherwise windows of 64
// elements, one per lane, one ballot, two words.  Elements past d contribute 0: the pad bits.
template <typename T, bool VEC>
__global__ __launch_bounds__(kPackBlock) void k_bq_pack(const T *__restrict__ x, uint64_t n, uint32_t d, uint32_t W, float thr,
                                                       uint32_t high, uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kPackBlock / 64);
    for (uint64_t r = (uint64_t)blockIdx.x * (kPackBlock / 64) + (threadIdx.x >> 6); r < n; r += waves) {
        const T *xr = x + r * d;
        uint32_t *o = out + r * W;
        if constexpr (VEC) {
            for (uint32_t t0 = 0; t0 < d; t0 += 256) {
                const uint32_t t = t0 + 4 * lane;
                bool b0 = false, b1 = false, b2 = false, b3 = false;
                if (t < d) {
                    if constexpr (sizeof(T) == 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(xr + t);
                        b0 = bq_bit(v.x, thr, high), b1 = bq_bit(v.y, thr, high);
                        b2 = bq_bit(v.z, thr, high), b3 = bq_bit(v.w, thr, high);
                    } else {
                        const uint32_t v = *reinterpret_cast<const uint32_t *>(xr + t);
                        b0 = (v & 0xffu) >= high, b1 = ((v >> 8) & 0xffu) >= high;
                        b2 = ((v >> 16) & 0xffu) >= high, b3 = (v >> 24) >= high;
                    }
                }
                const uint64_t m0 = __ballot(b0), m1 = __ballot(b1), m2 = __ballot(b2), m3 = __ballot(b3);
                const uint32_t c = t0 / 32 + lane;
                if (lane < 8 && c < W) {
                    const uint32_t s = 8 * lane;
                    o[c] = spread4((uint32_t)(m0 >> s) & 0xffu) | (spread4((uint32_t)(m1 >> s) & 0xffu) << 1) |
                           (spread4((uint32_t)(m2 >> s) & 0xffu) << 2) | (spread4((uint32_t)(m3 >> s) & 0xffu) << 3);
                }
            }
        } else {
            for (uint32_t t0 = 0; t0 < d; t0 += 64) {
                const uint32_t t = t0 + lane;
                const uint64_t m = __ballot(t < d && bq_bit(xr[t], thr, high));
                const uint32_t c = t0 / 32;
                if (lane == 0) o[c] = (uint32_t)m;
                if (lane == 1 && c + 1 < W) o[c + 1] = (uint32_t)(m >> 32);
            }
        }
    }
}

// nonzero where a pad bit (dimension >= d) of a packed row is set
__global__ __launch_bounds__(256) void k_bin_padcheck(const uint32_t *__restrict__ P, uint64_t n, uint32_t W, uint32_t mask,
                                                      uint32_t *__restrict__ bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (P[i * W + (W - 1)] & ~mask) atomicOr(bad, 1u);
}

// H of QG queries for the lane's rows r[0..RR): words of the rows from global memory, of the queries from LDS
template <uint32_t QG, bool V4>
__device__ __forceinline__ void bin_hamming(const uint32_t *__restrict__ P, const uint64_t (&r)[kScanRR], const bool (&ok)[kScanRR],
                                            uint32_t W, const uint32_t *qs, uint32_t (&h)[kScanRR][QG]) {
#pragma unroll
    for (uint32_t j = 0; j < kScanRR; ++j)
#pragma unroll
        for (uint32_t q = 0; q < QG; ++q) h[j][q] = 0;
    if constexpr (V4) {
        for (uint32_t c = 0; c < W; c += 4) {
            uint4 w[kScanRR];
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j)
                w[j] = ok[j] ? *reinterpret_cast<const uint4 *>(P + r[j] * W + c) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (uint32_t q = 0; q < QG; ++q) {
                const uint4 v = *reinterpret_cast<const uint4 *>(qs + q * W + c);
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) {
                    uint32_t a = h[j][q];
                    a = __builtin_popcount(w[j].x ^ v.x) + a;
                    a = __builtin_popcount(w[j].y ^ v.y) + a;
                    a = __builtin_popcount(w[j].z ^ v.z) + a;
                    a = __builtin_popcount(w[j].w ^ v.w) + a;
                    h[j][q] = a;
                }
            }
        }
    } else {
        for (uint32_t c = 0; c < W; ++c) {
            uint32_t w[kScanRR];
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) w[j] = ok[j] ? P[r[j] * W + c] : 0u;
#pragma unroll
            for (uint32_t q = 0; q < QG; ++q) {
                const uint32_t v = qs[q * W + c];
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) h[j][q] = __builtin_popcount(w[j] ^ v) + h[j][q];
            }
        }
    }
}

// The row mask of a filtered call over the 64 rows [g, g + 64) that one wave takes at one (step, j):
// g is a multiple of 64 and wave-uniform, so the rows are the two mask words g / 32 and g / 32 + 1, read as two u32 (the
// mask is only 4-byte aligned) through uniform addresses -- the second only where it exists (nwords = ceil(n / 32)).  Bit
// b of the result: row g + b is allowed and below hi (hi <= n, so the bits at or past n are cleared with them).
__device__ __forceinline__ uint64_t bin_mask64(const uint32_t *__restrict__ mask, uint32_t nwords, uint64_t g, uint64_t hi) {
    if (g >= hi) return 0;
    const uint32_t k = (uint32_t)(g >> 5);
    uint64_t m = mask[k];
    if (k + 1 < nwords) m |= (uint64_t)mask[k + 1] << 32;
    const uint64_t left = hi - g;
    if (left < 64) m &= (1ull << left) - 1ull;
    return m;
}

// the wave of a lane as a uniform value
__device__ __forceinline__ uint32_t bin_wave() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Q [nb][W] packed queries of the batch; workgroup (x, y) scans rows [x * slice, (x + 1) * slice) for queries
// [y * QG, y * QG + QG) of them.  HIST: adds each query's histogram of H to hist [nb][d + 1].  COLLECT: appends the rows
// that sel admits to cand [nb][kAdcCand] through the counters cnt [nb].
// MASKED: slice is a multiple of 64, so the 64 rows of a wave at (step, j) are two words of mask; a row counts only where
// its bit is set, and a wave without an allowed row at either j leaves the step before it loads a row or a query word.
template <uint32_t QG, bool V4, int MODE, bool MASKED>
__device__ __forceinline__ void bin_scan_body(const uint32_t *__restrict__ P, uint64_t n, uint32_t W, uint32_t d,
                                              const uint32_t *__restrict__ Q, uint32_t nb, uint64_t slice,
                                              uint32_t *__restrict__ hist, const BinSel *__restrict__ sel,
                                              const float *__restrict__ S, unsigned long long *__restrict__ cand,
                                              uint32_t *__restrict__ cnt, const uint32_t *__restrict__ mask) {
    extern __shared__ uint32_t lds[];
    uint32_t *qs = lds;                 // [QG][W]
    uint32_t *hs = lds + QG * W;        // HIST: [QG][(d + 2) / 2] bin pairs; COLLECT: [QG][2] (cut, take ties)
    const uint32_t q0 = blockIdx.y * QG;
    const uint32_t qn = min(QG, nb - q0);
    const uint32_t H2 = (d + 2) / 2;
    for (uint32_t e = threadIdx.x; e < QG * W; e += kScanBlock) qs[e] = e / W < qn ? Q[(size_t)(q0 + e / W) * W + e % W] : 0u;
    if constexpr (MODE == BIN_HIST) {
        for (uint32_t e = threadIdx.x; e < QG * H2; e += kScanBlock) hs[e] = 0;
    } else {
        for (uint32_t q = threadIdx.x; q < QG; q += kScanBlock) {
            hs[2 * q] = q < qn ? sel[q0 + q].hstar : 0u;
            hs[2 * q + 1] = q < qn ? (sel[q0 + q].heavy ? 0u : 1u) : 0u;
        }
    }
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * slice, hi = min(n, lo + slice);
    // (MASKED: base is the step's first row, uniform; otherwise the lane's)
    for (uint64_t base = MASKED ? lo : lo + threadIdx.x; base < hi; base += kScanBlock * kScanRR) {
        uint64_t r[kScanRR];
        bool ok[kScanRR];
        if constexpr (MASKED) {
            const uint32_t nwords = (uint32_t)((n + 31) >> 5), wv = bin_wave(), lane = threadIdx.x & 63u;
            uint64_t m[kScanRR];
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) m[j] = bin_mask64(mask, nwords, base + (uint64_t)j * kScanBlock + wv * 64u, hi);
            if (!(m[0] | m[1])) continue;  // (uniform) no allowed row in the wave's 128
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) {
                r[j] = base + (uint64_t)j * kScanBlock + threadIdx.x;
                ok[j] = (m[j] >> lane) & 1ull;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) {
                r[j] = base + (uint64_t)j * kScanBlock;
                ok[j] = r[j] < hi;
            }
        }
        uint32_t h[kScanRR][QG];
        bin_hamming<QG, V4>(P, r, ok, W, qs, h);
#pragma unroll
        for (uint32_t q = 0; q < QG; ++q) {
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) {
                if (!ok[j] || q >= qn) continue;
                const uint32_t v = h[j][q];
                if constexpr (MODE == BIN_HIST) {
                    atomicAdd(&hs[q * H2 + (v >> 1)], 1u << ((v & 1u) << 4));
                } else {
                    const uint32_t cut = hs[2 * q];
                    if (v < cut || (v == cut && hs[2 * q + 1])) {
                        const uint32_t pos = atomicAdd(&cnt[q0 + q], 1u);
                        if (pos < kAdcCand)
                            cand[(size_t)(q0 + q) * kAdcCand + pos] =
                                ((unsigned long long)adc_key(S[v]) << 32) | (uint32_t)r[j];
                    }
                }
            }
        }
    }
    if constexpr (MODE == BIN_HIST) {
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < qn * H2; e += kScanBlock) {
            const uint32_t v = hs[e];
            if (!v) continue;
            const uint32_t q = e / H2, b = 2 * (e % H2);
            uint32_t *g = hist + (size_t)(q0 + q) * (d + 1);
            if (v & 0xffffu) atomicAdd(&g[b], v & 0xffffu);
            if ((v >> 16) && b + 1 <= d) atomicAdd(&g[b + 1], v >> 16);
        }
    }
}

template <uint32_t QG, bool V4, int MODE>
__global__ __launch_bounds__(kScanBlock) void k_bin_scan(const uint32_t *__restrict__ P, uint64_t n, uint32_t W, uint32_t d,
                                                        const uint32_t *__restrict__ Q, uint32_t nb, uint64_t slice,
                                                        uint32_t *__restrict__ hist, const BinSel *__restrict__ sel,
                                                        const float *__restrict__ S, unsigned long long *__restrict__ cand,
                                                        uint32_t *__restrict__ cnt) {
    bin_scan_body<QG, V4, MODE, false>(P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, nullptr);
}

// (the second launch bound: the one instantiation whose mask registers would cost it a wave against its unmasked twin,
// 81 VGPRs against 80, is held to the twin's six waves a SIMD; every other one is left to the compiler)
template <uint32_t QG, bool V4, int MODE>
__global__ __launch_bounds__(kScanBlock, (QG == 32 && !V4 && MODE == BIN_HIST) ? 6 : 1) void k_bin_scan_masked(
                                                               const uint32_t *__restrict__ P, uint64_t n, uint32_t W, uint32_t d,
                                                               const uint32_t *__restrict__ Q, uint32_t nb, uint64_t slice,
                                                               uint32_t *__restrict__ hist, const BinSel *__restrict__ sel,
                                                               const float *__restrict__ S, unsigned long long *__restrict__ cand,
                                                               uint32_t *__restrict__ cnt, const uint32_t *__restrict__ mask) {
    bin_scan_body<QG, V4, MODE, true>(P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, mask);
}

// per query: the cut H* = the smallest H with count(H' <= H) >= topk; rows below it, rows at it; adc_sel [2 q + 1] = the
// candidates k_adc_sort_out will find (heavy: topk)
// UNDER (a filtered call: the histogram counts allowed rows only, and there may be fewer than topk of them): a query
// whose total is below topk takes every allowed row -- cut d with its ties, not heavy, adc_sel [2 q + 1] = the total, which
// k_adc_sort_out pads to topk.  Without it topk <= n keeps the walk inside the bins.
template <bool UNDER>
__device__ __forceinline__ void bin_pick_body(const uint32_t *__restrict__ hist, uint32_t d, uint32_t topk,
                                              BinSel *__restrict__ sel, uint32_t *__restrict__ adc_sel,
                                              uint32_t *__restrict__ cnt) {
    __shared__ unsigned long long seg_sum[256];
    __shared__ unsigned long long s_before;
    __shared__ uint32_t s_seg;
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    const uint32_t bins = d + 1, per = (bins + 255) / 256;
    const uint32_t *hq = hist + (size_t)q * bins;
    const uint32_t b0 = min(bins, t * per), b1 = min(bins, b0 + per);
    unsigned long long s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += hq[b];
    seg_sum[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long cum = 0;
        uint32_t j = 0;
        for (; j < 255; ++j) {
            if (cum + seg_sum[j] >= topk) break;
            cum += seg_sum[j];
        }
        s_before = cum;
        s_seg = j;
        if constexpr (UNDER) {
            if (j == 255 && cum + seg_sum[255] < topk) {  // (total < topk <= 1024)
                const uint32_t total = (uint32_t)(cum + seg_sum[255]);
                sel[q] = BinSel{d, total, 0u, 0u};
                adc_sel[2 * q] = d;
                adc_sel[2 * q + 1] = total;
                cnt[q] = 0;
                s_seg = 256;  // no thread walks a segment
            }
        }
    }
    __syncthreads();
    if (t == s_seg) {
        unsigned long long cum = s_before;
        uint32_t b = b0;
        for (; b + 1 < b1; ++b) {
            if (cum + hq[b] >= topk) break;
            cum += hq[b];
        }
        const unsigned long long eq = hq[b];
        const bool heavy = cum + eq > kAdcCand;
        sel[q] = BinSel{b, (uint32_t)cum, topk - (uint32_t)cum, heavy ? 1u : 0u};
        adc_sel[2 * q] = b;
        adc_sel[2 * q + 1] = heavy ? topk : (uint32_t)(cum + eq);
        cnt[q] = 0;
    }
}

__global__ __launch_bounds__(256) void k_bin_pick(const uint32_t *__restrict__ hist, uint32_t d, uint32_t topk,
                                                  BinSel *__restrict__ sel, uint32_t *__restrict__ adc_sel,
                                                  uint32_t *__restrict__ cnt) {
    bin_pick_body<false>(hist, d, topk, sel, adc_sel, cnt);
}

__global__ __launch_bounds__(256) void k_bin_pick_masked(const uint32_t *__restrict__ hist, uint32_t d, uint32_t topk,
                                                         BinSel *__restrict__ sel, uint32_t *__restrict__ adc_sel,
                                                         uint32_t *__restrict__ cnt) {
    bin_pick_body<true>(hist, d, topk, sel, adc_sel, cnt);
}

// heavy cut: the lowest sel.need row ids with H == H*, by an ordered scan in chunks of 1024 rows, to cand [q][less ..)
// MASKED: the lowest allowed ones -- H is computed for allowed rows only (a chunk starts on a multiple of 1024, a wave's
// rows are two words of mask)
template <bool MASKED>
__device__ __forceinline__ void bin_ties_body(const uint32_t *__restrict__ P, uint64_t n, uint32_t W,
                                              const uint32_t *__restrict__ Q, const BinSel *__restrict__ sel,
                                              const float *__restrict__ S, unsigned long long *__restrict__ cand,
                                              const uint32_t *__restrict__ mask) {
    const uint32_t q = blockIdx.x;
    const BinSel s = sel[q];
    if (!s.heavy) return;
    extern __shared__ uint32_t qw[];  // [W]
    __shared__ uint32_t wsum[kTiesBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (uint32_t c = tid; c < W; c += kTiesBlock) qw[c] = Q[(size_t)q * W + c];
    __syncthreads();
    const unsigned long long key = (unsigned long long)adc_key(S[s.hstar]) << 32;
    unsigned long long *out = cand + (size_t)q * kAdcCand + s.less;
    uint32_t taken = 0;  // uniform
    for (uint64_t base = 0; base < n && taken < s.need; base += kTiesBlock) {
        const uint64_t i = base + tid;
        bool eq = false, in = i < n;
        if constexpr (MASKED)
            in = (bin_mask64(mask, (uint32_t)((n + 31) >> 5), base + (uint64_t)bin_wave() * 64u, n) >> lane) & 1ull;
        if (in) {
            uint32_t h = 0;
            for (uint32_t c = 0; c < W; ++c) h = __builtin_popcount(P[i * W + c] ^ qw[c]) + h;
            eq = h == s.hstar;
        }
        const uint64_t m = __ballot(eq);
        if (lane == 0) wsum[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (uint32_t w = 0; w < kTiesBlock / 64; ++w) {
            if (w < wv) before += wsum[w];
            total += wsum[w];
        }
        if (eq && taken + before < s.need) out[taken + before] = key | (uint32_t)i;
        taken += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kTiesBlock) void k_bin_ties(const uint32_t *__restrict__ P, uint64_t n, uint32_t W,
                                                         const uint32_t *__restrict__ Q, const BinSel *__restrict__ sel,
                                                         const float *__restrict__ S, unsigned long long *__restrict__ cand) {
    bin_ties_body<false>(P, n, W, Q, sel, S, cand, nullptr);
}

__global__ __launch_bounds__(kTiesBlock) void k_bin_ties_masked(const uint32_t *__restrict__ P, uint64_t n, uint32_t W,
                                                                const uint32_t *__restrict__ Q, const BinSel *__restrict__ sel,
                                                                const float *__restrict__ S, unsigned long long *__restrict__ cand,
                                                                const uint32_t *__restrict__ mask) {
    bin_ties_body<true>(P, n, W, Q, sel, S, cand, mask);
}

// QG queries per scan workgroup: their H histograms in 16-bit halves must fit in LDS with room for two workgroups a CU
// where d allows it
uint32_t bin_qg(uint32_t d) { return d <= 1024 ? 32u : 8u; }

size_t bin_scan_lds(uint32_t qg, uint32_t W, uint32_t d, int mode) {
    return (size_t)qg * W * 4 + (mode == BIN_HIST ? (size_t)qg * ((d + 2) / 2) * 4 : (size_t)qg * 2 * 4);
}

template <uint32_t QG, bool V4, int MODE>
int bin_scan_launch(dim3 grid, size_t lds, const uint32_t *P, uint64_t n, uint32_t W, uint32_t d, const uint32_t *Q, uint32_t nb,
                    uint64_t slice, uint32_t *hist, const BinSel *sel, const float *S, unsigned long long *cand, uint32_t *cnt,
                    const uint32_t *mask, hipStream_t stream) {
    if (mask) {
        static PerDeviceOnce attr_m;
        if (attr_m.needed()) {
            VQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bin_scan_masked<QG, V4, MODE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            attr_m.done();
        }
        hipLaunchKernelGGL((k_bin_scan_masked<QG, V4, MODE>), grid, dim3(kScanBlock), lds, stream, P, n, W, d, Q, nb, slice, hist,
                           sel, S, cand, cnt, mask);
        VQ_LAUNCH_CHECK("k_bin_scan_masked");
        return VQHIP_OK;
    }
    static PerDeviceOnce attr;
    if (attr.needed()) {
        VQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bin_scan<QG, V4, MODE>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.done();
    }
    hipLaunchKernelGGL((k_bin_scan<QG, V4, MODE>), grid, dim3(kScanBlock), lds, stream, P, n, W, d, Q, nb, slice, hist, sel, S,
                       cand, cnt);
    VQ_LAUNCH_CHECK("k_bin_scan");
    return VQHIP_OK;
}

template <int MODE>
int bin_scan(const uint32_t *P, uint64_t n, uint32_t W, uint32_t d, const uint32_t *Q, uint32_t nb, uint32_t *hist,
             const BinSel *sel, const float *S, unsigned long long *cand, uint32_t *cnt, const uint32_t *mask,
             hipStream_t stream) {
    const uint32_t qg = bin_qg(d), groups = (nb + qg - 1) / qg;
    // slices: at most 65535 rows each, and about 2048 workgroups in all where n allows 512 rows a workgroup
    uint64_t slices = std::max<uint64_t>((n + kSliceMax - 1) / kSliceMax,
                                         std::min<uint64_t>((2048 + groups - 1) / groups, (n + 511) / 512));
    uint64_t slice = (n + slices - 1) / slices;
    if (mask) slice = binary_masked_slice(n, groups);
    slices = (n + slice - 1) / slice;
    const dim3 grid((uint32_t)slices, groups);
    const size_t lds = bin_scan_lds(qg, W, d, MODE);
    const bool v4 = W % 4 == 0;
    if (qg == 32)
        return v4 ? bin_scan_launch<32, true, MODE>(grid, lds, P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, mask, stream)
                  : bin_scan_launch<32, false, MODE>(grid, lds, P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, mask, stream);
    return v4 ? bin_scan_launch<8, true, MODE>(grid, lds, P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, mask, stream)
              : bin_scan_launch<8, false, MODE>(grid, lds, P, n, W, d, Q, nb, slice, hist, sel, S, cand, cnt, mask, stream);
}

template <typename T, bool VEC>
int pack_launch(const T *x, uint64_t n, uint32_t d, float thr, uint32_t high, uint32_t *out, hipStream_t stream) {
    const uint64_t blocks = std::min<uint64_t>((n + kPackBlock / 64 - 1) / (kPackBlock / 64), 8192);
    hipLaunchKernelGGL((k_bq_pack<T, VEC>), dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(kPackBlock), 0, stream, x, n, d,
                       bin_words(d), thr, high, out);
    VQ_LAUNCH_CHECK("k_bq_pack");
    return VQHIP_OK;
}

}  // namespace

uint32_t bin_words(uint32_t d) { return (d + 31) / 32; }

// Rows per scan workgroup of a filtered call: bin_scan's slicing with every slice a multiple of 64, so that a wave's 64
// rows are two whole mask words, and at most 65472 = 65535 rounded down to one (rounding 65535 up would let a 16-bit
// histogram half carry).  groups: the query groups of the batch.
uint64_t binary_masked_slice(uint64_t n, uint32_t groups) {
    constexpr uint64_t kMax = kSliceMax / 64 * 64;
    groups = std::max(groups, 1u);
    const uint64_t slices = std::max<uint64_t>((n + kMax - 1) / kMax, std::min<uint64_t>((2048 + groups - 1) / groups, (n + 511) / 512));
    return ((n + slices - 1) / slices + 63) / 64 * 64;
}

int binary_table(uint32_t d, uint32_t low, uint32_t high, int metric, float *S) {
    const float a = (float)high - (float)low;
    const float t = metric == VQHIP_MANHATTAN ? a : a * a;
    float s = 0.0f;  // -0.0 + +0.0 (d >= 1 agreeing dimensions or not) = +0.0
    S[0] = s;
    for (uint32_t j = 1; j <= d; ++j) {
        s = s + t;
        S[j] = s;
    }
    return VQHIP_OK;
}

int launch_bq_pack(const void *x, int kind, uint64_t n, uint32_t d, float thr, uint32_t high, uint32_t *out, hipStream_t stream) {
    if (n == 0) return VQHIP_OK;
    if (kind == VQHIP_BINARY_U8) {
        const uint8_t *c = static_cast<const uint8_t *>(x);
        if (d % 4 == 0 && (reinterpret_cast<uintptr_t>(c) & 3) == 0) return pack_launch<uint8_t, true>(c, n, d, thr, high, out, stream);
        return pack_launch<uint8_t, false>(c, n, d, thr, high, out, stream);
    }
    const float *f = static_cast<const float *>(x);
    if (d % 4 == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0) return pack_launch<float, true>(f, n, d, thr, high, out, stream);
    return pack_launch<float, false>(f, n, d, thr, high, out, stream);
}

int launch_bin_padcheck(const uint32_t *P, uint64_t n, uint32_t d, uint32_t *bad, hipStream_t stream) {
    if (d % 32 == 0 || n == 0) return VQHIP_OK;
    const uint32_t W = bin_words(d), mask = (1u << (d % 32)) - 1u;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_bin_padcheck, dim3((uint32_t)blocks), dim3(256), 0, stream, P, n, W, mask, bad);
    VQ_LAUNCH_CHECK("k_bin_padcheck");
    return VQHIP_OK;
}

size_t binary_hist_bytes(uint32_t qb, uint32_t d) { return (size_t)qb * (d + 1) * 4; }

int launch_binary_search(const uint32_t *P, uint64_t n, uint32_t d, int metric, const float *S, const uint32_t *Q, uint32_t nb,
                         uint32_t topk, uint32_t *hist, BinSel *sel, uint32_t *adc_sel, uint32_t *cnt,
                         unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream, const uint32_t *mask) {
    if (topk == 0 || topk > 1024 || topk > n) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, min(n, 1024)]");
    if (nb == 0) return VQHIP_OK;
    VQ_TRY(topk_sort_attr());
    const uint32_t W = bin_words(d);
    VQ_HIP(hipMemsetAsync(hist, 0, binary_hist_bytes(nb, d), stream));
    VQ_TRY(bin_scan<BIN_HIST>(P, n, W, d, Q, nb, hist, sel, S, cand, cnt, mask, stream));
    if (mask) hipLaunchKernelGGL(k_bin_pick_masked, dim3(nb), dim3(256), 0, stream, hist, d, topk, sel, adc_sel, cnt);
    else hipLaunchKernelGGL(k_bin_pick, dim3(nb), dim3(256), 0, stream, hist, d, topk, sel, adc_sel, cnt);
    VQ_LAUNCH_CHECK("k_bin_pick");
    VQ_TRY(bin_scan<BIN_COLLECT>(P, n, W, d, Q, nb, hist, sel, S, cand, cnt, mask, stream));
    if (mask) hipLaunchKernelGGL(k_bin_ties_masked, dim3(nb), dim3(kTiesBlock), (size_t)W * 4, stream, P, n, W, Q, sel, S, cand, mask);
    else hipLaunchKernelGGL(k_bin_ties, dim3(nb), dim3(kTiesBlock), (size_t)W * 4, stream, P, n, W, Q, sel, S, cand);
    VQ_LAUNCH_CHECK("k_bin_ties");
    hipLaunchKernelGGL(k_adc_sort_out, dim3(nb), dim3(1024), (size_t)kAdcCand * 8, stream, cand, adc_sel, topk,
                       metric == VQHIP_EUCLIDEAN ? 1 : 0, idx_out, dist_out);
    VQ_LAUNCH_CHECK("k_adc_sort_out");
    return VQHIP_OK;
}

// ------------------------------------------------------------------ Hamming-radius range search ----
// Row i is a hit of query q iff H(q, i) <= hcut[q] (the caller's radius, clamped to d); the result is range.hpp's CSR,
// the hits of a query in ascending row id, dist = S[H] (its root under Euclidean).  No H is materialised: the rows are
// scanned twice, as a search scans them, and range.hpp's protocol runs between the scans.  Per batch of nb queries:
//   launch_bq_pack        the batch's queries as words Q [nb][W]
//   k_bin_range<COUNT>    workgroup = (block of kBinRangeRows consecutive rows) x (group of QG queries, their words in
//                         LDS), k_bin_scan's lane-to-row mapping; every lane counts its hits per query in registers, the
//                         counts are summed over the wave (shuffles) and the four waves (LDS) into cnt[q][blk]
//   k_range_scan          (range.hpp) cnt -> off[q][blk] in query-major order, lims, the batch total
//   range_scan_room       (range.hpp) that scan, then the 8-byte read, max_results, room for the hits
//   k_bin_range<FILL>     the count's grid; a workgroup whose QG counts are all zero returns before it reads a row.  The
//                         others recompute H; a hit of query q goes to base + off[q][blk] + its rank in the block.
// Ascending row id within a block is the order (step, j, wave, lane) of the scan: a step is kScanBlock * kScanRR rows, row
// j of a lane is base + j * kScanBlock + tid.  The rank of a hit is therefore
//   the hits of earlier steps (run[q], uniform: the sum of the steps' totals)
//   + for j = 1 the step's hits at j = 0, + the hits of earlier waves at the same (step, j)   (wave totals through LDS)
//   + the hits of lower lanes of its wave at (step, j)                                         (the ballot, masked below the lane)
// No slot depends on the order of an atomic; there are none.  A step's wave totals go through LDS as one word per (query,
// wave), j = 0 in the low half and j = 1 in the high half (at most 64 each, their sums over four waves at most 256), in
// two buffers used in turn: one barrier per step.
namespace {

enum { BIN_COUNT = 0, BIN_FILL = 1 };
static_assert(kScanRR == 2, "k_bin_range<FILL> packs the two rows of a lane into one word");
constexpr uint32_t kBinRangeRows = VQHIP_BINARY_RANGE_BLOCK;      // rows per workgroup: 16 steps
constexpr uint32_t kBinRangeStep = kScanBlock * kScanRR;          // rows per step: 512
static_assert(kBinRangeRows % kBinRangeStep == 0 && kBinRangeRows / kBinRangeStep * kScanRR < 256, "a block is whole steps, a lane's hits a byte");
constexpr uint64_t kBinRangeEntries = 1ull << 17;                 // count entries of a batch of several queries, at most

// MASKED (a filtered call): a block starts on a multiple of 8192, so a wave's 64 rows at (step, j)
// are two words of mask (bin_mask64); a row is a hit only where its bit is set.  A wave without an allowed row at either j
// skips the step's Hamming work: COUNT goes on to the next step, FILL still meets the step's barrier with zero totals.
// The mask is the kernel's optional last argument (MASK: no type, or const uint32_t *), so the unmasked instantiation is
// the kernel of an unfiltered call with its arguments, and nothing of the masked form is in it.
template <uint32_t QG, bool V4, int MODE, class... MASK>
__global__ __launch_bounds__(kScanBlock, 3) void k_bin_range(const uint32_t *__restrict__ P, uint64_t n, uint32_t W,
                                                         const uint32_t *__restrict__ Q, uint32_t nb,
                                                         const uint32_t *__restrict__ hcut, uint32_t nblk,
                                                         uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ off,
                                                         unsigned long long base, const float *__restrict__ S, int root,
                                                         uint32_t *__restrict__ idx_out, float *__restrict__ dist_out,
                                                         MASK... mask_arg) {
    constexpr bool MASKED = sizeof...(MASK) == 1;
    static_assert(sizeof...(MASK) <= 1, "one row mask at most");
    [[maybe_unused]] const uint32_t *mask = nullptr;
    if constexpr (MASKED) mask = (mask_arg, ...);
    extern __shared__ __attribute__((aligned(16))) uint32_t range_lds[];  // qs [QG][W]
    __shared__ __attribute__((aligned(16))) uint32_t wt[2][QG][4];  // FILL: a step's wave totals; COUNT: wt[0][q][wave]
    __shared__ uint32_t s_c[QG];                                     // FILL: the block's count per query
    __shared__ unsigned long long s_at[QG];                          // FILL: the block's first slot per query
    uint32_t *qs = range_lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t q0 = blockIdx.y * QG;
    const uint32_t qn = min(QG, nb - q0);
    const uint64_t lo = (uint64_t)blockIdx.x * kBinRangeRows, hi = min(n, lo + kBinRangeRows);
    uint32_t act = 0;  // FILL: bit q set where query q0 + q has hits in this block (uniform)
    if constexpr (MODE == BIN_FILL) {
        uint32_t mine = 0;
        if (tid < QG) {
            unsigned long long at = 0;
            if (tid < qn) {
                const size_t e = (size_t)(q0 + tid) * nblk + blockIdx.x;
                mine = cnt[e];
                at = base + off[e];
            }
            s_c[tid] = mine;
            s_at[tid] = at;
        }
        if (!__syncthreads_or(mine != 0)) return;  // (uniform) nothing to write: no row is read
#pragma unroll
        for (uint32_t q = 0; q < QG; ++q) act |= (s_c[q] != 0 ? 1u : 0u) << q;
        act = (uint32_t)__builtin_amdgcn_readfirstlane((int)act);
    }
    for (uint32_t e = tid; e < QG * W; e += kScanBlock) qs[e] = e / W < qn ? Q[(size_t)(q0 + e / W) * W + e % W] : 0u;
    uint32_t cut[QG];  // (uniform addresses: hcut has QG entries of padding behind the last query)
#pragma unroll
    for (uint32_t q = 0; q < QG; ++q) cut[q] = hcut[q0 + q];
    __syncthreads();
    if constexpr (MODE == BIN_COUNT) {
        uint32_t c[QG / 4];  // the lane's hits per query, four queries to a word: at most 2 * 16 per block, a byte each
#pragma unroll
        for (uint32_t q = 0; q < QG / 4; ++q) c[q] = 0;
        for (uint64_t b0 = lo; b0 < hi; b0 += kBinRangeStep) {
            uint64_t r[kScanRR];
            bool ok[kScanRR];
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) {
                r[j] = b0 + tid + (uint64_t)j * kScanBlock;
                ok[j] = r[j] < hi;
            }
            if constexpr (MASKED) {
                const uint32_t nwords = (uint32_t)((n + 31) >> 5), wvu = bin_wave();
                uint64_t m[kScanRR];
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) m[j] = bin_mask64(mask, nwords, b0 + (uint64_t)j * kScanBlock + wvu * 64u, hi);
                if (!(m[0] | m[1])) continue;  // (uniform; no barrier in this loop)
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) ok[j] = (m[j] >> lane) & 1ull;
            }
            uint32_t h[kScanRR][QG];
            bin_hamming<QG, V4>(P, r, ok, W, qs, h);
#pragma unroll
            for (uint32_t q = 0; q < QG; ++q)
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) c[q / 4] += (ok[j] && h[j][q] <= cut[q]) ? 1u << (8 * (q % 4)) : 0u;
        }
#pragma unroll
        for (uint32_t q = 0; q < QG; ++q) {
            uint32_t v = (c[q / 4] >> (8 * (q % 4))) & 0xFFu;
#pragma unroll
            for (uint32_t o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o);
            if (lane == 0) wt[0][q][wv] = v;
        }
        __syncthreads();
        if (tid < qn) cnt[(size_t)(q0 + tid) * nblk + blockIdx.x] = wt[0][tid][0] + wt[0][tid][1] + wt[0][tid][2] + wt[0][tid][3];
    } else {
        const unsigned long long below = (1ull << lane) - 1ull;
        const uint32_t mk0 = wv > 0 ? 0xFFFFFFFFu : 0u, mk1 = wv > 1 ? 0xFFFFFFFFu : 0u, mk2 = wv > 2 ? 0xFFFFFFFFu : 0u;
        uint32_t run[QG];  // the block's hits of earlier steps per query (uniform)
#pragma unroll
        for (uint32_t q = 0; q < QG; ++q) run[q] = 0;
        uint32_t buf = 0;
        for (uint64_t b0 = lo; b0 < hi; b0 += kBinRangeStep, buf ^= 1u) {  // (uniform bounds: every wave meets every barrier)
            uint64_t r[kScanRR];
            bool ok[kScanRR];
#pragma unroll
            for (uint32_t j = 0; j < kScanRR; ++j) {
                r[j] = b0 + tid + (uint64_t)j * kScanBlock;
                ok[j] = r[j] < hi;
            }
            [[maybe_unused]] uint64_t m[kScanRR] = {~0ull, ~0ull};  // the wave's allowed rows at (step, j)
            if constexpr (MASKED) {
                const uint32_t nwords = (uint32_t)((n + 31) >> 5), wvu = bin_wave();
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j) {
                    m[j] = bin_mask64(mask, nwords, b0 + (uint64_t)j * kScanBlock + wvu * 64u, hi);
                    ok[j] = (m[j] >> lane) & 1ull;
                }
            }
            uint32_t h[kScanRR][QG];
            if (!MASKED || (m[0] | m[1])) {  // (uniform)
                bin_hamming<QG, V4>(P, r, ok, W, qs, h);
            } else {  // no allowed row: ok is false in every lane, zero totals for the barrier below, and no h is ever a hit
#pragma unroll
                for (uint32_t j = 0; j < kScanRR; ++j)
#pragma unroll
                    for (uint32_t q = 0; q < QG; ++q) h[j][q] = 0;
            }
            uint32_t mine = 0, any = 0;  // mine: lane q holds the wave's totals of query q; any: the wave has a hit (uniform)
            if (!MASKED || (m[0] | m[1])) {
#pragma unroll
                for (uint32_t q = 0; q < QG; ++q) {
                    if (!((act >> q) & 1u)) continue;
                    const unsigned long long m0 = __ballot(ok[0] && h[0][q] <= cut[q]);
                    const unsigned long long m1 = __ballot(ok[1] && h[1][q] <= cut[q]);
                    const uint32_t pk = (uint32_t)__popcll(m0) | ((uint32_t)__popcll(m1) << 16);
                    mine = lane == q ? pk : mine;
                    any |= pk;
                }
            }
            if (lane < QG) wt[buf][lane][wv] = mine;
            if (!__syncthreads_or(any != 0)) continue;  // (uniform) no hit in the step
#pragma unroll
            for (uint32_t q = 0; q < QG; ++q) {
                if (!((act >> q) & 1u)) continue;
                const uint4 w = *reinterpret_cast<const uint4 *>(&wt[buf][q][0]);
                const uint32_t pt = (uint32_t)__builtin_amdgcn_readfirstlane((int)(w.x + w.y + w.z + w.w));
                asm volatile("" ::: "memory");  // (keeps the 32 LDS reads of this loop in their iterations: registers)
                if (pt == 0) continue;
                const uint32_t pb = (w.x & mk0) + (w.y & mk1) + (w.z & mk2);  // the earlier waves' totals
                const uint32_t t0 = pt & 0xFFFFu;
                const bool hit0 = ok[0] && h[0][q] <= cut[q], hit1 = ok[1] && h[1][q] <= cut[q];
                const unsigned long long m0 = __ballot(hit0), m1 = __ballot(hit1);
                if (hit0) {
                    const unsigned long long slot = s_at[q] + run[q] + (pb & 0xFFFFu) + (uint32_t)__popcll(m0 & below);
                    const float v = S[h[0][q]];
                    idx_out[slot] = (uint32_t)r[0];
                    dist_out[slot] = root ? sqrtf(v) : v;
                }
                if (hit1) {
                    const unsigned long long slot = s_at[q] + run[q] + t0 + (pb >> 16) + (uint32_t)__popcll(m1 & below);
                    const float v = S[h[1][q]];
                    idx_out[slot] = (uint32_t)r[1];
                    dist_out[slot] = root ? sqrtf(v) : v;
                }
                run[q] += t0 + (pt >> 16);
            }
        }
    }
}

template <uint32_t QG, bool V4>
int bin_range_launch(int mode, dim3 grid, size_t lds, const uint32_t *P, uint64_t n, uint32_t W, const uint32_t *Q, uint32_t nb,
                     const uint32_t *hcut, uint32_t nblk, uint32_t *cnt, const unsigned long long *off, unsigned long long base,
                     const float *S, int root, uint32_t *idx_out, float *dist_out, const uint32_t *mask, hipStream_t stream) {
    if (mask) {
        if (mode == BIN_COUNT)
            hipLaunchKernelGGL((k_bin_range<QG, V4, BIN_COUNT, const uint32_t *>), grid, dim3(kScanBlock), lds, stream, P, n, W, Q, nb, hcut, nblk,
                               cnt, off, base, S, root, idx_out, dist_out, mask);
        else
            hipLaunchKernelGGL((k_bin_range<QG, V4, BIN_FILL, const uint32_t *>), grid, dim3(kScanBlock), lds, stream, P, n, W, Q, nb, hcut, nblk,
                               cnt, off, base, S, root, idx_out, dist_out, mask);
        VQ_LAUNCH_CHECK("k_bin_range (masked)");
        return VQHIP_OK;
    }
    if (mode == BIN_COUNT)
        hipLaunchKernelGGL((k_bin_range<QG, V4, BIN_COUNT>), grid, dim3(kScanBlock), lds, stream, P, n, W, Q, nb, hcut, nblk, cnt, off,
                           base, S, root, idx_out, dist_out);
    else
        hipLaunchKernelGGL((k_bin_range<QG, V4, BIN_FILL>), grid, dim3(kScanBlock), lds, stream, P, n, W, Q, nb, hcut, nblk, cnt, off,
                           base, S, root, idx_out, dist_out);
    VQ_LAUNCH_CHECK("k_bin_range");
    return VQHIP_OK;
}

int bin_range_scan(int mode, const uint32_t *P, uint64_t n, uint32_t W, uint32_t d, const uint32_t *Q, uint32_t nb,
                   const uint32_t *hcut, uint32_t nblk, uint32_t *cnt, const unsigned long long *off, unsigned long long base,
                   const float *S, int root, uint32_t *idx_out, float *dist_out, const uint32_t *mask, hipStream_t stream) {
    const uint32_t qg = bin_qg(d);
    const dim3 grid(nblk, (nb + qg - 1) / qg);
    const size_t lds = (size_t)qg * W * 4;  // at most 8 KB (QG = 8, W = 256): k_bin_scan's words without its histogram
    const bool v4 = W % 4 == 0;
    if (qg == 32)
        return v4 ? bin_range_launch<32, true>(mode, grid, lds, P, n, W, Q, nb, hcut, nblk, cnt, off, base, S, root, idx_out, dist_out, mask, stream)
                  : bin_range_launch<32, false>(mode, grid, lds, P, n, W, Q, nb, hcut, nblk, cnt, off, base, S, root, idx_out, dist_out, mask, stream);
    return v4 ? bin_range_launch<8, true>(mode, grid, lds, P, n, W, Q, nb, hcut, nblk, cnt, off, base, S, root, idx_out, dist_out, mask, stream)
              : bin_range_launch<8, false>(mode, grid, lds, P, n, W, Q, nb, hcut, nblk, cnt, off, base, S, root, idx_out, dist_out, mask, stream);
}

uint32_t bin_range_blocks(uint64_t n) { return (uint32_t)((n + kBinRangeRows - 1) / kBinRangeRows); }

}  // namespace

// Queries per batch: 1024 as a search, fewer where the batch would have more than 2^17 count entries (nb * ceil(n / 8192)
// <= 2^17 whenever nb > 1, in whole query groups while there are any): k_range_scan is one workgroup, and 65 536 entries
// cost it 0.10 ms.  A single-query batch over n < 2^32 rows has at most 2^19 entries.
uint32_t binary_range_batch(uint64_t n, uint32_t d, uint32_t nq) {
    const uint64_t nblk = bin_range_blocks(n);
    uint64_t nb = std::min<uint64_t>(std::max<uint32_t>(nq, 1), 1024);
    if (nb * nblk > kBinRangeEntries) {
        nb = std::max<uint64_t>(1, kBinRangeEntries / nblk);
        const uint32_t qg = bin_qg(d);
        if (nb >= qg) nb -= nb % qg;
    }
    return (uint32_t)nb;
}

// range.hpp's workspace over qb = binary_range_batch(n, d, nq) queries of bin_range_blocks(n) count entries
size_t binary_range_ws_bytes(uint64_t n, uint32_t d, uint32_t nq) {
    return range_ws_entries((size_t)binary_range_batch(n, d, nq) * bin_range_blocks(n));
}

int launch_binary_range(const uint32_t *P, uint64_t n, uint32_t d, int metric, const float *S, const float *queries_dev, float thr,
                        uint32_t high, uint32_t nq, const uint32_t *hcut, uint64_t max_results, uint32_t *qw, void *range_ws,
                        RangeOut *out, hipStream_t stream, const uint32_t *mask) {
    VQ_TRY(range_begin(out, nq, max_results, stream));
    const uint32_t W = bin_words(d), nblk = bin_range_blocks(n), qb = binary_range_batch(n, d, nq);
    const int root = metric == VQHIP_EUCLIDEAN ? 1 : 0;
    const RangeWs w = vqhip::range_ws(range_ws, qb, nblk);
    for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
        const uint32_t nb = std::min(qb, nq - q0);
        VQ_TRY(launch_bq_pack(queries_dev + (size_t)q0 * d, VQHIP_BINARY_F32, nb, d, thr, high, qw, stream));
        VQ_TRY(bin_range_scan(BIN_COUNT, P, n, W, d, qw, nb, hcut + q0, nblk, w.cnt, w.off, 0, S, root, nullptr, nullptr, mask, stream));
        uint64_t got = 0;
        VQ_TRY(range_scan_room(w, nb, nblk, q0, max_results, out, &got, stream));
        if (got == 0) continue;
        VQ_TRY(bin_range_scan(BIN_FILL, P, n, W, d, qw, nb, hcut + q0, nblk, w.cnt, w.off, (unsigned long long)out->total, S, root,
                              out->idx.as<uint32_t>(), out->dist.as<float>(), mask, stream));
        out->total += got;
    }
    VQ_HIP(hipStreamSynchronize(stream));  // *out is complete on return
    return VQHIP_OK;
}

}  // namespace vqhip
