// ivf_range.hpp -- the exact range stage behind vqhip_ivfflat_range_search, vqhip_ivfsq_range_search and
// vqhip_ivfbin_range_search (k_ivfflat.hip): range.hpp's threshold compaction over the RAGGED
// distances the inverted-file distance kernels leave -- W[q][0 .. |S(q)|), a query's positions in probe-slot order
// (IvffRows, ivf_plan.hpp) -- followed by a segmented sort that puts each query's hits in ascending row id.  Semantics
// (include/vqhip.h): row i is a hit of query q iff i is in S(q) and W[q][pos(i)] <= radii[q] as an f32 comparison (NaN
// never hits, -0.0 <= 0.0 holds).
//   range_passes   (range.hpp, over IvffRows) count, scan, room and the fill: each hit (ids[row of its position], D) at
//                  off[q][blk] + its rank in the block, into a staging area of the batch -- position order
//   k_ivfr_sort    block = query, one launch per 8 bits of the row id (ceil(log2 n) bits in all): a stable LSD radix pass
//                  over the query's segment, staging areas in turn, the last pass landing in the result at `base`
// One probed list (nprobe == 1): positions are in row order already, and the fill writes the result itself.
//
// The sort pass.  A workgroup of four waves owns one query's segment [lims[q], lims[q + 1]); wave w owns the w-th quarter
// of it (contiguous).  (1) every wave counts its quarter's digits into hist[w][256] (LDS integer atomics: counts only);
// (2) thread t (= digit t) turns them into first slots, hist[w][t] = the elements with a smaller digit + those with
// digit t in earlier waves -- so slots follow (digit, position), which is what makes the pass stable; (3) every wave walks
// its quarter 64 elements at a time: the lanes holding a lane's digit (eight ballots), the lane's rank among them (a
// popcount below the lane), slot = hist[w][digit] + rank, and the last lane of each digit moves hist[w][digit] on.  No
// slot depends on the order of an atomic, so the same call gives the same arrays on every run.
#pragma once
#include "ivf_plan.hpp"
#include "range.hpp"

namespace vqhip {
namespace {

constexpr uint32_t kIvfrSortThreads = 256;                    // (= the digits of a pass: thread t scans digit t)
constexpr uint32_t kIvfrSortWaves = kIvfrSortThreads / 64;  // quarters of a segment

// One stable pass of the segmented LSD radix sort over bits [shift, shift + 8) of the row id.  lims: the result's lims at
// the batch's first query (lims[q] .. lims[q + 1] is query q's segment, from `base` = lims[0]); src / dst point at the
// batch's first hit (a staging area, or the result at `base`).  Elements never leave their segment.
__attribute__((unused)) __global__ __launch_bounds__(kIvfrSortThreads) void k_ivfr_sort(
    const unsigned long long *__restrict__ lims, unsigned long long base, const uint32_t *__restrict__ src_idx,
    const float *__restrict__ src_dist, uint32_t *__restrict__ dst_idx, float *__restrict__ dst_dist, uint32_t shift) {
    __shared__ uint32_t hist[kIvfrSortWaves][256];
    __shared__ uint32_t wsum[kIvfrSortWaves];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const unsigned long long s0 = lims[q] - base;                   // the segment's first element: 64-bit
    const uint32_t cnt = (uint32_t)(lims[q + 1] - lims[q]);         // (at most |S(q)| < 2^32)
    if (cnt == 0) return;                                           // (uniform)
    src_idx += s0, src_dist += s0, dst_idx += s0, dst_dist += s0;
#pragma unroll
    for (uint32_t w = 0; w < kIvfrSortWaves; ++w) hist[w][tid] = 0u;
    __syncthreads();
    const uint32_t per = (uint32_t)(((uint64_t)cnt + kIvfrSortWaves - 1) / kIvfrSortWaves);
    const uint32_t a = (uint32_t)min((uint64_t)cnt, (uint64_t)wv * per), b = (uint32_t)min((uint64_t)cnt, (uint64_t)a + per);
    for (uint64_t e = (uint64_t)a + lane; e < b; e += 64) atomicAdd(&hist[wv][(src_idx[e] >> shift) & 255u], 1u);
    __syncthreads();
    {  // thread t: digit t.  Exclusive scan of the digits' totals, then the waves' first slots in wave order
        uint32_t c[kIvfrSortWaves], tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < kIvfrSortWaves; ++w) {
            c[w] = hist[w][tid];
            tot += c[w];
        }
        uint32_t x = tot;  // inclusive scan within the wave
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        uint32_t run = x - tot;
#pragma unroll
        for (uint32_t w = 0; w < kIvfrSortWaves; ++w)
            if (w < wv) run += wsum[w];
#pragma unroll
        for (uint32_t w = 0; w < kIvfrSortWaves; ++w) {
            hist[w][tid] = run;
            run += c[w];
        }
    }
    __syncthreads();
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (uint32_t it = 0; it < (per + 63) / 64; ++it) {  // (uniform: every wave makes the passes of a whole quarter)
        const uint64_t e = (uint64_t)a + (uint64_t)it * 64 + lane;
        const bool valid = e < b;
        uint32_t id = 0, digit = 0;
        float dv = 0.0f;
        if (valid) {
            id = src_idx[e];
            dv = src_dist[e];
            digit = (id >> shift) & 255u;
        }
        unsigned long long peer = __ballot(valid);  // the wave's lanes holding this lane's digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const bool one = (digit >> bit) & 1u;
            const unsigned long long m = __ballot(valid && one);
            peer &= one ? m : ~m;
        }
        uint32_t slot = 0;
        if (valid) slot = hist[wv][digit] + (uint32_t)__popcll(peer & lower);
        __syncthreads();                                                    // every lane has read its first slot
        if (valid && (peer >> lane) == 1ull) hist[wv][digit] = slot + 1u;  // the digit's last lane moves it on
        __syncthreads();
        if (valid) {
            dst_idx[slot] = id;
            dst_dist[slot] = dv;
        }
    }
}

// radix passes over the ids of an index of n rows: 8 bits each over the ceil(log2 n) significant ones, at least one
inline uint32_t ivfr_passes(uint64_t n) {
    uint32_t bits = 0;
    while (bits < 32 && (1ull << bits) < n) ++bits;
    return std::max<uint32_t>(1, (bits + 7) / 8);
}

// The stage over one batch v: W [nb][wstride] on the device (queued on `stream`) with the batch's plan in pref / seg,
// radii [nb] on the device, ws >= range_ws_size(wstride, nb), q0 the batch's first query in the result.  *stage: the
// staging areas, grown here to the batch's hits (16 bytes each).  Waits for the stream once.  A batch that takes the
// result past max_results is VQHIP_ERR_UNSUPPORTED.
// k_range_scan's one-workgroup bound holds unchanged: a batch of several queries keeps nb * wstride <= 2^28 floats of W
// (ivf_batch, api_ivf.hip), so it has at most nb * ceil(wstride / 4096) <= 2^16 + nb entries, and a single-query batch at most
// 2^20 (wstride < 2^32).
inline int ivfr_batch(const IvfBatchView &v, uint32_t q0, const float *radii, void *ws, DevBuf *stage, uint64_t max_results,
                      RangeOut *out, hipStream_t stream) {
    const uint64_t base = out->total;  // lims[q0] = base: the batch's first hit
    const uint32_t passes = v.nprobe == 1 ? 0 : ivfr_passes(v.n);
    uint32_t *res_idx = nullptr, *a_idx = nullptr, *b_idx = nullptr;
    float *res_dist = nullptr, *a_dist = nullptr, *b_dist = nullptr;
    uint64_t got = 0;
    VQ_TRY(range_passes<IvffRows>({v.W, v.wstride, v.pref, v.seg, v.ids, v.nprobe}, v.nb, q0, radii, ws, max_results, out, &got, stream,
                                  [&](uint64_t g, uint32_t **idx, float **dist) -> int {
        res_idx = out->idx.as<uint32_t>() + base;
        res_dist = out->dist.as<float>() + base;
        // staging areas A and B of the batch: idx | dist each; B only where a pass has to land outside A and the result
        if (passes) {
            VQ_TRY(stage->ensure((size_t)g * 4 * (passes > 1 ? 4 : 2)));
            a_idx = stage->as<uint32_t>();
            a_dist = reinterpret_cast<float *>(a_idx + g);
            if (passes > 1) {
                b_idx = a_idx + 2 * g;
                b_dist = reinterpret_cast<float *>(b_idx + g);
            }
        }
        *idx = passes ? a_idx : res_idx;
        *dist = passes ? a_dist : res_dist;
        return VQHIP_OK;
    }));
    if (got == 0) return VQHIP_OK;
    const unsigned long long *lims = out->lims.as<unsigned long long>() + q0;
    for (uint32_t p = 0; p < passes; ++p) {  // A -> B -> A ..., the last pass into the result
        const bool from_a = (p & 1u) == 0, last = p + 1 == passes;
        hipLaunchKernelGGL(k_ivfr_sort, dim3(v.nb), dim3(kIvfrSortThreads), 0, stream, lims, (unsigned long long)base,
                           from_a ? a_idx : b_idx, from_a ? a_dist : b_dist, last ? res_idx : (from_a ? b_idx : a_idx),
                           last ? res_dist : (from_a ? b_dist : a_dist), 8 * p);
        VQ_LAUNCH_CHECK("k_ivfr_sort");
    }
    out->total = base + got;
    return VQHIP_OK;
}

}  // namespace
}  // namespace vqhip
