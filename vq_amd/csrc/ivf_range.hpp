// ivf_range.hpp -- the exact range stage behind vqhip_ivfflat_range_search and vqhip_ivfsq_range_search (k_ivfflat.hip;
// DESIGN.md section 17): range.hpp's threshold compaction over the RAGGED distances the inverted-file distance kernels
// leave -- W[q][0 .. |S(q)|), a query's positions in probe-slot order (ivf_plan.hpp) -- followed by a segmented sort that
// puts each query's hits in ascending row id.  Semantics (include/vqhip.h): row i is a hit of query q iff i is in S(q) and
// W[q][pos(i)] <= radii[q] as an f32 comparison (NaN never hits, -0.0 <= 0.0 holds).
//   k_ivfr_count   grid (ceil(wstride / 4096), nb): the hits among a block's 4096 positions below |S(q)| -> cnt[q][blk];
//                  k_range_count's lanes, strides and ballots, no atomics; a block past |S(q)| writes 0
//   k_range_scan   (range.hpp, as it is) off[q][blk], the batch's end of every query into lims, the batch total
//   range_room     (range.hpp) the 8-byte read, max_results, range_grow
//   k_ivfr_fill    the count's grid: each hit (ids[row of its position], D) at off[q][blk] + its rank in the block, into a
//                  staging area of the batch -- position order; a block without hits returns before it reads
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

// the four positions p0 .. p0 + 3 of a query's distances wq[0 .. len): v, and bit j set where position p0 + j is a hit.
// VEC: wstride % 4 == 0, so q * wstride + p0 is a multiple of 4 and a float4 at p0 < len lies inside the query's row of W
// (positions from len on hold what an earlier batch left: read, never a hit)
template <bool VEC>
__device__ __forceinline__ uint32_t ivfr_load(const float *__restrict__ wq, uint64_t len, uint64_t p0, float rad, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    uint32_t hits = 0;
    if constexpr (VEC) {
        if (p0 < len) {
            const float4 a = *reinterpret_cast<const float4 *>(wq + p0);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) hits |= ((p0 + j < len && v[j] <= rad) ? 1u : 0u) << j;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (p0 + j < len) {
                v[j] = wq[p0 + j];
                hits |= (v[j] <= rad ? 1u : 0u) << j;
            }
    }
    return hits;
}

__device__ __forceinline__ uint64_t ivfr_len(const uint32_t *__restrict__ pref, uint32_t nprobe, uint32_t q, uint64_t wstride) {
    return min((uint64_t)pref[(size_t)q * (nprobe + 1) + nprobe], wstride);
}

template <bool VEC>
__global__ __launch_bounds__(kRangeThreads) void k_ivfr_count(const float *__restrict__ W, uint64_t wstride,
                                                              const uint32_t *__restrict__ pref, uint32_t nprobe,
                                                              const float *__restrict__ radii, uint32_t nblk,
                                                              uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kRangeThreads / 64];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint64_t len = ivfr_len(pref, nprobe, q, wstride);
    const uint64_t pos0 = (uint64_t)blockIdx.x * kRangeRows;
    if (pos0 >= len) {  // (uniform) past the query's positions
        if (tid == 0) cnt[(size_t)q * nblk + blockIdx.x] = 0u;
        return;
    }
    const float rad = radii[q];
    const float *wq = W + (size_t)q * wstride;
    uint32_t c = 0;  // the wave's hits (uniform)
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        float v[4];
        const uint32_t hits = ivfr_load<VEC>(wq, len, pos0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4, rad, v);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) c += (uint32_t)__popcll(__ballot((hits >> j) & 1u));
    }
    if ((tid & 63u) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) cnt[(size_t)q * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// k_range_fill over positions: slot = off[q][blk] + the block's hits in front, counted from the batch's first hit
// (idx_out / dist_out point at it: the staging area, or the result at `base` when nprobe == 1)
template <bool VEC>
__global__ __launch_bounds__(kRangeThreads) void k_ivfr_fill(const float *__restrict__ W, uint64_t wstride,
                                                             const uint32_t *__restrict__ pref, const uint32_t *__restrict__ seg,
                                                             const uint32_t *__restrict__ ids, uint32_t nprobe,
                                                             const float *__restrict__ radii, uint32_t nblk,
                                                             const uint32_t *__restrict__ cnt,
                                                             const unsigned long long *__restrict__ off,
                                                             uint32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
    __shared__ uint32_t wsum[kRangeStrides][kRangeThreads / 64];
    const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const size_t entry = (size_t)q * nblk + blockIdx.x;
    if (cnt[entry] == 0) return;  // (uniform) nothing to write: the distances are not read again
    const uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    const uint32_t *sq = seg + (size_t)q * nprobe;
    const uint64_t len = min((uint64_t)pq[nprobe], wstride);
    const float rad = radii[q];
    const float *wq = W + (size_t)q * wstride;
    const uint64_t pos0 = (uint64_t)blockIdx.x * kRangeRows;
    const unsigned long long below = (1ull << lane) - 1ull;
    float v[kRangeStrides][4];
    uint32_t hits[kRangeStrides], pre[kRangeStrides];  // pre: the stride's hits in lower lanes of this wave
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        hits[s] = ivfr_load<VEC>(wq, len, pos0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4, rad, v[s]);
        uint32_t p = 0, t = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const unsigned long long m = __ballot((hits[s] >> j) & 1u);
            p += (uint32_t)__popcll(m & below);
            t += (uint32_t)__popcll(m);
        }
        pre[s] = p;
        if (lane == 0) wsum[s][wv] = t;
    }
    __syncthreads();
    const unsigned long long at = off[entry];  // the block's first slot: 64-bit throughout
    uint32_t run = 0;                          // the block's hits in front of (stride s, wave w), in position order
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t w = 0; w < kRangeThreads / 64; ++w) {
            if (w == wv) mine = run;
            run += wsum[s][w];
        }
        unsigned long long slot = at + mine + pre[s];
        const uint64_t p0 = pos0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if ((hits[s] >> j) & 1u) {  // (a hit is below len <= pq[nprobe] < 2^32)
                idx_out[slot] = ids[ivf_row(pq, sq, nprobe, (uint32_t)(p0 + j))];
                dist_out[slot] = v[s][j];
                ++slot;
            }
    }
}

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

// bytes of the stage's workspace for batches of up to qb queries of wstride positions: range.hpp's layout over
// blocks of positions
inline size_t ivfr_ws_size(uint64_t wstride, uint32_t qb) { return range_ws_size(wstride, qb); }

// The stage over one batch: W [nb][wstride] on the device (queued on `stream`) with pref / seg [nb] of the batch's plan,
// ids the index's row ids in list order (n rows in all), radii [nb] on the device, ws >= ivfr_ws_size(wstride, nb), q0
// the batch's first query in the result.  *stage: the staging areas, grown here to the batch's hits (16 bytes each).
// Waits for the stream once.  A batch that takes the result past max_results is VQHIP_ERR_UNSUPPORTED.
// k_range_scan's one-workgroup bound holds unchanged: a batch of several queries keeps nb * wstride <= 2^28 floats of W
// (ivf_batch, api.hip), so it has at most nb * ceil(wstride / 4096) <= 2^16 + nb entries, and a single-query batch at most
// 2^20 (wstride < 2^32).
inline int ivfr_batch(const float *W, uint64_t wstride, const uint32_t *pref, const uint32_t *seg, const uint32_t *ids, uint64_t n,
                      uint32_t nb, uint32_t nprobe, uint32_t q0, const float *radii, void *ws, DevBuf *stage, uint64_t max_results,
                      RangeOut *out, hipStream_t stream) {
    const uint32_t nblk = range_blocks(wstride);
    unsigned long long *total = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *off = total + 2;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(off + (size_t)nb * nblk);
    unsigned long long *lims = out->lims.as<unsigned long long>() + q0;  // lims[0] = out->total: the batch's first hit
    const bool vec = (wstride & 3u) == 0;
    const dim3 grid(nblk, nb), block(kRangeThreads);
    if (vec) hipLaunchKernelGGL(k_ivfr_count<true>, grid, block, 0, stream, W, wstride, pref, nprobe, radii, nblk, cnt);
    else hipLaunchKernelGGL(k_ivfr_count<false>, grid, block, 0, stream, W, wstride, pref, nprobe, radii, nblk, cnt);
    VQ_LAUNCH_CHECK("k_ivfr_count");
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(1024), 0, stream, cnt, nb, nblk, (unsigned long long)out->total, off, lims + 1, total);
    VQ_LAUNCH_CHECK("k_range_scan");
    uint64_t got = 0;
    VQ_TRY(range_room(total, nb, q0, max_results, out, &got, stream));
    if (got == 0) return VQHIP_OK;
    const uint64_t base = out->total;
    uint32_t *res_idx = out->idx.as<uint32_t>() + base;
    float *res_dist = out->dist.as<float>() + base;
    const uint32_t passes = nprobe == 1 ? 0 : ivfr_passes(n);
    // staging areas A and B of the batch: idx | dist each; B only where a pass has to land outside A and the result
    uint32_t *a_idx = nullptr, *b_idx = nullptr;
    float *a_dist = nullptr, *b_dist = nullptr;
    if (passes) {
        VQ_TRY(stage->ensure((size_t)got * 4 * (passes > 1 ? 4 : 2)));
        a_idx = stage->as<uint32_t>();
        a_dist = reinterpret_cast<float *>(a_idx + got);
        if (passes > 1) {
            b_idx = a_idx + 2 * got;
            b_dist = reinterpret_cast<float *>(b_idx + got);
        }
    }
    uint32_t *fill_idx = passes ? a_idx : res_idx;
    float *fill_dist = passes ? a_dist : res_dist;
    if (vec)
        hipLaunchKernelGGL(k_ivfr_fill<true>, grid, block, 0, stream, W, wstride, pref, seg, ids, nprobe, radii, nblk, cnt, off, fill_idx,
                           fill_dist);
    else
        hipLaunchKernelGGL(k_ivfr_fill<false>, grid, block, 0, stream, W, wstride, pref, seg, ids, nprobe, radii, nblk, cnt, off, fill_idx,
                           fill_dist);
    VQ_LAUNCH_CHECK("k_ivfr_fill");
    for (uint32_t p = 0; p < passes; ++p) {  // A -> B -> A ..., the last pass into the result
        const bool from_a = (p & 1u) == 0, last = p + 1 == passes;
        hipLaunchKernelGGL(k_ivfr_sort, dim3(nb), dim3(kIvfrSortThreads), 0, stream, lims, (unsigned long long)base,
                           from_a ? a_idx : b_idx, from_a ? a_dist : b_dist, last ? res_idx : (from_a ? b_idx : a_idx),
                           last ? res_dist : (from_a ? b_dist : a_dist), 8 * p);
        VQ_LAUNCH_CHECK("k_ivfr_sort");
    }
    out->total = base + got;
    return VQHIP_OK;
}

}  // namespace
}  // namespace vqhip
