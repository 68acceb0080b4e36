// ivf_view.hpp -- the view of a filtered call on an inverted file (include/vqhip.h, vqhip_ivfflat_*_masked and
// vqhip_ivfsq_*_masked): the inverted file of the allowed rows, built once per call on the device.
// The index in list order is ids [n] and off [nlist + 1] (ivf_plan.hpp); the call's row mask `allowed` has ceil(n / 32)
// words, row i allowed iff bit i & 31 of word i >> 5 is set.  The view is
//   pick [na]         the list-order positions g of the allowed rows, ascending -- so grouped by list, and ascending in row
//                     id within a list
//   aids [na]         aids[j] = ids[pick[j]]
//   aoff [nlist + 1]  aoff[l] = the allowed positions below off[l]: list l of the view is the run aoff[l] .. aoff[l + 1]
// and every stage behind the distances (plan, histogram, selection, range) runs over {aoff, aids} as it runs over
// {off, ids}; the distance kernels read row pick[j] of the payload for row j of the view (PickedRows, ivf_tile.hpp).
// Schedule: count / scan / fill, as range.hpp's --
//   k_ivfv_count   block = kIvfvBlock positions: the allowed ones among them -> cnt[blk] (ballots and a sum of four wave
//                  counts through LDS)
//   k_ivfv_scan    one workgroup: the exclusive scan of cnt, 1024 entries at a time with a running carry -> start[blk],
//                  start[nblk] = na
//   k_ivfv_fill    the count's grid: every allowed position g goes to slot start[blk] + its rank in the block
//   k_ivfv_off     one thread per list boundary: aoff[l] = the lower bound of off[l] in pick[0 .. na)
// No atomics: the same call gives the same arrays on every run.  n < 2^32, so positions and counts are u32.  A position
// reads ids[g] and one mask word; the mask is n / 8 bytes and stays in cache.  Every including file gets its own copy (an
// anonymous namespace).
#pragma once
#include "common.hpp"

namespace vqhip {
namespace {

constexpr uint32_t kIvfvThreads = 256;                           // four waves
constexpr uint32_t kIvfvPasses = 4;                              // positions per lane
constexpr uint32_t kIvfvBlock = kIvfvThreads * kIvfvPasses;  // positions per workgroup: 1024
constexpr uint32_t kIvfvScan = 1024;                             // count entries the scan takes per pass

// whether position g (pass s of the block at g0) exists and its row is allowed
__device__ __forceinline__ bool ivfv_allowed(const uint32_t *__restrict__ allowed, const uint32_t *__restrict__ ids, uint64_t n,
                                             uint64_t g) {
    if (g >= n) return false;
    const uint32_t id = ids[g];  // (< n: the mask has its word)
    return (allowed[id >> 5] >> (id & 31u)) & 1u;
}

__global__ __launch_bounds__(kIvfvThreads) void k_ivfv_count(const uint32_t *__restrict__ allowed, const uint32_t *__restrict__ ids,
                                                             uint64_t n, uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kIvfvThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * kIvfvBlock;
    uint32_t c = 0;  // the wave's allowed positions (uniform)
#pragma unroll
    for (uint32_t s = 0; s < kIvfvPasses; ++s)
        c += (uint32_t)__popcll(__ballot(ivfv_allowed(allowed, ids, n, g0 + s * kIvfvThreads + tid)));
    if ((tid & 63u) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Exclusive scan of cnt[0 .. nblk) by one workgroup, kIvfvScan entries at a time with a running carry: at most 2^22
// entries (n < 2^32), 4096 passes of two barriers each beside a search over 2^32 rows.  start[nblk] = na <= n < 2^32.
__global__ __launch_bounds__(kIvfvScan) void k_ivfv_scan(const uint32_t *__restrict__ cnt, uint32_t nblk, uint32_t *__restrict__ start) {
    __shared__ uint32_t wsum[kIvfvScan / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = 0;  // replicated in every thread (uniform updates)
    for (uint32_t e0 = 0; e0 < nblk; e0 += kIvfvScan) {
        const uint32_t e = e0 + tid;  // (nblk <= 2^22: no wrap)
        const uint32_t c = e < nblk ? cnt[e] : 0u;
        uint32_t x = c;  // inclusive scan within the wave
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        uint32_t before = carry, chunk = 0;
#pragma unroll
        for (uint32_t w = 0; w < kIvfvScan / 64; ++w) {
            if (w < wv) before += wsum[w];
            chunk += wsum[w];
        }
        if (e < nblk) start[e] = before + x - c;
        carry += chunk;
        __syncthreads();  // wsum is rewritten by the next pass
    }
    if (tid == 0) start[nblk] = carry;
}

// ascending position is the order (pass, wave, lane): the rank of an allowed position in its block is the allowed ones of
// earlier passes and of earlier waves of its pass (16 wave totals through LDS) + those of lower lanes of its wave
__global__ __launch_bounds__(kIvfvThreads) void k_ivfv_fill(const uint32_t *__restrict__ allowed, const uint32_t *__restrict__ ids,
                                                            uint64_t n, const uint32_t *__restrict__ start,
                                                            uint32_t *__restrict__ pick, uint32_t *__restrict__ aids) {
    __shared__ uint32_t wsum[kIvfvPasses][kIvfvThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t at = start[blockIdx.x];
    if (start[blockIdx.x + 1] == at) return;  // (uniform) nothing allowed in this block
    const uint64_t g0 = (uint64_t)blockIdx.x * kIvfvBlock;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool ok[kIvfvPasses];
    uint32_t pre[kIvfvPasses];
#pragma unroll
    for (uint32_t s = 0; s < kIvfvPasses; ++s) {
        ok[s] = ivfv_allowed(allowed, ids, n, g0 + s * kIvfvThreads + tid);
        const unsigned long long m = __ballot(ok[s]);
        pre[s] = (uint32_t)__popcll(m & below);
        if (lane == 0) wsum[s][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t run = 0;  // the block's allowed positions in front of (pass s, wave w)
#pragma unroll
    for (uint32_t s = 0; s < kIvfvPasses; ++s) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t w = 0; w < kIvfvThreads / 64; ++w) {
            if (w == wv) mine = run;
            run += wsum[s][w];
        }
        if (ok[s]) {  // (an allowed position is below n; its slot below na <= n)
            const uint32_t g = (uint32_t)(g0 + s * kIvfvThreads + tid), slot = at + mine + pre[s];
            pick[slot] = g;
            aids[slot] = ids[g];
        }
    }
}

// aoff[l] for l = 0 .. nlist: the first j with pick[j] >= off[l] (pick ascends), na where there is none
__global__ __launch_bounds__(256) void k_ivfv_off(const uint32_t *__restrict__ off, uint32_t nlist, const uint32_t *__restrict__ pick,
                                                  const uint32_t *__restrict__ na, uint32_t *__restrict__ aoff) {
    const uint32_t l = blockIdx.x * 256 + threadIdx.x;
    if (l > nlist) return;
    const uint32_t o = off[l];
    uint32_t lo = 0, hi = *na;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (pick[mid] < o) lo = mid + 1;
        else hi = mid;
    }
    aoff[l] = lo;
}

inline uint32_t ivfv_blocks(uint64_t n) { return (uint32_t)((n + kIvfvBlock - 1) / kIvfvBlock); }
// start [nblk + 1] | cnt [nblk]
inline size_t ivfv_ws_bytes(uint64_t n) { return ((size_t)2 * ivfv_blocks(n) + 1) * 4; }

inline int ivfv_build(const uint32_t *allowed, const uint32_t *ids, uint64_t n, const uint32_t *off, uint32_t nlist, void *ws,
                      uint32_t *pick, uint32_t *aids, uint32_t *aoff, hipStream_t stream) {
    const uint32_t nblk = ivfv_blocks(n);
    uint32_t *start = reinterpret_cast<uint32_t *>(ws), *cnt = start + nblk + 1;
    if (nblk) {
        hipLaunchKernelGGL(k_ivfv_count, dim3(nblk), dim3(kIvfvThreads), 0, stream, allowed, ids, n, cnt);
        VQ_LAUNCH_CHECK("k_ivfv_count");
    }
    hipLaunchKernelGGL(k_ivfv_scan, dim3(1), dim3(kIvfvScan), 0, stream, cnt, nblk, start);
    VQ_LAUNCH_CHECK("k_ivfv_scan");
    if (nblk) {
        hipLaunchKernelGGL(k_ivfv_fill, dim3(nblk), dim3(kIvfvThreads), 0, stream, allowed, ids, n, start, pick, aids);
        VQ_LAUNCH_CHECK("k_ivfv_fill");
    }
    hipLaunchKernelGGL(k_ivfv_off, dim3(nlist / 256 + 1), dim3(256), 0, stream, off, nlist, pick, start + nblk, aoff);
    VQ_LAUNCH_CHECK("k_ivfv_off");
    return VQHIP_OK;
}

}  // namespace
}  // namespace vqhip
