// k_compact.hip -- stable compaction of resident rows under a remove mask (include/vqhip.h, "adding and removing rows";
// DESIGN.md section 26).  n rows of rb bytes at src, a remove mask of ceil(n / 32) words on the device; the na survivors
// go to dst in their old order.  Schedule: count / scan / move, as range.hpp's and ivf_view.hpp's --
//   k_compact_count  one lane per mask word: the rows it keeps (a popcount), summed over the 32 words of a block of 1024
//                    rows through shuffles -> cnt[blk]
//   k_compact_scan   one workgroup: the exclusive scan of cnt, 1024 entries at a time with a running carry -> start[blk],
//                    start[nblk] = na
//   k_compact_move   one workgroup per block, one wave per group of 64 rows: the group's survivors are one contiguous
//                    run of dst, which the wave walks in units of 16, 4 or 1 bytes (compact.hpp); a lane finds its unit's
//                    source row as the k-th clear bit of the group's two mask words.  Both sides coalesce: the run is
//                    contiguous, and the source is the group's 64 rows with the removed ones skipped.  A block or a group
//                    without a survivor loads nothing.
// No atomics: the same call gives the same bytes on every run.  The compaction is out of place -- src and dst never
// overlap -- because a workgroup's run may lie where another's source rows are.
#include "compact.hpp"
#include "kernels.hpp"

namespace vqhip {
namespace {

__global__ __launch_bounds__(kCompactThreads) void k_compact_count(const uint32_t *__restrict__ remove, uint64_t n, uint32_t nblk,
                                                                   uint32_t *__restrict__ cnt) {
    const uint64_t w = (uint64_t)blockIdx.x * kCompactThreads + threadIdx.x;  // the lane's mask word
    uint32_t c = w * 32 < n ? compact_popc32(compact_keep_word(remove[w], w, n)) : 0u;
#pragma unroll
    for (uint32_t o = 16; o >= 1; o >>= 1) c += (uint32_t)__shfl_xor((int)c, (int)o);  // (stays within a half wave: one block)
    const uint64_t blk = w >> 5;
    if ((threadIdx.x & 31u) == 0 && blk < nblk) cnt[blk] = c;
}

// Exclusive scan of cnt[0 .. nblk) by one workgroup, kCompactScan entries at a time with a running carry: at most 2^22
// entries (n < 2^32).  start[nblk] = na <= n < 2^32.
__global__ __launch_bounds__(kCompactScan) void k_compact_scan(const uint32_t *__restrict__ cnt, uint32_t nblk,
                                                               uint32_t *__restrict__ start) {
    __shared__ uint32_t wsum[kCompactScan / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = 0;  // replicated in every thread (uniform updates)
    for (uint32_t e0 = 0; e0 < nblk; e0 += kCompactScan) {
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
        for (uint32_t w = 0; w < kCompactScan / 64; ++w) {
            if (w < wv) before += wsum[w];
            chunk += wsum[w];
        }
        if (e < nblk) start[e] = before + x - c;
        carry += chunk;
        __syncthreads();  // wsum is rewritten by the next pass
    }
    if (tid == 0) start[nblk] = carry;
}

// U: the unit (uint4, uint32_t or uint8_t); rb is a multiple of sizeof(U) and src and dst are aligned to it.  Every wave
// reads the block's 32 mask words (lanes 0 .. 31) and scans their keep counts, so that a group's first destination row
// needs no LDS and no barrier; wave v then moves groups v, v + 4, v + 8 and v + 12.
template <class U>
__global__ __launch_bounds__(kCompactThreads) void k_compact_move(const uint32_t *__restrict__ remove, uint64_t n,
                                                                  const uint32_t *__restrict__ start, const U *__restrict__ src,
                                                                  U *__restrict__ dst, uint64_t rb) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t at = start[blockIdx.x];
    if (start[blockIdx.x + 1] == at) return;  // (uniform) no survivor in this block
    const uint64_t w = (uint64_t)blockIdx.x * (kCompactBlock / 32) + lane;
    const uint32_t keep = (lane < 32 && w * 32 < n) ? compact_keep_word(remove[w], w, n) : 0u;
    const uint32_t c = compact_popc32(keep);
    uint32_t x = c;
#pragma unroll
    for (uint32_t o = 1; o < 32; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o);
        if (lane >= o) x += y;
    }
    const uint32_t excl = x - c;  // rows the block keeps in front of the lane's word
    const uint64_t upr = compact_units_per_row(rb, (uint32_t)sizeof(U));
    for (uint32_t g = wv; g < kCompactBlock / kCompactGroup; g += kCompactThreads / 64) {
        const uint32_t lo = (uint32_t)__shfl((int)keep, (int)(2 * g)), hi = (uint32_t)__shfl((int)keep, (int)(2 * g + 1));
        const uint32_t before = (uint32_t)__shfl((int)excl, (int)(2 * g));
        const uint64_t keep64 = (uint64_t)lo | ((uint64_t)hi << 32);
        const uint32_t kept = compact_popc64(keep64);
        if (kept == 0) continue;  // (uniform)
        const uint64_t src_row0 = (uint64_t)blockIdx.x * kCompactBlock + (uint64_t)g * kCompactGroup;
        const uint64_t dst_row0 = (uint64_t)at + before;
        const uint64_t total = (uint64_t)kept * upr;  // units of the run
#pragma unroll 4
        for (uint64_t u = lane; u < total; u += 64) {
            uint32_t rank;
            uint64_t within;
            compact_unit_row(u, upr, &rank, &within);
            const uint64_t row = src_row0 + compact_kth_set(keep64, rank);  // (< n: keep64 has no bit at or past n)
            dst[compact_dst_offset(dst_row0, rb, u, (uint32_t)sizeof(U)) / sizeof(U)] =
                src[compact_src_offset(row, rb, within, (uint32_t)sizeof(U)) / sizeof(U)];
        }
    }
}

template <class U>
int move_launch(const uint32_t *remove, uint64_t n, const uint32_t *start, const void *src, void *dst, uint64_t rb, hipStream_t stream) {
    hipLaunchKernelGGL(k_compact_move<U>, dim3(compact_blocks(n)), dim3(kCompactThreads), 0, stream, remove, n, start,
                       static_cast<const U *>(src), static_cast<U *>(dst), rb);
    VQ_LAUNCH_CHECK("k_compact_move");
    return VQHIP_OK;
}

}  // namespace

// start [nblk + 1] | cnt [nblk]
size_t compact_ws_bytes(uint64_t n) { return ((size_t)2 * compact_blocks(n) + 1) * 4; }
const uint32_t *compact_survivors(const void *ws, uint64_t n) { return static_cast<const uint32_t *>(ws) + compact_blocks(n); }

int launch_compact_plan(const uint32_t *remove_dev, uint64_t n, void *ws, hipStream_t stream) {
    const uint32_t nblk = compact_blocks(n);
    uint32_t *start = static_cast<uint32_t *>(ws), *cnt = start + nblk + 1;
    if (nblk) {
        hipLaunchKernelGGL(k_compact_count, dim3((nblk + 7) / 8), dim3(kCompactThreads), 0, stream, remove_dev, n, nblk, cnt);
        VQ_LAUNCH_CHECK("k_compact_count");
    }
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(kCompactScan), 0, stream, cnt, nblk, start);
    VQ_LAUNCH_CHECK("k_compact_scan");
    return VQHIP_OK;
}

int launch_compact_move(const uint32_t *remove_dev, uint64_t n, const void *ws, const void *src, void *dst, uint64_t rb,
                        hipStream_t stream) {
    if (n == 0 || rb == 0) return VQHIP_OK;
    const uint32_t *start = static_cast<const uint32_t *>(ws);
    switch (compact_unit(rb, reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst))) {
        case 16: return move_launch<uint4>(remove_dev, n, start, src, dst, rb, stream);
        case 4: return move_launch<uint32_t>(remove_dev, n, start, src, dst, rb, stream);
        default: return move_launch<uint8_t>(remove_dev, n, start, src, dst, rb, stream);
    }
}

}  // namespace vqhip
