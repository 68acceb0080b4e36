// compact.hpp -- the arithmetic of a stable row compaction (include/vqhip.h, "adding and removing rows"; DESIGN.md
// section 26; the kernels are k_compact.hip's).  n rows of rb bytes and a remove mask of ceil(n / 32) words, row i
// removed iff bit i & 31 of word i >> 5 is set (bits at or past n ignored): the survivors go to a second buffer in
// their old order.  Rows are taken in groups of 64 (two mask words, one wave) and blocks of kCompactBlock; the survivors
// of a group land in one contiguous run of the destination, which the group's wave walks in units of 16, 4 or 1 bytes.
// Everything here is host and device code with no HIP in it when a host compiler reads it, so that the unit choice, the
// unit -> row mapping and the 64-bit byte offsets are tested on the CPU (tests/cpp/test_compact_hpp.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VQ_COMPACT_HD __host__ __device__ inline
#else
#define VQ_COMPACT_HD inline
#endif

namespace vqhip {

constexpr uint32_t kCompactGroup = 64;     // rows of a group: one wave, two mask words
constexpr uint32_t kCompactThreads = 256;  // four waves
constexpr uint32_t kCompactBlock = 1024;   // rows of a block: 16 groups, 32 mask words, one entry of the scan
constexpr uint32_t kCompactScan = 1024;    // block counts the scan takes per pass

VQ_COMPACT_HD uint32_t compact_popc32(uint32_t x) {
    return (uint32_t)__builtin_popcount(x);
}
VQ_COMPACT_HD uint32_t compact_popc64(uint64_t x) {
    return (uint32_t)__builtin_popcountll(x);
}

// blocks of n rows (n < 2^32: at most 2^22)
VQ_COMPACT_HD uint32_t compact_blocks(uint64_t n) { return (uint32_t)((n + kCompactBlock - 1) / kCompactBlock); }

// The rows that mask word w (rows 32 w .. 32 w + 31) keeps, as bits: the clear bits of `word` below n.  A word wholly at
// or past n keeps nothing (the caller does not read it: the mask has ceil(n / 32) words).
VQ_COMPACT_HD uint32_t compact_keep_word(uint32_t word, uint64_t w, uint64_t n) {
    const uint64_t r0 = w * 32;
    if (r0 >= n) return 0u;
    const uint32_t keep = ~word;
    return n - r0 >= 32 ? keep : keep & ((1u << (uint32_t)(n - r0)) - 1u);
}

// the position of the k-th set bit of `keep`, k counted from 0 and below its popcount: a binary search on popcounts
VQ_COMPACT_HD uint32_t compact_kth_set(uint64_t keep, uint32_t k) {
    uint32_t pos = 0;
    for (uint32_t w = 32; w >= 1; w >>= 1) {  // the bit is among the low 2 w bits of keep
        const uint32_t c = compact_popc64(keep & ((1ull << w) - 1ull));
        if (k >= c) {
            k -= c;
            keep >>= w;
            pos += w;
        }
    }
    return pos;
}
// the k-th clear bit of a group's two remove words (lo: rows 0 .. 31 of the group), k below the number of clear bits
VQ_COMPACT_HD uint32_t compact_kth_clear(uint32_t lo, uint32_t hi, uint32_t k) {
    return compact_kth_set(~((uint64_t)lo | ((uint64_t)hi << 32)), k);
}

// The unit, in bytes, a wave moves per lane: 16 where the row width and both bases are multiples of 16 (every row and
// every run then starts on one), else 4 on the same condition, else 1.
VQ_COMPACT_HD uint32_t compact_unit(uint64_t rb, uint64_t src_base, uint64_t dst_base) {
    const uint64_t a = rb | src_base | dst_base;
    return a % 16 == 0 ? 16u : a % 4 == 0 ? 4u : 1u;
}
VQ_COMPACT_HD uint64_t compact_units_per_row(uint64_t rb, uint32_t unit) { return rb / unit; }

// unit u of a run of whole rows of upr units each: the rank of its row in the run, and the unit within that row
VQ_COMPACT_HD void compact_unit_row(uint64_t u, uint64_t upr, uint32_t *rank, uint64_t *within) {
    if ((u | upr) >> 32) {
        *rank = (uint32_t)(u / upr);
        *within = u % upr;
    } else {  // (the usual case: a 32-bit division)
        const uint32_t u32 = (uint32_t)u, p32 = (uint32_t)upr, r = u32 / p32;
        *rank = r;
        *within = u32 - r * p32;
    }
}

// byte offsets, 64-bit throughout: n * rb passes 2^32 at ordinary sizes
VQ_COMPACT_HD uint64_t compact_row_offset(uint64_t row, uint64_t rb) { return row * rb; }
// the source byte of unit `within` of row `row`
VQ_COMPACT_HD uint64_t compact_src_offset(uint64_t row, uint64_t rb, uint64_t within, uint32_t unit) {
    return compact_row_offset(row, rb) + within * unit;
}
// the destination byte of unit u of the run that starts at destination row `row0`
VQ_COMPACT_HD uint64_t compact_dst_offset(uint64_t row0, uint64_t rb, uint64_t u, uint32_t unit) {
    return compact_row_offset(row0, rb) + u * unit;
}

}  // namespace vqhip
