// ivf_remove.hpp -- the arithmetic of removing rows from an inverted file on the device (include/vqhip.h, "removing rows
// from an inverted file"; the kernels are k_ivf_remove.hip's).  Two things are computed:
//   the renumbering   a surviving row i becomes i - below(i), below(i) the removed rows under i: the exclusive prefix
//                     popcount of the remove mask at word i >> 5 (ivf_below_prefix, filled on the host while it counts
//                     the survivors) plus the popcount of that word's bits under i & 31
//   the take          row j of the destination is row pick[j] of the source, j < na.  The destination is one run of
//                     na * upr units of 16, 4 or 1 bytes (compact.hpp's unit choice); a workgroup takes kIvfTakeBlock
//                     consecutive units in kIvfTakePasses passes of kIvfTakeThreads, so a wave's store is 64 consecutive
//                     units.  A unit's destination row and its offset within the row are compact_unit_row's.
// Everything here is host and device code with no HIP in it when a host compiler reads it, so that both are tested on the
// CPU (tests/cpp/test_ivf_remove_hpp.cpp).
#pragma once
#include <cstdint>

#include "compact.hpp"

namespace vqhip {

constexpr uint32_t kIvfTakeThreads = 256;                                // four waves
constexpr uint32_t kIvfTakePasses = 4;                                   // units per lane
constexpr uint32_t kIvfTakeBlock = kIvfTakeThreads * kIvfTakePasses;  // units per workgroup: 1024

// below(i) for a row i < n: `before` = the set bits of the remove mask in words 0 .. (i >> 5) - 1, `word` = word i >> 5.
// Only bits under i are counted, and i < n, so a bit at or past n never is -- in the last, partial word as elsewhere.
VQ_COMPACT_HD uint32_t ivf_below(uint32_t before, uint32_t word, uint32_t i) {
    return before + compact_popc32(word & ((1u << (i & 31u)) - 1u));
}
// the new id of a surviving row i
VQ_COMPACT_HD uint32_t ivf_new_id(uint32_t before, uint32_t word, uint32_t i) { return i - ivf_below(before, word, i); }

// prefix[w] = the removed rows below row 32 w, for the ceil(n / 32) words of `remove`; returns the rows removed (bits at
// or past n ignored).  Host code: the caller walks the mask once for the count, the prefix and the complement.
inline uint64_t ivf_below_prefix(const uint32_t *remove, uint64_t n, uint32_t *prefix) {
    uint64_t gone = 0;
    for (uint64_t w = 0; w < (n + 31) / 32; ++w) {
        prefix[w] = (uint32_t)gone;
        const uint32_t rows = n - w * 32 >= 32 ? 32u : (uint32_t)(n - w * 32);  // rows of this word
        gone += rows - compact_popc32(compact_keep_word(remove[w], w, n));
    }
    return gone;
}

// the take's grid: workgroups for `units` units
VQ_COMPACT_HD uint64_t ivf_take_blocks(uint64_t units) { return (units + kIvfTakeBlock - 1) / kIvfTakeBlock; }
// the unit of (workgroup, pass, thread): consecutive across the threads of a pass
VQ_COMPACT_HD uint64_t ivf_take_unit(uint64_t block, uint32_t pass, uint32_t tid) {
    return block * kIvfTakeBlock + (uint64_t)pass * kIvfTakeThreads + tid;
}
// unit u of the destination: its row j = *row (the caller reads pick[j]) and the unit within the row
VQ_COMPACT_HD void ivf_take_row(uint64_t u, uint64_t upr, uint32_t *row, uint64_t *within) { compact_unit_row(u, upr, row, within); }
// byte offsets, 64-bit throughout: the source byte of unit `within` of source row `src_row`, the destination byte of unit u
VQ_COMPACT_HD uint64_t ivf_take_src_offset(uint64_t src_row, uint64_t rb, uint64_t within, uint32_t unit) {
    return compact_src_offset(src_row, rb, within, unit);
}
VQ_COMPACT_HD uint64_t ivf_take_dst_offset(uint64_t u, uint32_t unit) { return u * unit; }

}  // namespace vqhip
