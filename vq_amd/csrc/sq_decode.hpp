// sq_decode.hpp -- the SQ decode rule in registers, shared by the passes that read resident SQ codes (k_sqindex.hip over
// every row, k_ivfsq.hip over the probed lists): v(c) = mn + (float)c * step for every byte value, two roundings, never
// fused.  Every including file gets its own copy (an anonymous namespace).
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// the SQ decode rule for one byte: two roundings, never fused
__device__ __forceinline__ float sq_val(uint32_t byte, float mn, float step) {
    const float t = (float)byte * step;
    return mn + t;
}

// f(t, v(row[t])) for t = 0 .. d-1 ascending; W4: the row starts on a 4-byte boundary and d % 4 == 0 (dword loads)
template <bool W4, class F>
__device__ __forceinline__ void sq_row_walk(const uint8_t *__restrict__ r, uint32_t d, float mn, float step, F &&f) {
    if constexpr (W4) {
        for (uint32_t t = 0; t < d; t += 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t *>(r + t);
            f(t, sq_val(w & 0xffu, mn, step));
            f(t + 1, sq_val((w >> 8) & 0xffu, mn, step));
            f(t + 2, sq_val((w >> 16) & 0xffu, mn, step));
            f(t + 3, sq_val(w >> 24, mn, step));
        }
    } else {
        for (uint32_t t = 0; t < d; ++t) f(t, sq_val(r[t], mn, step));
    }
}

// widest load the row loader may use: every row starts at base + i * d
inline int sq_load_width(const uint8_t *C, uint32_t d) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(C);
    if (d % 16 == 0 && a % 16 == 0) return 16;
    if (d % 4 == 0 && a % 4 == 0) return 4;
    return 1;
}

}  // namespace
}  // namespace vqhip
