// sq_decode.hpp -- the SQ decode rule in registers and the row source of resident SQ codes (knn_tile.hpp's kernels over
// every row in k_sqindex.hip, ivf_tile.hpp's over the probed lists in k_ivfsq.hip): v(c) = mn + (float)c * step for
// every byte value, two roundings, never fused.  A byte is decoded where it leaves global memory: v_cvt_f32_ubyteN takes
// byte N of a loaded dword straight to f32, then one multiply and one add.  Every including file gets its own copy (an
// anonymous namespace).
#pragma once
#include "common.hpp"
#include "knn_tile.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// the SQ decode rule for one byte: two roundings, never fused
__device__ __forceinline__ float sq_val(uint32_t byte, float mn, float step) {
    const float t = (float)byte * step;
    return mn + t;
}

struct SqScale {
    float mn, step;
};

// The row source of SQ codes X [n][d] u8 (knn_tile.hpp).  LW = bytes per load: 16 (d % 16 == 0 and a 16-byte aligned
// base), 4 (d % 4 == 0, 4-byte aligned) or 1.  A chunk of a row starts at byte row * d + t0 with t0 a multiple of 32, so
// those conditions align every load; a row's last chunk holds tc < 32 dimensions, a multiple of LW.  The walk of LW 16 is
// that of LW 4: dwords.
template <int LW>
struct SqRows {
    using Elem = uint8_t;
    using Walk = SqRows<(LW >= 4 ? 4 : 1)>;
    using Scale = SqScale;
    const uint8_t *X;
    uint32_t d;
    SqScale sc;

    __device__ __forceinline__ void fill(float (&rs)[kKnnKC][kKnnTR + 4], uint64_t row0, uint32_t nvalid, uint32_t t0,
                                         uint32_t tc) const {
        fill_rows(rs, [&](uint32_t r) { return row0 + r; }, nvalid, t0, tc);
    }
    __device__ __forceinline__ uint64_t row(uint64_t j) const { return j; }
    // tile row r read from row row_of(r) of X (asked only for r < nvalid): the one loader behind fill and PickedRows
    template <class RF>
    __device__ __forceinline__ void fill_rows(float (&rs)[kKnnKC][kKnnTR + 4], RF &&row_of, uint32_t nvalid, uint32_t t0,
                                              uint32_t tc) const {
        constexpr uint32_t TR = kKnnTR, KC = kKnnKC;
        const uint32_t tid = threadIdx.x;
        const float mn = sc.mn, step = sc.step;
        if constexpr (LW == 16) {  // 64 rows x two 16-byte halves: the first 128 lanes
            if (tid < TR * KC / 16) {
                const uint32_t r = tid >> 1, c0 = (tid & 1u) * 16;
                const bool ok = r < nvalid && c0 < tc;
                uint4 w = make_uint4(0, 0, 0, 0);
                if (ok) w = *reinterpret_cast<const uint4 *>(X + row_of(r) * d + t0 + c0);
                const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j)
                    rs[c0 + j][r] = ok ? sq_val((ws[j >> 2] >> (8 * (j & 3))) & 0xffu, mn, step) : 0.0f;
            }
        } else if constexpr (LW == 4) {  // 64 rows x eight dwords: two per lane
#pragma unroll
            for (uint32_t e = 0; e < TR * KC / 4 / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / (KC / 4), c0 = (idx % (KC / 4)) * 4;
                const bool ok = r < nvalid && c0 < tc;
                uint32_t w = 0;
                if (ok) w = *reinterpret_cast<const uint32_t *>(X + row_of(r) * d + t0 + c0);
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) rs[c0 + j][r] = ok ? sq_val((w >> (8 * j)) & 0xffu, mn, step) : 0.0f;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < TR * KC / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / KC, c1 = idx % KC;
                rs[c1][r] = (r < nvalid && c1 < tc) ? sq_val(X[row_of(r) * d + t0 + c1], mn, step) : 0.0f;
            }
        }
    }
    // (the load width is the type's: t0 and tc are multiples of 4 under LW >= 4)
    template <class F>
    __device__ __forceinline__ void walk(uint64_t row, uint32_t t0, uint32_t tc, bool, F &&f) const {
        const uint8_t *r = X + row * d + t0;
        const float mn = sc.mn, step = sc.step;
        if constexpr (LW >= 4) {
            for (uint32_t t = 0; t < tc; t += 4) {
                const uint32_t w = *reinterpret_cast<const uint32_t *>(r + t);
                f(t0 + t, sq_val(w & 0xffu, mn, step));
                f(t0 + t + 1, sq_val((w >> 8) & 0xffu, mn, step));
                f(t0 + t + 2, sq_val((w >> 16) & 0xffu, mn, step));
                f(t0 + t + 3, sq_val(w >> 24, mn, step));
            }
        } else {
            for (uint32_t t = 0; t < tc; ++t) f(t0 + t, sq_val(r[t], mn, step));
        }
    }
};

// f(the row source of C [.][d]) with the widest load the row loader may use: every row starts at C + i * d
template <class F>
int sq_rows(const uint8_t *C, uint32_t d, float mn, float step, F &&f) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(C);
    if (d % 16 == 0 && a % 16 == 0) return f(SqRows<16>{C, d, {mn, step}});
    if (d % 4 == 0 && a % 4 == 0) return f(SqRows<4>{C, d, {mn, step}});
    return f(SqRows<1>{C, d, {mn, step}});
}

}  // namespace
}  // namespace vqhip
