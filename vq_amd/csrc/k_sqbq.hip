// k_sqbq.hip -- ScalarQuantizer (src/sq.rs) and BinaryQuantizer (src/bq.rs): elementwise, HBM-streaming.
//
// Both maps are one pass over f32 <-> u8 with no reuse, so the kernels are shaped for the memory pipe: 16 elements per
// lane: an encode lane reads four float4 and writes one 16-byte word of codes, a decode lane reads four codes four
// times and writes four float4, each store instruction of a wave 1 KB contiguous (see k_sqbq_decode).  Pointers need only
// their element alignment: a scalar head brings the CODE pointer to 16 bytes; if the f32 side is then 16-aligned too
// the body runs vectorised, else every element goes the scalar way (correct, slower).  A scalar tail finishes.
//
// Exactness comes from tables the host builds with the reference's own arithmetic:
//  * SQ encode, finite step > 0: code(x) = min(sat(round((clamp(x) - min) / step)), levels - 1) is monotone
//    non-decreasing in x, so it is described by b[i] = the smallest f32 whose code is >= i (i = 1..levels-1), found by
//    bisection over ordered bit patterns (sq_thresholds).  The device estimates rint((x - min) * (1/step)) -- within
//    one code of the truth -- and corrects it by one comparison each way against b[] in LDS.  NaN -> 0.
//  * SQ encode, step = inf / 0 (or 1/step overflows): the direct form, IEEE '/' (-fhip-fp32-correctly-rounded-divide-
//    sqrt), roundf (half away from zero) and an explicit saturating cast (a C++ cast of NaN / inf is undefined).
//  * SQ decode and BQ decode: a 256-entry f32 table of the reference's formula per code byte.
//  * BQ encode: a compare and a select.
#include "kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace vqhip {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint32_t sat_code(float r, uint32_t top) {  // `r as usize` then .min(top); NaN -> 0
    return r >= 0.0f ? (r < (float)top ? (uint32_t)r : top) : 0u;
}

template <int MODE>
__device__ __forceinline__ uint32_t encode_one(const SqbqEncodeOp &p, const float *tb, float x) {
    if constexpr (MODE == SQBQ_BINARY) {
        return x >= p.thr ? p.high : p.low;
    } else if constexpr (MODE == SQBQ_DIRECT) {
        float c = x < p.mn ? p.mn : x;  // f32::clamp: a NaN stays NaN
        c = c > p.mx ? p.mx : c;
        return sat_code(roundf((c - p.mn) / p.step), p.top);
    } else {
        uint32_t e = sat_code(rintf((x - p.mn) * p.inv), p.top);  // NaN -> 0, and b[] keeps it there
        e -= x < tb[e] ? 1u : 0u;                                  // tb[0] = -inf
        e += x >= tb[e + 1] ? 1u : 0u;                             // tb[top + 1] = NaN
        return e;
    }
}

// count elements x -> codes; `head` scalar elements, then `groups` runs of 16 from x + head / codes + head (both
// 16-byte aligned: four float4 loads and one 16-byte store per lane), then the scalar rest
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_sqbq_encode(SqbqEncodeOp p, const float *__restrict__ x, uint64_t count,
                                                        uint8_t *__restrict__ codes, uint64_t head, uint64_t groups) {
    __shared__ float tb[kSqTable];
    if constexpr (MODE == SQBQ_TABLE) {
        for (uint32_t i = threadIdx.x; i < kSqTable; i += kBlock) tb[i] = p.b[i];
        __syncthreads();
    }
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
        const float4 *src = reinterpret_cast<const float4 *>(x + head + g * 16);
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = src[q];
        uint4 w;
        uint32_t *wp = &w.x;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            wp[q] = encode_one<MODE>(p, tb, v[q].x) | (encode_one<MODE>(p, tb, v[q].y) << 8) |
                    (encode_one<MODE>(p, tb, v[q].z) << 16) | (encode_one<MODE>(p, tb, v[q].w) << 24);
        *reinterpret_cast<uint4 *>(codes + head + g * 16) = w;
    }
    const uint64_t body_end = head + groups * 16, scalar = head + (count - body_end);
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < scalar; j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t e = j < head ? j : body_end + (j - head);
        codes[e] = (uint8_t)encode_one<MODE>(p, tb, x[e]);
    }
}

// count codes -> out through lut[256] (SQ: min + c * step; BQ: c >= high ? high : low).  After the `head` scalar
// elements, each wave converts runs of kRun = 1024: its q-th store instruction writes elements [256 q, 256 q + 256) of
// the run -- 16 contiguous bytes per lane, 1 KB per wave-instruction -- from the four codes the lane loaded for them
// by one dword load (256 contiguous bytes per wave-instruction).  (Sixteen elements per lane from one 16-byte load put
// each store instruction's 16-byte pieces 64 bytes apart: 3.7 TB/s against 5.x at 1M x 384.)  Then the scalar rest.
constexpr uint64_t kRun = 1024;
__global__ __launch_bounds__(kBlock) void k_sqbq_decode(SqbqDecodeLut p, const uint8_t *__restrict__ codes, uint64_t count,
                                                        float *__restrict__ out, uint64_t head, uint64_t runs) {
    __shared__ float lut[256];
    lut[threadIdx.x] = p.lut[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
    for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < runs; r += waves) {
        const uint8_t *c = codes + head + r * kRun + lane * 4;
        float *o = out + head + r * kRun + lane * 4;
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = *reinterpret_cast<const uint32_t *>(c + q * 256);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4 *>(o + q * 256) =
                make_float4(lut[w[q] & 0xffu], lut[(w[q] >> 8) & 0xffu], lut[(w[q] >> 16) & 0xffu], lut[w[q] >> 24]);
    }
    const uint64_t body_end = head + runs * kRun, scalar = head + (count - body_end);
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < scalar; j += (uint64_t)gridDim.x * kBlock) {
        const uint64_t e = j < head ? j : body_end + (j - head);
        out[e] = lut[codes[e]];
    }
}

// split [0, count) into a scalar head that 16-aligns the byte side, runs of `unit` elements, and the rest; no runs when
// the f32 side is then not 16-aligned as well (everything scalar)
void split16(const void *f32_side, const void *byte_side, uint64_t count, uint64_t unit, uint64_t *head, uint64_t *runs) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(byte_side);
    uint64_t h = (16 - (b & 15)) & 15;
    if (h > count) h = count;
    const bool ok = ((reinterpret_cast<uintptr_t>(f32_side) + 4 * h) & 15) == 0;
    *head = ok ? h : count;
    *runs = ok ? (count - h) / unit : 0;
}

// enough workgroups for `items` body items of `per_block` each and for the scalar elements (one per lane)
uint32_t sqbq_grid(uint64_t items, uint64_t per_block, uint64_t scalar) {
    uint64_t b = std::max((items + per_block - 1) / per_block, (scalar + kBlock - 1) / kBlock);
    if (b > (1ull << 30)) b = 1ull << 30;
    return (uint32_t)std::max<uint64_t>(b, 1);
}

template <int MODE>
int launch_encode_mode(const SqbqEncodeOp &p, const float *x, uint64_t count, uint8_t *codes, uint64_t head,
                       uint64_t groups, hipStream_t stream) {
    const uint32_t grid = sqbq_grid(groups, kBlock, count - groups * 16);
    hipLaunchKernelGGL(k_sqbq_encode<MODE>, dim3(grid), dim3(kBlock), 0, stream, p, x, count, codes, head, groups);
    VQ_LAUNCH_CHECK("k_sqbq_encode");
    return VQHIP_OK;
}

// ---- the reference's arithmetic on the host (built with -ffp-contract=off: no fused multiply-add; SSE f32 division
// and subnormals as on the reference's CPU) ----
uint32_t sq_code_host(float mn, float mx, float step, uint32_t top, float x) {
    float c = x;  // f32::clamp (src/sq.rs quantize_scalar): NaN passes through
    if (c < mn) c = mn;
    if (c > mx) c = mx;
    const float r = std::round((c - mn) / step);
    if (!(r >= 0.0f)) return 0;  // NaN -> 0 (`as usize` saturates)
    if (r >= (float)top) return top;
    return (uint32_t)r;
}

// total order over non-NaN f32 bit patterns: -inf < ... < -0 < +0 < ... < +inf
uint32_t f32_key(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float key_f32(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

}  // namespace

int sq_check(float mn, float mx, uint32_t levels, float *step) {
    // src/sq.rs ScalarQuantizer::new: the order and the texts of its checks
    if (!std::isfinite(mn)) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'min': must be finite (not NaN or infinite)");
    if (!std::isfinite(mx)) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'max': must be finite (not NaN or infinite)");
    if (mx <= mn) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'max': must be greater than min");
    if (levels < 2) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'levels': must be at least 2");
    if (levels > 256) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'levels': must be no more than 256 to fit in u8");
    if (step) *step = (mx - mn) / (float)(levels - 1);
    return VQHIP_OK;
}

int bq_check(float threshold, uint32_t low, uint32_t high) {
    // src/bq.rs BinaryQuantizer::new; low / high are u8 there (the Python and C++ layers refuse wider values first)
    if (!std::isfinite(threshold)) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'threshold': must be finite (not NaN or infinite)");
    if (low > 255) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'low': must fit in u8");
    if (high > 255) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'high': must fit in u8");
    if (low >= high) return fail(VQHIP_ERR_INVALID_INPUT, "Invalid parameter 'low/high': low must be less than high");
    return VQHIP_OK;
}

void sq_thresholds(float mn, float mx, uint32_t levels, float step, float *b) {
    const uint32_t top = levels - 1;
    const uint32_t k_lo = f32_key(-INFINITY), k_hi = f32_key(INFINITY);
    b[0] = -INFINITY;
    for (uint32_t i = 1; i < levels; ++i) {
        if (sq_code_host(mn, mx, step, top, INFINITY) < i) {  // no input reaches code i (step = inf)
            b[i] = NAN;
            continue;
        }
        uint32_t lo = k_lo, hi = k_hi;  // smallest key whose code is >= i
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (sq_code_host(mn, mx, step, top, key_f32(mid)) >= i) hi = mid;
            else lo = mid + 1;
        }
        b[i] = key_f32(lo);
    }
}

int sq_encode_op(float mn, float mx, uint32_t levels, SqbqEncodeOp *p) {
    float step = 0;
    VQ_TRY(sq_check(mn, mx, levels, &step));
    // the bisection costs ~8k host divisions (tens of us): a per-vector caller repeats the same quantizer, so the last
    // table of each thread is kept, keyed by the parameters' bits
    thread_local struct {
        bool valid = false;
        uint32_t mn = 0, mx = 0, levels = 0;
        SqbqEncodeOp op;
    } last;
    uint32_t mn_bits, mx_bits;
    memcpy(&mn_bits, &mn, 4);
    memcpy(&mx_bits, &mx, 4);
    if (last.valid && last.mn == mn_bits && last.mx == mx_bits && last.levels == levels) {
        *p = last.op;
        return VQHIP_OK;
    }
    *p = SqbqEncodeOp{};
    p->mn = mn, p->mx = mx, p->step = step, p->top = levels - 1;
    p->inv = 1.0f / step;
    const bool table = std::isfinite(step) && step > 0.0f && std::isfinite(p->inv);
    p->mode = table ? SQBQ_TABLE : SQBQ_DIRECT;
    if (table) {
        sq_thresholds(mn, mx, levels, step, p->b);
        p->b[levels] = NAN;  // x >= NaN never holds: the estimate never steps past the top code
    }
    last.op = *p;
    last.mn = mn_bits, last.mx = mx_bits, last.levels = levels, last.valid = true;
    return VQHIP_OK;
}

int bq_encode_op(float threshold, uint32_t low, uint32_t high, SqbqEncodeOp *p) {
    VQ_TRY(bq_check(threshold, low, high));
    *p = SqbqEncodeOp{};
    p->mode = SQBQ_BINARY;
    p->thr = threshold, p->low = low, p->high = high;
    return VQHIP_OK;
}

int sq_decode_lut(float mn, float mx, uint32_t levels, SqbqDecodeLut *p) {
    float step = 0;
    VQ_TRY(sq_check(mn, mx, levels, &step));
    for (uint32_t c = 0; c < 256; ++c) {  // `self.min + idx as f32 * self.step`, every byte (codes >= levels too)
        const float t = (float)c * step;
        p->lut[c] = mn + t;
    }
    return VQHIP_OK;
}

int bq_decode_lut(float threshold, uint32_t low, uint32_t high, SqbqDecodeLut *p) {
    VQ_TRY(bq_check(threshold, low, high));
    for (uint32_t c = 0; c < 256; ++c) p->lut[c] = c >= high ? (float)high : (float)low;
    return VQHIP_OK;
}

int launch_sqbq_encode(const SqbqEncodeOp &p, const float *x, uint64_t count, uint8_t *codes, hipStream_t stream) {
    if (count == 0) return VQHIP_OK;
    uint64_t head, groups;
    split16(x, codes, count, 16, &head, &groups);
    switch (p.mode) {
        case SQBQ_TABLE: return launch_encode_mode<SQBQ_TABLE>(p, x, count, codes, head, groups, stream);
        case SQBQ_DIRECT: return launch_encode_mode<SQBQ_DIRECT>(p, x, count, codes, head, groups, stream);
        default: return launch_encode_mode<SQBQ_BINARY>(p, x, count, codes, head, groups, stream);
    }
}

int launch_sqbq_decode(const SqbqDecodeLut &p, const uint8_t *codes, uint64_t count, float *out, hipStream_t stream) {
    if (count == 0) return VQHIP_OK;
    uint64_t head, runs;
    split16(out, codes, count, kRun, &head, &runs);
    const uint32_t grid = sqbq_grid(runs, kBlock / 64, count - runs * kRun);
    hipLaunchKernelGGL(k_sqbq_decode, dim3(grid), dim3(kBlock), 0, stream, p, codes, count, out, head, runs);
    VQ_LAUNCH_CHECK("k_sqbq_decode");
    return VQHIP_OK;
}

}  // namespace vqhip
