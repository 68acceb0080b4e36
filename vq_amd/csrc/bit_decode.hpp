// bit_decode.hpp -- the 1-bit decode rule and the row source of packed BQ rows for the exact-distance kernels
// (knn_tile.hpp's, instantiated in k_abin.hip): v(bit) = bit ? (float)high : (float)low, so an f32 query meets the
// dequantized row and never the row's own bits.  The layout is the binary index's: dimension t of row i is bit t % 32
// of u32 word i * W + t / 32, W = ceil(d / 32), pad bits zero.  The tile's LDS chunk is 32 dimensions (kKnnKC) and
// starts at a multiple of 32, so a chunk of a row is exactly one word.
// The decode, the word offsets and one lane's share of a chunk's fill are host and device code with no HIP in it when a
// host compiler reads it, so that they are tested on the CPU (tests/cpp/test_bit_decode_hpp.cpp); the row source itself
// follows under hipcc.  Every including file gets its own copy (an anonymous namespace).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VQ_BIT_HD __host__ __device__ inline
#else
#define VQ_BIT_HD inline
#endif

namespace vqhip {

constexpr uint32_t kBitTileRows = 64;   // rows of a tile (kKnnTR)
constexpr uint32_t kBitChunk = 32;      // dimensions of a chunk (kKnnKC): one packed word per row
constexpr uint32_t kBitLanes = 256;     // lanes that fill a chunk
constexpr uint32_t kBitLaneDims = kBitTileRows * kBitChunk / kBitLanes;  // LDS writes per lane and chunk: 8

// the decode rule: dimension t of a row whose word t / 32 is `word`
VQ_BIT_HD float bit_value(uint32_t word, uint32_t t, float lo, float hi) { return ((word >> (t & 31u)) & 1u) ? hi : lo; }

// words of a row of d dimensions
VQ_BIT_HD uint32_t bit_row_words(uint32_t d) { return (d + 31u) / 32u; }

// the word of X that holds dimensions t0 .. t0 + 31 of `row` (t0 a multiple of 32), in words; 64-bit: n * W passes 2^32
VQ_BIT_HD uint64_t bit_word_offset(uint64_t row, uint32_t W, uint32_t t0) { return row * (uint64_t)W + (t0 >> 5); }

// One lane's share of a chunk's fill.  Lane tid of 256 owns tile row tid % 64 and the eight dimensions (tid / 64) * 8 ..
// + 7 of the chunk: a wave is the 64 rows of one band of eight dimensions.  It reads its row's word once -- load(r), and
// only where the row is below nvalid and the band's first dimension below tc -- and calls store(c, r, value) for its
// eight positions: the decoded bit where c < tc and r < nvalid, 0.0f elsewhere.  Every (c, r) of the chunk is stored
// exactly once by the 256 lanes.  A store of one wave instruction goes to 64 consecutive floats of one LDS row, so each
// 32-lane half meets 32 different banks: no bank conflict.
template <class LOAD, class STORE>
VQ_BIT_HD void bit_fill_lane(uint32_t tid, uint32_t nvalid, uint32_t tc, float lo, float hi, LOAD &&load, STORE &&store) {
    const uint32_t r = tid % kBitTileRows, c0 = (tid / kBitTileRows) * kBitLaneDims;
    const bool ok = r < nvalid && c0 < tc;
    const uint32_t word = ok ? load(r) : 0u;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < kBitLaneDims; ++j) {
        const uint32_t c = c0 + j;
        store(c, r, (ok && c < tc) ? bit_value(word, c, lo, hi) : 0.0f);
    }
}

}  // namespace vqhip

#if defined(__HIPCC__)
#include "common.hpp"
#include "knn_tile.hpp"

namespace vqhip {
namespace {

static_assert(kBitTileRows == kKnnTR && kBitChunk == kKnnKC, "the bit row source is written for the 64 x 32 tile chunk");

struct BitScale {
    float lo, hi;  // (float)low, (float)high of the BinaryQuantizer
};

// The row source of packed rows X [n][W] u32 (knn_tile.hpp).  The kernels hand it {X, d, sc}; the row stride is W words,
// which it derives from d.
struct BitRows {
    using Elem = uint32_t;
    using Walk = BitRows;
    using Scale = BitScale;
    const uint32_t *X;
    uint32_t d;
    BitScale sc;

    __device__ __forceinline__ void fill(float (&rs)[kKnnKC][kKnnTR + 4], uint64_t row0, uint32_t nvalid, uint32_t t0,
                                         uint32_t tc) const {
        fill_rows(rs, [&](uint32_t r) { return row0 + r; }, nvalid, t0, tc);
    }
    __device__ __forceinline__ uint64_t row(uint64_t j) const { return j; }
    // tile row r read from row row_of(r) of X (asked only for r < nvalid): the one loader behind fill
    template <class RF>
    __device__ __forceinline__ void fill_rows(float (&rs)[kKnnKC][kKnnTR + 4], RF &&row_of, uint32_t nvalid, uint32_t t0,
                                              uint32_t tc) const {
        const uint32_t W = bit_row_words(d);
        bit_fill_lane(threadIdx.x, nvalid, tc, sc.lo, sc.hi,
                      [&](uint32_t r) { return X[bit_word_offset((uint64_t)row_of(r), W, t0)]; },
                      [&](uint32_t c, uint32_t r, float v) { rs[c][r] = v; });
    }
    // one word per 32 dimensions (t0 a multiple of 32, as every caller's is)
    template <class F>
    __device__ __forceinline__ void walk(uint64_t row, uint32_t t0, uint32_t tc, bool, F &&f) const {
        const uint32_t *w = X + bit_word_offset(row, bit_row_words(d), t0);
        const float lo = sc.lo, hi = sc.hi;
        for (uint32_t t = 0; t < tc; t += 32) {
            const uint32_t word = w[t >> 5], m = min(32u, tc - t);
            for (uint32_t j = 0; j < m; ++j) f(t0 + t + j, bit_value(word, j, lo, hi));
        }
    }
};

}  // namespace
}  // namespace vqhip
#endif
