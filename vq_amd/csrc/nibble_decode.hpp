// nibble_decode.hpp -- the 4-bit decode and the row source of packed 4-bit SQ rows for the exact-distance kernels
// (knn_tile.hpp's, instantiated in k_sq4index.hip): v(c) = mn + (float)c * step, the rule of sq_val (sq_decode.hpp), two
// roundings, never fused, for every nibble value 0 .. 15.  The layout: dimension t of row i is bits 4 (t % 8) .. + 3 of
// u32 word i * W + t / 8, W = ceil(d / 8), pad nibbles zero; rows are word-aligned.  The tile's LDS chunk is 32
// dimensions (kKnnKC) and starts at a multiple of 32, so a chunk of a row is exactly four consecutive words.
// The code extraction, the word offsets and one lane's share of a chunk's fill are host and device code with no HIP in
// it when a host compiler reads it, so that they are tested on the CPU (tests/cpp/test_nibble_decode_hpp.cpp); the row
// source itself follows under hipcc.  Every including file gets its own copy (an anonymous namespace).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VQ_NIB_HD __host__ __device__ inline
#else
#define VQ_NIB_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vqhip {

constexpr uint32_t kNibTileRows = 64;   // rows of a tile (kKnnTR)
constexpr uint32_t kNibChunk = 32;      // dimensions of a chunk (kKnnKC): four packed words per row
constexpr uint32_t kNibLanes = 256;     // lanes that fill a chunk
constexpr uint32_t kNibWordDims = 8;    // dimensions of a word, and LDS writes per lane and chunk

// the code of dimension t of a row whose word t / 8 is `word`
VQ_NIB_HD uint32_t nib_code(uint32_t word, uint32_t t) { return (word >> (4u * (t & 7u))) & 15u; }

// the decode rule for one code: a multiply and an add, two roundings
VQ_NIB_HD float nib_value(uint32_t code, float mn, float step) {
    const float t = (float)code * step;
    return mn + t;
}

// words of a row of d dimensions (any d: d + 7 would wrap above 2^32 - 8)
VQ_NIB_HD uint32_t nib_row_words(uint32_t d) { return d / 8u + (d % 8u != 0u ? 1u : 0u); }

// the first of the four words of X that hold dimensions t0 .. t0 + 31 of `row` (t0 a multiple of 32), in words; 64-bit:
// n * W * 4 bytes passes 2^32
VQ_NIB_HD uint64_t nib_word_offset(uint64_t row, uint32_t W, uint32_t t0) { return row * (uint64_t)W + (t0 >> 3); }

// One lane's share of a chunk's fill.  Lane tid of 256 owns tile row tid % 64 and word tid / 64 of the chunk, the eight
// dimensions (tid / 64) * 8 .. + 7: a wave is the 64 rows of one word.  It reads that word once -- load(r, word of the
// chunk), and only where the row is below nvalid and the word's first dimension below tc -- and calls store(c, r, value)
// for its eight positions: the decoded nibble where c < tc and r < nvalid, 0.0f elsewhere.  Every (c, r) of the chunk is
// stored exactly once by the 256 lanes and no word is loaded twice.  A store of one wave instruction goes to 64
// consecutive floats of one LDS row, so each 32-lane half meets 32 different banks: no bank conflict.
template <class LOAD, class STORE>
VQ_NIB_HD void nib_fill_lane(uint32_t tid, uint32_t nvalid, uint32_t tc, float mn, float step, LOAD &&load, STORE &&store) {
    const uint32_t r = tid % kNibTileRows, wi = tid / kNibTileRows, c0 = wi * kNibWordDims;
    const bool ok = r < nvalid && c0 < tc;
    const uint32_t word = ok ? load(r, wi) : 0u;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < kNibWordDims; ++j) {
        const uint32_t c = c0 + j;
        store(c, r, (ok && c < tc) ? nib_value(nib_code(word, j), mn, step) : 0.0f);
    }
}

}  // namespace vqhip

#if defined(__HIPCC__)
#include "common.hpp"
#include "knn_tile.hpp"

namespace vqhip {
namespace {

static_assert(kNibTileRows == kKnnTR && kNibChunk == kKnnKC && kNibLanes == 256 &&
                  kNibTileRows * kNibChunk == kNibLanes * kNibWordDims,
              "the nibble row source is written for the 64 x 32 tile chunk and 256 lanes");

struct NibbleScale {
    float mn, step;  // the ScalarQuantizer's min and step
};

// The row source of packed rows X [n][W] u32 (knn_tile.hpp).  The kernels hand it {X, d, sc}; the row stride is W words,
// which it derives from d.
struct NibbleRows {
    using Elem = uint32_t;
    using Walk = NibbleRows;
    using Scale = NibbleScale;
    const uint32_t *X;
    uint32_t d;
    NibbleScale sc;

    __device__ __forceinline__ void fill(float (&rs)[kKnnKC][kKnnTR + 4], uint64_t row0, uint32_t nvalid, uint32_t t0,
                                         uint32_t tc) const {
        fill_rows(rs, [&](uint32_t r) { return row0 + r; }, nvalid, t0, tc);
    }
    __device__ __forceinline__ uint64_t row(uint64_t j) const { return j; }
    // tile row r read from row row_of(r) of X (asked only for r < nvalid): the one loader behind fill
    template <class RF>
    __device__ __forceinline__ void fill_rows(float (&rs)[kKnnKC][kKnnTR + 4], RF &&row_of, uint32_t nvalid, uint32_t t0,
                                              uint32_t tc) const {
        const uint32_t W = nib_row_words(d);
        nib_fill_lane(threadIdx.x, nvalid, tc, sc.mn, sc.step,
                      [&](uint32_t r, uint32_t wi) { return X[nib_word_offset((uint64_t)row_of(r), W, t0) + wi]; },
                      [&](uint32_t c, uint32_t r, float v) { rs[c][r] = v; });
    }
    // one word per eight dimensions (t0 a multiple of 8, as every caller's is)
    template <class F>
    __device__ __forceinline__ void walk(uint64_t row, uint32_t t0, uint32_t tc, bool, F &&f) const {
        const uint32_t *w = X + nib_word_offset(row, nib_row_words(d), t0);
        const float mn = sc.mn, step = sc.step;
        for (uint32_t t = 0; t < tc; t += 8) {
            const uint32_t word = w[t >> 3], m = min(8u, tc - t);
            for (uint32_t j = 0; j < m; ++j) f(t0 + t + j, nib_value(nib_code(word, j), mn, step));
        }
    }
};

}  // namespace
}  // namespace vqhip
#endif
