// vq_amd/csrc/bit_decode.hpp under a host compiler: the 1-bit decode rule against a loop, one lane's share of a chunk's
// fill (bit_fill_lane, the code the device runs) emulated lane by lane over the 256 lanes, and the word offsets on both
// sides of 2^31 and 2^32 bytes (arithmetic only).  Driver: tests/test_cpp_bit_decode.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bit_decode.hpp"

using namespace vqhip;

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static bool same_bits(float a, float b) { return !std::memcmp(&a, &b, 4); }

static void decode_rule() {
    std::mt19937 rng(7);
    const float pairs[][2] = {{0.0f, 1.0f}, {3.0f, 200.0f}, {0.0f, 255.0f}, {-0.0f, 7.0f}};
    for (int trial = 0; trial < 2000; ++trial) {
        const uint32_t word = trial == 0 ? 0u : trial == 1 ? 0xFFFFFFFFu : (uint32_t)rng();
        const float lo = pairs[trial % 4][0], hi = pairs[trial % 4][1];
        for (uint32_t t = 0; t < 32; ++t) {
            const bool bit = (word / (1u << t)) % 2u == 1u;  // the loop's own arithmetic: no shift-and-mask
            EXPECT(same_bits(bit_value(word, t, lo, hi), bit ? hi : lo));
            EXPECT(same_bits(bit_value(word, t + 64, lo, hi), bit ? hi : lo));  // dimension t of a later word
        }
    }
    EXPECT(bit_row_words(1) == 1 && bit_row_words(32) == 1 && bit_row_words(33) == 2 && bit_row_words(8192) == 256);
}

// the 256 lanes of one chunk: every (c, r) stored exactly once, a load only where the row is valid and the lane's band
// starts below tc, the decoded bit inside [0, tc) x [0, nvalid) and +0.0f elsewhere
static void fill_schedule() {
    std::mt19937 rng(11);
    const uint32_t tcs[] = {1, 31, 32}, nvs[] = {1, 63, 64};
    const float lo = 3.0f, hi = 200.0f;
    for (uint32_t tc : tcs)
        for (uint32_t nvalid : nvs) {
            uint32_t words[kBitTileRows];
            for (uint32_t r = 0; r < kBitTileRows; ++r) words[r] = (uint32_t)rng() | (r == 0 ? 1u : 0u);
            std::vector<int> stores(kBitChunk * kBitTileRows, 0), loads(kBitTileRows, 0);
            std::vector<float> tile(kBitChunk * kBitTileRows, -7.0f);
            for (uint32_t tid = 0; tid < kBitLanes; ++tid) {
                int lane_loads = 0;
                bit_fill_lane(
                    tid, nvalid, tc, lo, hi,
                    [&](uint32_t r) {
                        EXPECT(r < nvalid && r == tid % kBitTileRows);  // its own row, and a valid one
                        EXPECT((tid / kBitTileRows) * kBitLaneDims < tc);  // its band starts inside the chunk
                        ++lane_loads;
                        ++loads[r];
                        return words[r];
                    },
                    [&](uint32_t c, uint32_t r, float v) {
                        EXPECT(c < kBitChunk && r < kBitTileRows);
                        ++stores[c * kBitTileRows + r];
                        tile[c * kBitTileRows + r] = v;
                    });
                EXPECT(lane_loads <= 1);
            }
            for (uint32_t c = 0; c < kBitChunk; ++c)
                for (uint32_t r = 0; r < kBitTileRows; ++r) {
                    EXPECT(stores[c * kBitTileRows + r] == 1);
                    const float want = (c < tc && r < nvalid) ? (((words[r] >> c) & 1u) ? hi : lo) : 0.0f;
                    EXPECT(same_bits(tile[c * kBitTileRows + r], want));
                }
            // a valid row's word is read once by each band that starts below tc, an invalid row's never
            const int bands = (int)((tc + kBitLaneDims - 1) / kBitLaneDims);
            for (uint32_t r = 0; r < kBitTileRows; ++r) EXPECT(loads[r] == (r < nvalid ? bands : 0));
        }
    // the stores of one wave instruction: 64 consecutive rows of one dimension, so each 32-lane half meets 32 banks of
    // the 68-float LDS rows
    for (uint32_t wave = 0; wave < kBitLanes / 64; ++wave)
        for (uint32_t j = 0; j < kBitLaneDims; ++j)
            for (uint32_t half = 0; half < 2; ++half) {
                uint32_t seen = 0;
                for (uint32_t l = 0; l < 32; ++l) {
                    const uint32_t tid = wave * 64 + half * 32 + l, r = tid % kBitTileRows, c = (tid / kBitTileRows) * kBitLaneDims + j;
                    seen |= 1u << ((c * (kBitTileRows + 4) + r) % 32);
                }
                EXPECT(seen == 0xFFFFFFFFu);
            }
}

static void offsets() {
    // W = 256 (d = 8192): row 2^21 starts at byte 2^31, row 2^22 at byte 2^32
    const uint32_t W = 256;
    const uint64_t rows[] = {(1ull << 21) - 1, 1ull << 21, (1ull << 22) - 1, 1ull << 22, (1ull << 32) - 1};
    for (uint64_t row : rows)
        for (uint32_t t0 : {0u, 32u, 8160u}) {
            const uint64_t off = bit_word_offset(row, W, t0);
            EXPECT(off == row * 256ull + t0 / 32);
            EXPECT(off * 4 / 4 == off);  // the byte offset fits 64 bits
        }
    EXPECT(bit_word_offset((1ull << 21) - 1, W, 8160) * 4 == (1ull << 31) - 4);
    EXPECT(bit_word_offset(1ull << 21, W, 0) * 4 == 1ull << 31);
    EXPECT(bit_word_offset((1ull << 22) - 1, W, 8160) * 4 == (1ull << 32) - 4);
    EXPECT(bit_word_offset(1ull << 22, W, 0) * 4 == 1ull << 32);
    EXPECT(bit_word_offset((1ull << 32) - 1, W, 8160) == ((1ull << 32) - 1) * 256 + 255);
    // W = 1 (d <= 32): only the row count passes 2^31 / 2^32 bytes
    EXPECT(bit_word_offset(1ull << 29, 1, 0) * 4 == 1ull << 31 && bit_word_offset(1ull << 30, 1, 0) * 4 == 1ull << 32);
    // W = 3 (d = 96), a stride that is no power of two
    EXPECT(bit_word_offset(715827883ull, 3, 64) == 715827883ull * 3 + 2 && 715827883ull * 3 * 4 > (1ull << 33));
}

int main() {
    decode_rule();
    fill_schedule();
    offsets();
    std::printf("BIT_DECODE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
