// vq_amd/csrc/nibble_decode.hpp under a host compiler: the nibble extraction against a loop, the decode rule, one lane's
// share of a chunk's fill (nib_fill_lane, the code the device runs) emulated lane by lane over the 256 lanes, the LDS
// banks of every wave store, and the word offsets on both sides of 2^31 and 2^32 bytes (arithmetic only).
// Driver: tests/test_cpp_nibble_decode.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nibble_decode.hpp"

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

// the decode of code c by two separately rounded operations (volatile: nothing may fuse or fold them)
static float decode_ref(uint32_t c, float mn, float step) {
    volatile float t = (float)c * step;
    volatile float v = mn + t;
    return v;
}

static void decode_rule() {
    std::mt19937 rng(7);
    for (int trial = 0; trial < 2000; ++trial) {
        const uint32_t word = trial == 0 ? 0u : trial == 1 ? 0xFFFFFFFFu : (uint32_t)rng();
        uint32_t rest = word;
        for (uint32_t t = 0; t < 8; ++t) {
            const uint32_t code = rest % 16u;  // the loop's own arithmetic: no shift-and-mask
            rest /= 16u;
            EXPECT(nib_code(word, t) == code);
            EXPECT(nib_code(word, t + 8) == code && nib_code(word, t + 1016) == code);  // dimension t of a later word
        }
    }
    EXPECT(nib_code(0x87654321u, 0) == 1 && nib_code(0x87654321u, 7) == 8 && nib_code(0xF0000000u, 7) == 15);
    const float scales[][2] = {{-1.0f, 2.0f / 15.0f}, {0.0f, 1.0f}, {-3.5f, 203.5f / 4.0f}, {0.0f, 1.0f}, {0.1f, 0.3f}};
    for (const auto &s : scales)
        for (uint32_t c = 0; c < 16; ++c) EXPECT(same_bits(nib_value(c, s[0], s[1]), decode_ref(c, s[0], s[1])));
    EXPECT(same_bits(nib_value(0, 0.0f, 1.0f), 0.0f) && same_bits(nib_value(0, -0.0f, 1.0f), 0.0f));  // -0.0 + +0.0 = +0.0
    EXPECT(nib_row_words(1) == 1 && nib_row_words(8) == 1 && nib_row_words(9) == 2 && nib_row_words(1024) == 128 &&
           nib_row_words(0xFFFFFFFFu) == 0x20000000u);
}

// the 256 lanes of one chunk: every (c, r) stored exactly once, a load only where the row is valid and the lane's word
// starts below tc, each word of a valid row loaded at most once, the decoded nibble inside [0, tc) x [0, nvalid) and
// +0.0f elsewhere (not mn)
static void fill_schedule() {
    std::mt19937 rng(11);
    const uint32_t tcs[] = {1, 7, 8, 9, 31, 32}, nvs[] = {1, 63, 64};
    const float mn = -3.5f, step = 50.875f;
    for (uint32_t tc : tcs)
        for (uint32_t nvalid : nvs) {
            uint32_t words[kNibTileRows][4];
            for (uint32_t r = 0; r < kNibTileRows; ++r)
                for (uint32_t w = 0; w < 4; ++w) words[r][w] = (uint32_t)rng();
            std::vector<int> stores(kNibChunk * kNibTileRows, 0), loads(kNibTileRows * 4, 0);
            std::vector<float> tile(kNibChunk * kNibTileRows, -7.0f);
            for (uint32_t tid = 0; tid < kNibLanes; ++tid) {
                int lane_loads = 0;
                nib_fill_lane(
                    tid, nvalid, tc, mn, step,
                    [&](uint32_t r, uint32_t wi) {
                        EXPECT(r < nvalid && r == tid % kNibTileRows);       // its own row, and a valid one
                        EXPECT(wi == tid / kNibTileRows && wi * 8 < tc);     // its own word, which starts inside the chunk
                        ++lane_loads;
                        ++loads[r * 4 + wi];
                        return words[r][wi];
                    },
                    [&](uint32_t c, uint32_t r, float v) {
                        EXPECT(c < kNibChunk && r < kNibTileRows);
                        EXPECT(r == tid % kNibTileRows && c / 8 == tid / kNibTileRows);
                        ++stores[c * kNibTileRows + r];
                        tile[c * kNibTileRows + r] = v;
                    });
                EXPECT(lane_loads <= 1);
            }
            for (uint32_t c = 0; c < kNibChunk; ++c)
                for (uint32_t r = 0; r < kNibTileRows; ++r) {
                    EXPECT(stores[c * kNibTileRows + r] == 1);
                    const uint32_t code = (words[r][c / 8] >> (4 * (c % 8))) & 15u;
                    const float want = (c < tc && r < nvalid) ? decode_ref(code, mn, step) : 0.0f;
                    EXPECT(same_bits(tile[c * kNibTileRows + r], want));
                }
            // word wi of a valid row is read once where it starts below tc; no other word, and no invalid row, ever
            for (uint32_t r = 0; r < kNibTileRows; ++r)
                for (uint32_t wi = 0; wi < 4; ++wi) EXPECT(loads[r * 4 + wi] == ((r < nvalid && wi * 8 < tc) ? 1 : 0));
        }
}

// the stores of one wave instruction: 64 consecutive rows of one dimension, so each 32-lane half meets 32 different banks
// of the 68-float LDS rows -- conflict degree 1
static void lds_banks() {
    for (uint32_t wave = 0; wave < kNibLanes / 64; ++wave)
        for (uint32_t j = 0; j < kNibWordDims; ++j)
            for (uint32_t half = 0; half < 2; ++half) {
                uint32_t hits[32] = {};
                for (uint32_t l = 0; l < 32; ++l) {
                    const uint32_t tid = wave * 64 + half * 32 + l;
                    uint32_t sc = 0, sr = 0, at = 0;
                    nib_fill_lane(
                        tid, 64, 32, 0.0f, 1.0f, [&](uint32_t, uint32_t) { return 0u; },
                        [&](uint32_t c, uint32_t r, float) {
                            if (at++ == j) sc = c, sr = r;  // the lane's j-th store
                        });
                    ++hits[(sc * (kNibTileRows + 4) + sr) % 32];
                }
                for (uint32_t b = 0; b < 32; ++b) EXPECT(hits[b] == 1);
            }
}

static void offsets() {
    // W = 128 (d = 1024): row 2^22 starts at byte 2^31, row 2^23 at byte 2^32
    const uint32_t W = 128;
    const uint64_t rows[] = {(1ull << 22) - 1, 1ull << 22, (1ull << 23) - 1, 1ull << 23, (1ull << 32) - 1};
    for (uint64_t row : rows)
        for (uint32_t t0 : {0u, 32u, 992u}) {
            const uint64_t off = nib_word_offset(row, W, t0);
            EXPECT(off == row * 128ull + t0 / 8);
            EXPECT(off * 4 / 4 == off);  // the byte offset fits 64 bits
        }
    EXPECT((nib_word_offset((1ull << 22) - 1, W, 992) + 3) * 4 == (1ull << 31) - 4);  // the chunk's fourth word
    EXPECT(nib_word_offset(1ull << 22, W, 0) * 4 == 1ull << 31);
    EXPECT((nib_word_offset((1ull << 23) - 1, W, 992) + 3) * 4 == (1ull << 32) - 4);
    EXPECT(nib_word_offset(1ull << 23, W, 0) * 4 == 1ull << 32);
    EXPECT(nib_word_offset((1ull << 32) - 1, W, 992) == ((1ull << 32) - 1) * 128 + 124);
    // W = 1 (d <= 8): only the row count passes 2^31 / 2^32 bytes
    EXPECT(nib_word_offset(1ull << 29, 1, 0) * 4 == 1ull << 31 && nib_word_offset(1ull << 30, 1, 0) * 4 == 1ull << 32);
    // W = 13 (d = 100), a stride that is no power of two
    EXPECT(nib_word_offset(330382100ull, 13, 96) == 330382100ull * 13 + 12 && 330382100ull * 13 * 4 > (1ull << 34));
    // the widest row: W = 2^29 words
    EXPECT(nib_word_offset(7, nib_row_words(0xFFFFFFFFu), 0xFFFFFFE0u) == 7ull * 0x20000000ull + 0x1FFFFFFCull);
}

int main() {
    decode_rule();
    fill_schedule();
    lds_banks();
    offsets();
    std::printf("NIBBLE_DECODE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
