// The arithmetic of a removal from an inverted file (vq_amd/csrc/ivf_remove.hpp), built with g++ alone: below(i) against
// a loop; the schedule of k_ivf_take emulated workgroup by workgroup, pass by pass and lane by lane against the obvious
// gather, every destination byte written once; its byte offsets on both sides of 2^31 and 2^32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ivf_remove.hpp"

using namespace vqhip;

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// one mask over n rows: the prefix, the count, and below / new id of every row against a loop
static void check_below(uint64_t n, std::vector<uint32_t> words) {
    const uint64_t nw = (n + 31) / 32;
    EXPECT(words.size() == nw);
    std::vector<uint32_t> prefix(nw, 0xDEADu);
    const uint64_t gone = ivf_below_prefix(words.data(), n, prefix.data());
    uint32_t below = 0;  // removed rows under i
    for (uint64_t i = 0; i < n; ++i) {
        const bool removed = (words[i >> 5] >> (i & 31)) & 1u;
        if ((i & 31) == 0) EXPECT(prefix[i >> 5] == below);
        EXPECT(ivf_below(prefix[i >> 5], words[i >> 5], (uint32_t)i) == below);
        if (!removed) EXPECT(ivf_new_id(prefix[i >> 5], words[i >> 5], (uint32_t)i) == (uint32_t)i - below);
        below += removed;
    }
    EXPECT(gone == below);  // (bits at or past n are not counted)
}

static void below_cases() {
    for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 64ull, 1501ull}) {
        const uint64_t nw = (n + 31) / 32;
        check_below(n, std::vector<uint32_t>(nw, 0u));           // all clear
        check_below(n, std::vector<uint32_t>(nw, 0xFFFFFFFFu));  // all set, the pad bits of the last word too
        for (uint64_t one : {(uint64_t)0, n / 2, n - 1}) {       // one bit
            std::vector<uint32_t> w(nw, 0u);
            w[one >> 5] |= 1u << (one & 31);
            check_below(n, w);
        }
        for (int rep = 0; rep < 8; ++rep) {  // random, at three densities, pad bits random
            std::vector<uint32_t> w(nw);
            for (auto &x : w) x = rep % 3 == 0 ? rnd() : rep % 3 == 1 ? (rnd() & rnd() & rnd()) : (rnd() | rnd() | rnd());
            check_below(n, w);
        }
    }
}

// k_ivf_take's schedule over a source of n rows at byte `src_base` of its buffer and a destination at `dst_base`
static void take_case(uint64_t rb, uint64_t src_base, uint64_t dst_base, uint32_t want_unit) {
    const uint32_t n = 300;
    std::vector<uint32_t> pick;  // ascending positions: runs and gaps
    for (uint32_t g = 0; g < n; ++g)
        if (g < 3 || (g >= 64 && g < 130) || rnd() % 3 == 0 || g == n - 1) pick.push_back(g);
    const uint64_t na = pick.size();
    const uint32_t unit = compact_unit(rb, src_base, dst_base);
    EXPECT(unit == want_unit);
    std::vector<uint8_t> src(src_base + n * rb), dst(dst_base + na * rb, 0), hits(dst_base + na * rb, 0);
    for (auto &b : src) b = (uint8_t)rnd();
    const uint64_t upr = compact_units_per_row(rb, unit), units = na * upr;
    EXPECT(upr * unit == rb);
    const uint64_t blocks = ivf_take_blocks(units);
    EXPECT(blocks * kIvfTakeBlock >= units && (blocks == 0 || (blocks - 1) * kIvfTakeBlock < units));
    for (uint64_t blk = 0; blk < blocks; ++blk)
        for (uint32_t s = 0; s < kIvfTakePasses; ++s) {
            uint64_t prev = 0;
            for (uint32_t tid = 0; tid < kIvfTakeThreads; ++tid) {
                const uint64_t u = ivf_take_unit(blk, s, tid);
                if (tid) EXPECT(u == prev + 1);  // a wave's store is contiguous
                prev = u;
                if (u >= units) continue;
                uint32_t j;
                uint64_t within;
                ivf_take_row(u, upr, &j, &within);
                EXPECT(j < na && within < upr);
                const uint64_t so = src_base + ivf_take_src_offset(pick[j], rb, within, unit);
                const uint64_t to = dst_base + ivf_take_dst_offset(u, unit);
                EXPECT(so % unit == 0 && to % unit == 0);  // (the bases are aligned to the unit)
                EXPECT(so + unit <= src.size() && to + unit <= dst.size());
                for (uint32_t b = 0; b < unit; ++b) {
                    dst[to + b] = src[so + b];
                    ++hits[to + b];
                }
            }
        }
    for (uint64_t j = 0; j < na; ++j)
        EXPECT(std::memcmp(dst.data() + dst_base + j * rb, src.data() + src_base + (uint64_t)pick[j] * rb, rb) == 0);
    for (uint64_t b = 0; b < hits.size(); ++b) EXPECT(hits[b] == (b >= dst_base ? 1 : 0));
}

static void take_cases() {
    for (uint64_t rb : {1ull, 2ull, 6ull, 21ull, 42ull, 84ull, 128ull, 512ull}) {
        const uint32_t aligned = rb % 16 == 0 ? 16u : rb % 4 == 0 ? 4u : 1u;
        take_case(rb, 0, 0, aligned);
        take_case(rb, 256, 4096, aligned);
        take_case(rb, 16, 4, aligned == 16 ? 4u : aligned);  // a base that is a multiple of 4 only
        take_case(rb, 3, 0, 1u);                             // unaligned bases: bytes
        take_case(rb, 0, 1, 1u);
    }
}

static void offset_cases() {
    // source: row * rb + within * unit, 64-bit
    EXPECT(ivf_take_src_offset((1ull << 22) - 1, 512, 31, 16) == (1ull << 31) - 16);
    EXPECT(ivf_take_src_offset(1ull << 22, 512, 0, 16) == 1ull << 31);
    EXPECT(ivf_take_src_offset((1ull << 23) - 1, 512, 31, 16) == (1ull << 32) - 16);
    EXPECT(ivf_take_src_offset(1ull << 23, 512, 1, 16) == (1ull << 32) + 16);
    EXPECT(ivf_take_src_offset(0xFFFFFFFEull, 84, 20, 4) == 0xFFFFFFFEull * 84 + 80);
    EXPECT(ivf_take_src_offset(0xFFFFFFFEull, 21, 20, 1) == 0xFFFFFFFEull * 21 + 20);
    // destination: u * unit
    EXPECT(ivf_take_dst_offset((1ull << 27) - 1, 16) == (1ull << 31) - 16 && ivf_take_dst_offset(1ull << 27, 16) == 1ull << 31);
    EXPECT(ivf_take_dst_offset((1ull << 28) - 1, 16) == (1ull << 32) - 16 && ivf_take_dst_offset(1ull << 28, 16) == 1ull << 32);
    EXPECT(ivf_take_dst_offset((1ull << 30) + 5, 4) == (1ull << 32) + 20);
    EXPECT(ivf_take_dst_offset((1ull << 32) + 7, 1) == (1ull << 32) + 7);
    // a unit's row and place on both sides of 2^32 units (the 32-bit and the 64-bit division)
    uint32_t j;
    uint64_t within;
    ivf_take_row(0xFFFFFFFFull, 21, &j, &within);
    EXPECT(j == 0xFFFFFFFFull / 21 && within == 0xFFFFFFFFull % 21);
    ivf_take_row(1ull << 32, 21, &j, &within);
    EXPECT(j == (1ull << 32) / 21 && within == (1ull << 32) % 21);
    ivf_take_row((1ull << 32) * 21 - 1, 21, &j, &within);  // the last unit of row 2^32 - 1
    EXPECT(j == 0xFFFFFFFFu && within == 20);
    ivf_take_row(12345ull * 32 + 31, 32, &j, &within);
    EXPECT(j == 12345 && within == 31);
    // units of a workgroup past 2^32
    EXPECT(ivf_take_unit(1ull << 22, 0, 0) == 1ull << 32 && ivf_take_unit((1ull << 22) - 1, 3, 255) == (1ull << 32) - 1);
    EXPECT(ivf_take_blocks(0) == 0 && ivf_take_blocks(1) == 1 && ivf_take_blocks(1024) == 1 && ivf_take_blocks(1025) == 2);
    EXPECT(ivf_take_blocks((1ull << 32) + 1) == (1ull << 22) + 1);
}

int main() {
    below_cases();
    take_cases();
    offset_cases();
    std::printf("IVF_REMOVE_%s\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
