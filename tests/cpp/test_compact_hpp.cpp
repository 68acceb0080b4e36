// The arithmetic of the row compaction (vq_amd/csrc/compact.hpp) on the CPU: the unit choice, the k-th clear bit against
// a loop, the unit -> row mapping and the byte offsets on both sides of 2^31 and 2^32 bytes, and the whole schedule of
// k_compact.hip -- count, scan, move, a wave's 64 lanes as a loop -- against the obvious compaction.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "compact.hpp"

using namespace vqhip;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

static uint32_t kth_clear_loop(uint32_t lo, uint32_t hi, uint32_t k) {
    const uint64_t removed = (uint64_t)lo | ((uint64_t)hi << 32);
    for (uint32_t p = 0; p < 64; ++p)
        if (!((removed >> p) & 1ull) && k-- == 0) return p;
    return 64;
}

static void check_kth(uint32_t lo, uint32_t hi) {
    const uint32_t clear = compact_popc64(~((uint64_t)lo | ((uint64_t)hi << 32)));
    for (uint32_t k = 0; k < clear; ++k) CHECK(compact_kth_clear(lo, hi, k) == kth_clear_loop(lo, hi, k));
}

static void test_kth_clear() {
    check_kth(0u, 0u);  // all clear: the k-th is k
    for (uint32_t k = 0; k < 64; ++k) CHECK(compact_kth_clear(0u, 0u, k) == k);
    for (uint32_t b = 0; b < 32; ++b) {  // one bit set, one bit clear
        check_kth(1u << b, 0u);
        check_kth(0u, 1u << b);
        check_kth(~(1u << b), 0xFFFFFFFFu);
        check_kth(0xFFFFFFFFu, ~(1u << b));
        CHECK(compact_kth_clear(~(1u << b), 0xFFFFFFFFu, 0) == b);
        CHECK(compact_kth_clear(0xFFFFFFFFu, ~(1u << b), 0) == 32 + b);
    }
    std::mt19937 rng(5);
    for (int t = 0; t < 2000; ++t) check_kth(rng(), rng());
    for (int t = 0; t < 500; ++t) check_kth(rng() & rng() & rng(), rng() | rng() | rng());  // sparse and dense words
}

static void test_keep_word() {
    CHECK(compact_keep_word(0u, 0, 32) == 0xFFFFFFFFu);
    CHECK(compact_keep_word(0u, 0, 1) == 1u);
    CHECK(compact_keep_word(0u, 1, 33) == 1u);
    CHECK(compact_keep_word(0u, 1, 32) == 0u);            // the word is wholly past n
    CHECK(compact_keep_word(0xFFFFFFFFu, 0, 32) == 0u);
    CHECK(compact_keep_word(0x80000001u, 0, 31) == 0x7FFFFFFEu);  // bit 31 is past n: ignored, not kept
    const uint64_t n = (1ull << 32) - 1;                  // the largest index
    CHECK(compact_keep_word(0u, (n >> 5), n) == 0x7FFFFFFFu);
    CHECK(compact_blocks(n) == (1u << 22));
    CHECK(compact_blocks(1) == 1 && compact_blocks(1024) == 1 && compact_blocks(1025) == 2);
    CHECK(compact_blocks((1ull << 20) + 1500) == 1026);   // more than one pass of the scan
    static_assert(kCompactBlock == 16 * kCompactGroup && kCompactBlock / 32 == 32, "a block is 16 groups, 32 mask words");
}

static void test_units() {
    CHECK(compact_unit(512, 0x1000, 0x2000) == 16);
    CHECK(compact_unit(512, 0x1004, 0x2000) == 4);
    CHECK(compact_unit(512, 0x1000, 0x2002) == 1);
    CHECK(compact_unit(84, 0x1000, 0x2000) == 4);
    CHECK(compact_unit(42, 0x1000, 0x2000) == 1);
    CHECK(compact_unit(21, 0x1000, 0x2000) == 1);
    CHECK(compact_unit(1, 0x1000, 0x2000) == 1);
    CHECK(compact_unit(4, 0x1000, 0x2000) == 4);   // rnorm
    CHECK(compact_unit(128, 0x1000, 0x2000) == 16);  // 32 packed words
    CHECK(compact_unit(1ull << 32, 0, 0) == 16);
}

// the offsets of the last unit of `row`, and of a run that ends there, against 128-bit arithmetic
static void check_offsets(uint64_t row, uint64_t rb) {
    const uint32_t unit = compact_unit(rb, 0, 0);
    const uint64_t upr = compact_units_per_row(rb, unit);
    CHECK(upr * unit == rb);
    const unsigned __int128 want_row = (unsigned __int128)row * rb;
    CHECK((unsigned __int128)compact_row_offset(row, rb) == want_row);
    CHECK((unsigned __int128)compact_src_offset(row, rb, upr - 1, unit) == want_row + rb - unit);
    // the run of 64 rows that ends with `row`: its last unit is the row's last
    if (row >= 63) {
        const uint64_t row0 = row - 63, u = 64 * upr - 1;
        CHECK((unsigned __int128)compact_dst_offset(row0, rb, u, unit) == want_row + rb - unit);
        uint32_t rank = 0;
        uint64_t within = 0;
        compact_unit_row(u, upr, &rank, &within);
        CHECK(rank == 63 && within == upr - 1);
        compact_unit_row(63 * upr, upr, &rank, &within);
        CHECK(rank == 63 && within == 0);
        compact_unit_row(upr - 1, upr, &rank, &within);
        CHECK(rank == 0 && within == upr - 1);
    }
}

static void test_offsets() {
    const uint64_t widths[] = {1, 21, 42, 84, 512};
    for (uint64_t rb : widths)
        for (uint64_t edge : {1ull << 31, 1ull << 32}) {
            const uint64_t at = edge / rb;  // the row in which, or before which, byte `edge` lies
            for (uint64_t row : {at - 64, at - 1, at, at + 1, at + 64}) check_offsets(row, rb);
        }
    check_offsets((1ull << 32) - 2, 512);   // the last row of the largest index: byte 2^41
    check_offsets(100, 1ull << 37);  // 2^33 units to a row: the 64-bit branch of the unit mapping
    uint32_t rank = 0;
    uint64_t within = 0;
    compact_unit_row((1ull << 32) + 5, 1ull << 29, &rank, &within);  // u past 32 bits
    CHECK(rank == 8 && within == 5);
}

// k_compact.hip's schedule with the same functions, a wave as a loop over 64 lanes
static void emulate(uint64_t n, uint64_t rb, const std::vector<uint32_t> &remove, const std::vector<uint8_t> &src,
                    std::vector<uint8_t> &dst, uint64_t *na) {
    const uint32_t nblk = compact_blocks(n);
    std::vector<uint32_t> cnt(nblk, 0), start(nblk + 1, 0);
    for (uint64_t w = 0; w * 32 < n; ++w) cnt[w >> 5] += compact_popc32(compact_keep_word(remove[w], w, n));
    for (uint32_t b = 0; b < nblk; ++b) start[b + 1] = start[b] + cnt[b];
    *na = start[nblk];
    dst.assign((size_t)(*na * rb), 0xEE);
    std::vector<uint8_t> written(dst.size(), 0);
    const uint32_t unit = compact_unit(rb, 0, 0);
    const uint64_t upr = compact_units_per_row(rb, unit);
    for (uint32_t blk = 0; blk < nblk; ++blk) {
        if (start[blk + 1] == start[blk]) continue;
        uint32_t keep[32], excl[32], run = 0;
        for (uint32_t l = 0; l < 32; ++l) {
            const uint64_t w = (uint64_t)blk * 32 + l;
            keep[l] = w * 32 < n ? compact_keep_word(remove[w], w, n) : 0u;
            excl[l] = run;
            run += compact_popc32(keep[l]);
        }
        for (uint32_t g = 0; g < 16; ++g) {
            const uint64_t keep64 = (uint64_t)keep[2 * g] | ((uint64_t)keep[2 * g + 1] << 32);
            const uint32_t kept = compact_popc64(keep64);
            const uint64_t src_row0 = (uint64_t)blk * kCompactBlock + g * kCompactGroup, dst_row0 = (uint64_t)start[blk] + excl[2 * g];
            const uint64_t total = kept * upr;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint64_t u = lane; u < total; u += 64) {
                    uint32_t rank = 0;
                    uint64_t within = 0;
                    compact_unit_row(u, upr, &rank, &within);
                    const uint64_t row = src_row0 + compact_kth_set(keep64, rank);
                    const uint64_t so = compact_src_offset(row, rb, within, unit), d_o = compact_dst_offset(dst_row0, rb, u, unit);
                    CHECK(row < n && so + unit <= n * rb && d_o + unit <= dst.size());
                    if (row >= n || so + unit > n * rb || d_o + unit > dst.size()) return;
                    std::memcpy(&dst[d_o], &src[so], unit);
                    for (uint32_t b = 0; b < unit; ++b) CHECK(written[d_o + b]++ == 0);  // every byte once
                }
        }
    }
    for (uint8_t wr : written) CHECK(wr == 1);
}

static void test_schedule() {
    std::mt19937 rng(9);
    const uint64_t sizes[] = {1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1501, 2500};
    const uint64_t widths[] = {1, 4, 21, 42, 84, 16, 128};
    for (uint64_t n : sizes)
        for (uint64_t rb : widths)
            for (int pattern = 0; pattern < 5; ++pattern) {
                std::vector<uint32_t> remove((n + 31) / 32, 0);
                for (uint64_t i = 0; i < n; ++i) {
                    bool r = false;
                    if (pattern == 0) r = rng() % 5 == 0;
                    if (pattern == 1) r = i >= 128 && i < 448;
                    if (pattern == 2) r = i != n / 2;  // all but one
                    if (pattern == 3) r = i == 0 || i == n - 1;
                    if (pattern == 4) r = rng() % 2 == 0;
                    if (r) remove[i >> 5] |= 1u << (i & 31);
                }
                if (n % 32) remove.back() |= ~((1u << (n % 32)) - 1u);  // bits at or past n are ignored
                std::vector<uint8_t> src((size_t)(n * rb)), dst, want;
                for (auto &b : src) b = (uint8_t)rng();
                for (uint64_t i = 0; i < n; ++i)
                    if (!((remove[i >> 5] >> (i & 31)) & 1u)) want.insert(want.end(), src.begin() + i * rb, src.begin() + (i + 1) * rb);
                uint64_t na = 0;
                emulate(n, rb, remove, src, dst, &na);
                CHECK(na * rb == want.size());
                CHECK(dst == want);
            }
}

int main() {
    test_kth_clear();
    test_keep_word();
    test_units();
    test_offsets();
    test_schedule();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("COMPACT_OK\n");
    return 0;
}
