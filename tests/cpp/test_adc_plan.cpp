// The ADC search's LDS plan (vq_amd/csrc/adc_plan.hpp), host arithmetic only: for every table size m * k the two
// schedules agree on what they take, every launch fits the CU's LDS and the kernel attribute of its schedule, and the
// batch sizes change at the documented edges.  Driver: tests/test_cpp_adc_plan.py.
#include <cstdio>

#include "adc_plan.hpp"

using namespace vqhip;

static int fails = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

int main() {
    for (uint32_t t = 1; t <= kAdcMaxTable + 64; ++t) {
        const AdcPlan full = adc_full_plan(1, t), fast = adc_fast_plan(1, t);
        if (t > kAdcMaxTable) {  // refused by both
            EXPECT(full.qb == 0 && fast.qb == 0);
            continue;
        }
        if (fails > 20) break;
        // the full pass takes every table the one-scan takes (it repeats the one-scan's flagged queries)
        EXPECT(full.qb >= 1 && full.qb <= 8);
        EXPECT(full.scan_lds == (size_t)full.qb * (t + 512) * 4);
        EXPECT(full.scan_lds <= kAdcFullScanLdsMax && kAdcFullScanLdsMax <= kAdcCuLds);
        // as many queries as fit 150 KiB, at most eight; one query past that (the rule before the largest tables)
        const size_t old_qb = kAdcTableLds / (((size_t)t + 512) * 4);
        EXPECT(full.qb == (old_qb == 0 ? 1 : (old_qb > 8 ? 8 : old_qb)));
        EXPECT(fast.qb == 8 || fast.qb == 4 || fast.qb == 2 || fast.qb == 1);
        EXPECT((size_t)t * fast.qb * 4 <= kAdcTableLds);
        EXPECT(fast.qb == 8 || (size_t)t * fast.qb * 2 * 4 > kAdcTableLds);
        EXPECT(fast.lut_lds == (size_t)adc_tabp(1, t, fast.qb) * 4 && fast.lut_lds % 16 == 0 && fast.lut_lds <= kAdcTableLds);
        // tables, staged candidates (8 B each), counts, list bases and thresholds
        EXPECT(fast.scan_lds == fast.lut_lds + (size_t)fast.qb * (128 * 8 + 12));
        EXPECT(fast.scan_lds <= adc_scan_thr_lds_max(fast.qb) && adc_scan_thr_lds_max(fast.qb) <= kAdcCuLds);
    }
    // the product alone decides
    EXPECT(adc_fast_plan(75, 64).qb == adc_fast_plan(1, 4800).qb && adc_full_plan(150, 256).qb == adc_full_plan(1, 38400).qb);
    // one-scan edges: 8 / 4 / 2 / 1 queries up to 4800 / 9600 / 19200 / 38400
    const uint32_t fast_edges[][2] = {{4800, 8}, {4801, 4}, {9600, 4}, {9601, 2}, {19200, 2}, {19201, 1}, {38400, 1}, {38401, 0}};
    for (const auto &e : fast_edges) EXPECT(adc_fast_plan(1, e[0]).qb == e[1]);
    // full-pass edges: min(8, 150 KiB / ((m k + 512) 4)), then 1 up to 38400
    const uint32_t full_edges[][2] = {{4288, 8}, {4289, 7}, {4973, 7}, {4974, 6}, {5888, 6}, {5889, 5}, {7168, 5}, {7169, 4},
                                      {9088, 4}, {9089, 3}, {12288, 3}, {12289, 2}, {18688, 2}, {18689, 1}, {37888, 1},
                                      {38400, 1}, {38401, 0}};
    for (const auto &e : full_edges) EXPECT(adc_full_plan(1, e[0]).qb == e[1]);
    // the largest requests: 8 queries at m k = 4800 (161,888 B) and one full-pass query at 38400 (155,648 B)
    EXPECT(adc_fast_plan(1, 4800).scan_lds == 161888 && adc_scan_thr_lds_max(8) == 161888);
    EXPECT(adc_full_plan(1, 38400).scan_lds == 155648 && kAdcFullScanLdsMax == 155648);
    EXPECT(!adc_table_fits(11, 3491) && adc_table_fits(150, 256) && !adc_table_fits(65536, 65536));
    if (fails) return 1;
    std::printf("PLAN_OK\n");
    return 0;
}
