// adc_plan.hpp -- the LDS plan of the ADC search (k_adc.hip): how many queries' tables share one workgroup's LDS and the
// exact dynamic LDS bytes each launch asks for, for both schedules.  Eligibility, workspace sizing, the launches and the
// kernels' MaxDynamicSharedMemorySize all come from here.  Host arithmetic only (no HIP): tests/cpp/test_adc_plan.cpp
// checks it against the CU's LDS.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vqhip {

constexpr size_t kAdcCuLds = 160 * 1024;        // LDS of one gfx950 CU: the most one workgroup can have
constexpr size_t kAdcTableLds = 150 * 1024;     // LDS a batch's tables may take (the rest: histograms, staged candidates)
constexpr uint32_t kAdcMaxTable = 38400;        // m * k: one query's f32 table in kAdcTableLds -- the largest ADC table
constexpr uint32_t kAdcBins = 512;              // histogram bins per query of the full pass's candidate filter
constexpr uint32_t kAdcStage = 128;             // candidates a one-scan workgroup stages per query before it appends them

constexpr bool adc_table_fits(uint32_t m, uint32_t k) { return (uint64_t)m * k <= kAdcMaxTable; }

// floats per batch of interleaved one-scan tables [m][k][qb], in whole 16-byte units
constexpr uint32_t adc_tabp(uint32_t m, uint32_t k, uint32_t qb) { return (m * k * qb + 3u) & ~3u; }

struct AdcPlan {
    uint32_t qb;      // queries per batch; 0: the table does not fit
    size_t scan_lds;  // dynamic LDS of the scan kernel (k_adc_scan / k_adc_scan_thr)
    size_t lut_lds;   // dynamic LDS of the one-scan sampler (k_adc_thresh): the batch's tables alone
};

// The full pass: k_adc_scan holds [qb][m][k] tables then [qb][kAdcBins] histograms.  As many queries as fit
// kAdcTableLds, at most eight; one query past that up to the largest table (k_adc_scan has no static LDS, the CU's
// whole LDS is its to take).
constexpr AdcPlan adc_full_plan(uint32_t m, uint32_t k) {
    if (!adc_table_fits(m, k)) return {0, 0, 0};
    const size_t per_query = ((size_t)m * k + kAdcBins) * 4;
    size_t qb = kAdcTableLds / per_query;
    qb = qb > 8 ? 8 : (qb < 1 ? 1 : qb);
    return {(uint32_t)qb, qb * per_query, 0};
}

// k_adc_scan_thr's dynamic LDS at qb queries per batch and `tab_floats` of tables: the tables, the staged candidates
// [qb][kAdcStage] (8 bytes each), their counts [qb], the list bases [qb] and the thresholds [qb]
constexpr size_t adc_scan_thr_lds(uint32_t qb, size_t tab_floats) { return tab_floats * 4 + (size_t)qb * (kAdcStage * 8 + 3 * 4); }

// The one-scan schedule: the largest power of two up to eight whose interleaved tables fit kAdcTableLds.
constexpr AdcPlan adc_fast_plan(uint32_t m, uint32_t k) {
    if (!adc_table_fits(m, k)) return {0, 0, 0};
    uint32_t qb = 8;
    while (qb > 1 && (size_t)m * k * qb * 4 > kAdcTableLds) qb >>= 1;
    const size_t tab = adc_tabp(m, k, qb);
    return {qb, adc_scan_thr_lds(qb, tab), tab * 4};
}

// the most dynamic LDS a kernel of each schedule is ever launched with (its MaxDynamicSharedMemorySize)
constexpr size_t kAdcFullScanLdsMax =
    kAdcTableLds > ((size_t)kAdcMaxTable + kAdcBins) * 4 ? kAdcTableLds : ((size_t)kAdcMaxTable + kAdcBins) * 4;
constexpr size_t adc_scan_thr_lds_max(uint32_t qb) { return adc_scan_thr_lds(qb, kAdcTableLds / 4); }
static_assert(kAdcFullScanLdsMax <= kAdcCuLds && adc_scan_thr_lds_max(8) <= kAdcCuLds, "an ADC plan exceeds the CU's LDS");

}  // namespace vqhip
