// Inverted-file search over PQ codes (include/vqhip.h, vqhip_ivfpq_*).  The index keeps its codes in
// list order: list l holds the rows ids[off[l] .. off[l + 1]) (ascending) and their codes, one contiguous run.  Per query:
//   P(q)    = the nprobe lists the flat search over the coarse centroids returns (launch_knn_search, k_knn.hip),
//   S(q)    = the rows of those lists, taken as ONE sequence of positions: probe slot 0's list, then slot 1's, ...,
//   D(q, i) = the ADC definition of k_adc.hip (the table from k_adc_lut, subspace 0 first, f32, no contraction),
//   result  = the topk rows of S(q) by (adc_key(D), row id) ascending; Euclidean reports sqrtf(D); padding (|S(q)| < topk)
//             idx 0xFFFFFFFF, dist +inf.
// Schedule (launch_ivf_search): k_ivf_plan (each query's prefix over its probed lists' lengths, and the histogram range)
// -> k_ivf_scan (work items = one query x one chunk of its positions: the table in LDS, D written per position, an LDS
// histogram of the distances) -> launch_topk_select (topk.hpp) over IvfSource: the positions of
// S(q), the row id of each through the plan's prefix.  The histogram only decides which positions become candidates;
// every candidate carries its exact unique key, so the result does not depend on the bins.
// A filtered call runs the same schedule over the view of its allowed rows (ivf_view.hpp): off / ids
// are the view's, and the scans' Picked variants read the codes of position j at row pick[j] of the payload.
#include "adc_plan.hpp"
#include "common.hpp"
#include "ivf_plan.hpp"
#include "kernels.hpp"
#include "topk.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// pref[q][0..nprobe]: the first position of each probe slot (pref[q][nprobe] = |S(q)|); seg[q][slot] = off[list];
// bounds[q] = {sum_s min_j t_s, sum_s max_j t_s} in a fixed reduction order (the histogram's range: any monotone bin
// function gives the same result, this one is deterministic)
__global__ __launch_bounds__(1024) void k_ivf_plan(const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                   const uint32_t *__restrict__ off, const float *__restrict__ lut,
                                                   uint32_t m, uint32_t k, uint32_t *__restrict__ pref,
                                                   uint32_t *__restrict__ seg, float *__restrict__ bounds) {
    __shared__ float s_lo[1024], s_hi[1024];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    ivf_plan_prefix(probe, nprobe, nlist, off, pref, seg);
    const float *lq = lut + (size_t)q * m * k;
    float lo = 0.0f, hi = 0.0f;
    for (uint32_t s = t; s < m; s += 1024) {
        float mn = lq[(size_t)s * k], mx = mn;
        for (uint32_t j = 1; j < k; ++j) {
            const float v = lq[(size_t)s * k + j];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
        lo = lo + mn;
        hi = hi + mx;
    }
    s_lo[t] = lo;
    s_hi[t] = hi;
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (t < h) {
            s_lo[t] = s_lo[t] + s_lo[t + h];
            s_hi[t] = s_hi[t] + s_hi[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        bounds[2 * q + 0] = s_lo[0];
        bounds[2 * q + 1] = s_hi[0];
    }
}

// the row of the payload behind position `at` of the list order: the position itself, or -- Picked, a filtered call
// whose pref / seg are the plan over the view's aoff -- pick[at], the view's position `at`
template <bool Picked>
__device__ __forceinline__ uint64_t ivf_code_row(const uint32_t *__restrict__ pick, uint64_t at) {
    if constexpr (Picked) return pick[at];
    return at;
}

// work item (blockIdx.x, blockIdx.y = query): positions [x chunk, (x + 1) chunk) of S(q); items past |S(q)| leave at once.
// W[q][pos] = D, hist[q][bin] += 1 (integer atomics: the counts do not depend on their order)
template <bool Picked>
__global__ __launch_bounds__(256) void k_ivf_scan(const uint8_t *__restrict__ codes, uint32_t m, uint32_t k,
                                                  const float *__restrict__ lut, const uint32_t *__restrict__ pref,
                                                  const uint32_t *__restrict__ seg, uint32_t nprobe,
                                                  const float *__restrict__ bounds, uint32_t chunk, uint64_t wstride,
                                                  float *__restrict__ W, uint32_t *__restrict__ hist,
                                                  const uint32_t *__restrict__ pick) {
    extern __shared__ __attribute__((aligned(16))) float lds_lut[];  // [m][k] table, then [kAdcBins] histogram
    const uint32_t q = blockIdx.y, tab = m * k;
    const uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    const uint32_t *sq = seg + (size_t)q * nprobe;
    const uint32_t total = (uint32_t)min((uint64_t)pq[nprobe], wstride);
    const uint64_t p0 = (uint64_t)blockIdx.x * chunk;
    if (p0 >= total) return;  // (uniform)
    const uint32_t p1 = (uint32_t)min((uint64_t)total, p0 + chunk);
    uint32_t *lds_hist = reinterpret_cast<uint32_t *>(lds_lut + tab);
    const float *lq = lut + (size_t)q * tab;
    for (uint32_t e = threadIdx.x; e < tab; e += 256) lds_lut[e] = lq[e];
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256) lds_hist[e] = 0u;
    const float lo = bounds[2 * q], scale = adc_scale(lo, bounds[2 * q + 1]);
    __syncthreads();
    const bool words = k <= 256 && (m & 7u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0;
    float *wq = W + (size_t)q * wstride;
    uint32_t pos = (uint32_t)p0 + threadIdx.x;
    if (pos < p1) {
        uint32_t slot = ivf_slot(pq, nprobe, pos), first = pq[slot], next = pq[slot + 1];
        for (; pos < p1; pos += 256) {
            while (pos >= next) {  // (empty lists: several steps)
                ++slot;
                first = next;
                next = pq[slot + 1];
            }
            float acc[1];  // (topk.hpp's adc_row, the ADC scans' operation order, for one query's table)
            adc_row<1>(codes, ivf_code_row<Picked>(pick, (uint64_t)sq[slot] + (pos - first)), m, k, words, lds_lut, 1u, 0u, acc);
            const float dv = acc[0];
            wq[pos] = dv;
            atomicAdd(&lds_hist[adc_bin(dv, lo, scale)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256)
        if (lds_hist[e]) atomicAdd(&hist[(size_t)q * kAdcBins + e], lds_hist[e]);
}

// the scans' output as a source of the selection stage (topk.hpp): W[q][wstride] over the positions of S(q), the row id
// of a position through the plan's prefix, the scans' float bins over bounds[q]
struct IvfSource {
    using Pos = uint32_t;
    const float *W;
    uint64_t wstride;
    const uint32_t *pref, *seg, *ids;
    uint32_t nprobe;
    const float *bounds;
    uint32_t total = 0;  // (device: of the opened query)
    float lo = 0, scale = 0;
    __device__ void open(uint32_t q) {
        W += (size_t)q * wstride;
        pref += (size_t)q * (nprobe + 1);
        seg += (size_t)q * nprobe;
        total = (uint32_t)min((uint64_t)pref[nprobe], wstride);
        lo = bounds[2 * q];
        scale = adc_scale(lo, bounds[2 * q + 1]);
    }
    __device__ Pos count() const { return total; }
    __device__ float at(Pos pos) const { return W[pos]; }
    __device__ uint32_t id(Pos pos) const { return ids[ivf_row(pref, seg, nprobe, pos)]; }
    __device__ uint32_t bin(float dval) const { return adc_bin(dval, lo, scale); }
    uint32_t blocks() const { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((wstride + 255) / 256, 1), 64); }
};

// ---- residual lists (VQHIP_IVF_RESIDUAL) ----
// A row of list l holds the codes of x - C[l], so its distance to q is the ADC definition applied to r = q - C[l] (f32,
// one rounding per element): one table per (query, probe slot).  k_ivf_rlut writes them, tabs[q][slot][m][k], and
// mm[q][slot] = {sum_s min_j, sum_s max_j}; k_ivf_rplan reduces those over the query's slots into the histogram range;
// k_ivf_rscan is k_ivf_scan with the slot's table reloaded into LDS at every slot boundary of its chunk.
constexpr uint32_t kIvfRSlots = 8;    // probe slots per k_ivf_rlut block (their residuals in LDS, one codebook read)
constexpr uint32_t kIvfRStage = 4096; // residual floats a k_ivf_rlut block stages (kIvfRSlots x sub_dim); past it, computed in place
constexpr uint32_t kIvfNoList = 0xFFFFFFFFu;

__device__ __forceinline__ float ivf_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float ivf_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block (x = group of kIvfRSlots probe slots, y = query), 256 threads: for each subspace s, thread j's centroid cb[s][j]
// against the group's residual sub-vectors (k_adc_lut's term: diff = r[t] - cb[s][j][t] from -0.0 (L2) or 0.0 (L1),
// t ascending, no contraction).  SD > 0: sub_dim == SD, the centroid held in registers; SD == 0: any sub_dim.  Empty
// slots (and a list id >= nlist) get no table.  The ranges are reduced in a fixed order: min / max over the lanes of a
// wave (xor tree), over the four waves in order, summed over the subspaces in order.
template <uint32_t SD>
__global__ __launch_bounds__(256) void k_ivf_rlut(const float *__restrict__ queries, const float *__restrict__ coarse,
                                                  const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                  const uint32_t *__restrict__ off, const float *__restrict__ cb, uint32_t m,
                                                  uint32_t k, uint32_t sd, int l1, float *__restrict__ tabs,
                                                  float *__restrict__ mm) {
    __shared__ __attribute__((aligned(16))) float rs[kIvfRStage];  // [slot in group][sd] residuals of subspace s
    __shared__ uint32_t s_list[kIvfRSlots];
    __shared__ float s_red[2][4][kIvfRSlots], s_sum[2][kIvfRSlots];
    const uint32_t q = blockIdx.y, g0 = blockIdx.x * kIvfRSlots, gn = min(kIvfRSlots, nprobe - g0);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t dim = m * sd, tab = m * k;
    if (tid < gn) {
        const uint32_t l = probe[(size_t)q * nprobe + g0 + tid];
        s_list[tid] = (l < nlist && off[l + 1] > off[l]) ? l : kIvfNoList;
    }
    __syncthreads();
    const float *x = queries + (size_t)q * dim;
    const bool staged = kIvfRSlots * sd <= kIvfRStage;  // (uniform; always with SD > 0)
    for (uint32_t s = 0; s < m; ++s) {
        if (staged)
            for (uint32_t e = tid; e < gn * sd; e += 256) {
                const uint32_t g = e / sd, u = s * sd + (e - g * sd), l = s_list[g];
                if (l != kIvfNoList) rs[e] = x[u] - coarse[(size_t)l * dim + u];
            }
        __syncthreads();
        for (uint32_t j0 = 0; j0 < k; j0 += 256) {
            const uint32_t j = j0 + tid;
            const bool active = j < k;
            const float *c = cb + ((size_t)s * k + (active ? j : 0)) * sd;
            float creg[SD > 0 ? SD : 1];
            if constexpr (SD > 0) {
#pragma unroll
                for (uint32_t t = 0; t < SD; ++t) creg[t] = c[t];
            }
            for (uint32_t g = 0; g < gn; ++g) {
                const uint32_t l = s_list[g];
                if (l == kIvfNoList) continue;  // (uniform)
                float acc = l1 ? 0.0f : -0.0f;
                if constexpr (SD > 0) {
#pragma unroll
                    for (uint32_t t = 0; t < SD; ++t) {
                        const float diff = rs[g * SD + t] - creg[t];
                        if (l1) {
                            acc = acc + fabsf(diff);
                        } else {
                            const float sq = diff * diff;
                            acc = acc + sq;
                        }
                    }
                } else {
                    const float *cl = coarse + (size_t)l * dim + (size_t)s * sd;
                    for (uint32_t t = 0; t < sd; ++t) {
                        const float r = staged ? rs[g * sd + t] : x[(size_t)s * sd + t] - cl[t];
                        const float diff = r - c[t];
                        if (l1) {
                            acc = acc + fabsf(diff);
                        } else {
                            const float sq = diff * diff;
                            acc = acc + sq;
                        }
                    }
                }
                if (active) tabs[((size_t)q * nprobe + g0 + g) * tab + (size_t)s * k + j] = acc;
                const float mn = ivf_wave_min(active ? acc : __builtin_inff());
                const float mx = ivf_wave_max(active ? acc : -__builtin_inff());
                if (lane == 0) {
                    s_red[0][wave][g] = j0 == 0 ? mn : fminf(s_red[0][wave][g], mn);
                    s_red[1][wave][g] = j0 == 0 ? mx : fmaxf(s_red[1][wave][g], mx);
                }
            }
        }
        __syncthreads();
        if (tid < gn) {
            const float mn = fminf(fminf(fminf(s_red[0][0][tid], s_red[0][1][tid]), s_red[0][2][tid]), s_red[0][3][tid]);
            const float mx = fmaxf(fmaxf(fmaxf(s_red[1][0][tid], s_red[1][1][tid]), s_red[1][2][tid]), s_red[1][3][tid]);
            s_sum[0][tid] = s == 0 ? mn : s_sum[0][tid] + mn;
            s_sum[1][tid] = s == 0 ? mx : s_sum[1][tid] + mx;
        }
        // (the next subspace's staging writes rs only; s_red is written again after its barrier)
    }
    if (tid < gn) {
        mm[2 * ((size_t)q * nprobe + g0 + tid) + 0] = s_sum[0][tid];
        mm[2 * ((size_t)q * nprobe + g0 + tid) + 1] = s_sum[1][tid];
    }
}

// k_ivf_plan's prefix and segments, and bounds[q] = {min over the non-empty slots of mm.lo, max of mm.hi} (a fixed tree;
// {0, 0} when every probed list is empty)
__global__ __launch_bounds__(1024) void k_ivf_rplan(const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                    const uint32_t *__restrict__ off, const float *__restrict__ mm,
                                                    uint32_t *__restrict__ pref, uint32_t *__restrict__ seg,
                                                    float *__restrict__ bounds) {
    __shared__ float s_lo[1024], s_hi[1024];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    const uint32_t len = ivf_plan_prefix(probe, nprobe, nlist, off, pref, seg);
    const bool real = t < nprobe && len > 0;
    s_lo[t] = real ? mm[2 * ((size_t)q * nprobe + t) + 0] : __builtin_inff();
    s_hi[t] = real ? mm[2 * ((size_t)q * nprobe + t) + 1] : -__builtin_inff();
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (t < h) {
            s_lo[t] = fminf(s_lo[t], s_lo[t + h]);
            s_hi[t] = fmaxf(s_hi[t], s_hi[t + h]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const bool none = !(s_lo[0] <= s_hi[0]);
        bounds[2 * q + 0] = none ? 0.0f : s_lo[0];
        bounds[2 * q + 1] = none ? 0.0f : s_hi[0];
    }
}

// k_ivf_scan over residual lists: the chunk [p0, p1) of S(q) in slot runs; at each slot boundary the block (uniformly)
// loads that slot's table into LDS.  W and the histogram exactly as k_ivf_scan writes them.
template <bool Picked>
__global__ __launch_bounds__(256) void k_ivf_rscan(const uint8_t *__restrict__ codes, uint32_t m, uint32_t k,
                                                   const float *__restrict__ tabs, const uint32_t *__restrict__ pref,
                                                   const uint32_t *__restrict__ seg, uint32_t nprobe,
                                                   const float *__restrict__ bounds, uint32_t chunk, uint64_t wstride,
                                                   float *__restrict__ W, uint32_t *__restrict__ hist,
                                                   const uint32_t *__restrict__ pick) {
    extern __shared__ __attribute__((aligned(16))) float lds_lut[];  // [m][k] table, then [kAdcBins] histogram
    const uint32_t q = blockIdx.y, tab = m * k;
    const uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    const uint32_t *sq = seg + (size_t)q * nprobe;
    const uint32_t total = (uint32_t)min((uint64_t)pq[nprobe], wstride);
    const uint64_t p0 = (uint64_t)blockIdx.x * chunk;
    if (p0 >= total) return;  // (uniform)
    const uint32_t p1 = (uint32_t)min((uint64_t)total, p0 + chunk);
    uint32_t *lds_hist = reinterpret_cast<uint32_t *>(lds_lut + tab);
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256) lds_hist[e] = 0u;
    const float lo = bounds[2 * q], scale = adc_scale(lo, bounds[2 * q + 1]);
    const bool words = k <= 256 && (m & 7u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0;
    const bool vec = (tab & 3u) == 0;  // (every table then starts on 16 bytes)
    float *wq = W + (size_t)q * wstride;
    for (uint32_t slot = ivf_slot(pq, nprobe, (uint32_t)p0); slot < nprobe && pq[slot] < p1; ++slot) {
        const uint32_t a = max((uint32_t)p0, pq[slot]), b = min(p1, pq[slot + 1]);
        if (a >= b) continue;  // an empty list (uniform)
        const float *ts = tabs + ((size_t)q * nprobe + slot) * tab;
        __syncthreads();  // (the previous slot's reads of the table are done)
        if (vec) {
            for (uint32_t e = 4 * threadIdx.x; e < tab; e += 4 * 256)
                *reinterpret_cast<float4 *>(lds_lut + e) = *reinterpret_cast<const float4 *>(ts + e);
        } else {
            for (uint32_t e = threadIdx.x; e < tab; e += 256) lds_lut[e] = ts[e];
        }
        __syncthreads();
        for (uint32_t pos = a + threadIdx.x; pos < b; pos += 256) {
            float acc[1];  // (topk.hpp's adc_row, the ADC scans' operation order, for one table)
            adc_row<1>(codes, ivf_code_row<Picked>(pick, (uint64_t)sq[slot] + (pos - pq[slot])), m, k, words, lds_lut, 1u, 0u, acc);
            const float dv = acc[0];
            wq[pos] = dv;
            atomicAdd(&lds_hist[adc_bin(dv, lo, scale)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kAdcBins; e += 256)
        if (lds_hist[e]) atomicAdd(&hist[(size_t)q * kAdcBins + e], lds_hist[e]);
}

}  // namespace

// positions per scan work item: about four items per CU over the batch's expected positions, whole passes of the block
uint32_t ivf_chunk(uint64_t expected_positions) {
    const uint64_t per_item = expected_positions / (4 * (uint64_t)num_cus());
    const uint64_t c = (per_item + 255) / 256 * 256;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c, 512), 8192);
}

// the dynamic LDS the scans take (up to the table limit), once per device
static int ivf_attrs() {
    static PerDeviceOnce attr;
    if (attr.needed()) {
        for (const void *scan : {reinterpret_cast<const void *>(k_ivf_scan<false>), reinterpret_cast<const void *>(k_ivf_scan<true>),
                                 reinterpret_cast<const void *>(k_ivf_rscan<false>), reinterpret_cast<const void *>(k_ivf_rscan<true>)})
            VQ_HIP(hipFuncSetAttribute(scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAdcFullScanLdsMax));
        attr.done();
    }
    return VQHIP_OK;
}

// One batch of nb queries whose probe lists (probe [nb][nprobe], launch_knn_search) and tables (lut [nb][m][k],
// launch_adc_lut) are on the device.  codes / ids / off: the index in list order.  W [nb][wstride] with wstride >= every
// |S(q)|; pref [nb][nprobe + 1], seg [nb][nprobe], bounds [nb][2], state >= topk_state_bytes(nb) (zeroed here),
// cand >= topk_cand_bytes(nb).  Results [nb][topk] on the device.  pick: a filtered call's (ivf_view.hpp) -- ids / off are
// then the view's aids / aoff, and position j of that list order is row pick[j] of codes; NULL: every row.
int launch_ivf_search(const uint8_t *codes, const uint32_t *ids, const uint32_t *off, uint32_t nlist, uint32_t m, uint32_t k, int metric,
                      const float *lut, const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk,
                      uint64_t wstride, float *W, uint32_t *pref, uint32_t *seg, float *bounds, void *state,
                      unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream, const uint32_t *pick) {
    if (nb == 0) return VQHIP_OK;
    if (nprobe == 0 || nprobe > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "nprobe must be in [1, 1024]");
    if (topk == 0 || topk > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, 1024]");
    if (!adc_table_fits(m, k)) return fail_adc_table(m, k);
    const size_t scan_lds = ((size_t)m * k + kAdcBins) * 4;
    VQ_TRY(ivf_attrs());
    const TopkState st = topk_state(state, nb);
    VQ_HIP(hipMemsetAsync(state, 0, topk_state_bytes(nb), stream));
    hipLaunchKernelGGL(k_ivf_plan, dim3(nb), dim3(1024), 0, stream, probe, nprobe, nlist, off, lut, m, k, pref, seg, bounds);
    VQ_LAUNCH_CHECK("k_ivf_plan");
    const uint64_t items = (wstride + chunk - 1) / chunk;
    if (items > 0) {
        hipLaunchKernelGGL(pick ? k_ivf_scan<true> : k_ivf_scan<false>, dim3((uint32_t)items, nb), dim3(256), scan_lds, stream, codes, m,
                           k, lut, pref, seg, nprobe, bounds, chunk, wstride, W, st.hist, pick);
        VQ_LAUNCH_CHECK("k_ivf_scan");
    }
    return launch_topk_select(IvfSource{W, wstride, pref, seg, ids, nprobe, bounds}, nb, topk, metric == VQHIP_EUCLIDEAN ? 1 : 0, st, cand,
                              idx_out, dist_out, stream);
}

size_t ivf_rtab_bytes(uint32_t qb, uint32_t nprobe, uint32_t m, uint32_t k) { return (size_t)qb * nprobe * m * k * 4; }
size_t ivf_rmm_bytes(uint32_t qb, uint32_t nprobe) { return (size_t)qb * nprobe * 2 * 4; }

// residual lists: a scan item reloads the table at each slot boundary of its chunk, m k floats against m LDS reads per
// position.  The chunk is at least 4 k positions (rounded to whole block passes), so one reload costs at most a quarter
// of the chunk's table reads; the rest as ivf_chunk.
uint32_t ivf_rchunk(uint64_t expected_positions, uint32_t k) {
    const uint64_t c = std::max<uint64_t>(ivf_chunk(expected_positions), ((uint64_t)4 * k + 255) / 256 * 256);
    return (uint32_t)std::min<uint64_t>(c, 8192);
}

// One batch of nb queries over residual lists: queries [nb][dim] and probe [nb][nprobe] on the device, coarse [nlist][dim]
// and cb [m][k][sd] the index's.  tabs >= ivf_rtab_bytes(nb, nprobe, m, k), mm >= ivf_rmm_bytes(nb, nprobe); the rest as
// launch_ivf_search.  Under a view, k_ivf_rlut and k_ivf_rplan see the same aoff: a probe slot without an allowed row
// gets no table and takes no part in the histogram range.
int launch_ivf_rsearch(const uint8_t *codes, const uint32_t *ids, const uint32_t *off, const float *coarse, uint32_t nlist,
                       const float *cb, uint32_t m, uint32_t k, uint32_t sd, int metric, const float *queries,
                       const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk, uint64_t wstride,
                       float *tabs, float *mm, float *W, uint32_t *pref, uint32_t *seg, float *bounds, void *state,
                       unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream, const uint32_t *pick) {
    if (nb == 0) return VQHIP_OK;
    if (nprobe == 0 || nprobe > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "nprobe must be in [1, 1024]");
    if (topk == 0 || topk > 1024) return fail(VQHIP_ERR_INVALID_INPUT, "topk must be in [1, 1024]");
    if (!adc_table_fits(m, k)) return fail_adc_table(m, k);
    const size_t scan_lds = ((size_t)m * k + kAdcBins) * 4;
    VQ_TRY(ivf_attrs());
    const int l1 = metric == VQHIP_MANHATTAN ? 1 : 0;
    const TopkState st = topk_state(state, nb);
    VQ_HIP(hipMemsetAsync(state, 0, topk_state_bytes(nb), stream));
    const dim3 tgrid((nprobe + kIvfRSlots - 1) / kIvfRSlots, nb);
    auto *rlut = sd == 16 ? k_ivf_rlut<16> : sd == 8 ? k_ivf_rlut<8> : sd == 4 ? k_ivf_rlut<4> : k_ivf_rlut<0>;
    hipLaunchKernelGGL(rlut, tgrid, dim3(256), 0, stream, queries, coarse, probe, nprobe, nlist, off, cb, m, k, sd, l1, tabs, mm);
    VQ_LAUNCH_CHECK("k_ivf_rlut");
    hipLaunchKernelGGL(k_ivf_rplan, dim3(nb), dim3(1024), 0, stream, probe, nprobe, nlist, off, mm, pref, seg, bounds);
    VQ_LAUNCH_CHECK("k_ivf_rplan");
    const uint64_t items = (wstride + chunk - 1) / chunk;
    if (items > 0) {
        hipLaunchKernelGGL(pick ? k_ivf_rscan<true> : k_ivf_rscan<false>, dim3((uint32_t)items, nb), dim3(256), scan_lds, stream, codes,
                           m, k, tabs, pref, seg, nprobe, bounds, chunk, wstride, W, st.hist, pick);
        VQ_LAUNCH_CHECK("k_ivf_rscan");
    }
    return launch_topk_select(IvfSource{W, wstride, pref, seg, ids, nprobe, bounds}, nb, topk, metric == VQHIP_EUCLIDEAN ? 1 : 0, st, cand,
                              idx_out, dist_out, stream);
}

}  // namespace vqhip
