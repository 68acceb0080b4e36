// Inverted-file search over SQ codes (include/vqhip.h, vqhip_ivfsq_*): k_ivfflat.hip's search with the
// row side read as one byte per dimension and decoded where it leaves global memory, as k_sqindex.hip decodes it:
//   v(c)    = mn + (float)c * step for every byte value c (sq_decode.hpp: two roundings, never fused),
//   D(q, i) = the flat index's distance over the decoded row (knn_tile.hpp: knn_step from -0.0 over ascending
//             dimensions, knn_finish), so every result equals IVFFlatIndex over the dequantized rows in the same lists.
// The index keeps its codes in list order: list l is the run C[off[l] * d .. off[l + 1] * d) of one buffer the index owns,
// so with d % 16 == 0 (d % 4 == 0) every row of every list starts on a 16-byte (4-byte) boundary.
// Schedule of one batch (launch_ivfsq_search): section 14's, step for step --
//   launch_ivff_plan    k_ivff_plan, k_ivff_lists, k_ivff_invert (k_ivfflat.hip): pref / seg, cnt, the inverted probe table
//   k_ivfsq_tile        k_ivff_tile with the row chunk loaded as codes: 16, 4 or 1 byte per load (LW)
//   k_ivfsq_scan        k_ivff_scan with the row walked as dwords (W4) or bytes
//   launch_ivff_select  k_ivff_hist and the selection stage over IvffSource (k_ivfflat.hip)
// Which kernel computes a pair depends on the batch; both run one pair's operations in one order, so the bits do not.
// A range search (launch_ivfsq_range) puts the range stage (launch_ivff_range) behind the same
// plan and distance passes.
#include "common.hpp"
#include "ivf_plan.hpp"
#include "kernels.hpp"
#include "knn_tile.hpp"
#include "sq_decode.hpp"

#include <type_traits>

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// block (x = query tile of the batch's tstart[nlist] tiles, y = column of row tiles): k_sq_dist over the rows of one list
// and the up to 128 queries of one tile of its run of inv.  Blocks past the last tile leave at once.  LW = bytes per
// load of the row loader: a chunk of a row starts at byte (off[l] + r) * d + t0 with t0 a multiple of 32, so d % LW == 0
// and an LW-aligned base align every load; a load is issued only where its row is inside the list and its first
// dimension below tc (a multiple of LW).  Padded rows and dimensions are 0.0f in the tile and never reach a result.
template <int METRIC, int LW>
__global__ __launch_bounds__(256) void k_ivfsq_tile(const float *__restrict__ Q, const uint8_t *__restrict__ C, uint32_t d, float mn,
                                                    float step, const float *__restrict__ qnorm, const float *__restrict__ rnorm,
                                                    const uint32_t *__restrict__ off, uint32_t nlist, const uint32_t *__restrict__ cnt,
                                                    const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ tstart,
                                                    const uint32_t *__restrict__ inv, const uint32_t *__restrict__ pref,
                                                    uint32_t nprobe, uint64_t wstride, float *__restrict__ W,
                                                    uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, KC = kKnnKC;
    __shared__ __attribute__((aligned(16))) float qs[KC][TQ + 4];
    __shared__ __attribute__((aligned(16))) float rs[KC][TR + 4];
    __shared__ uint32_t s_q[TQ], s_p[TQ];  // the tile's queries (0xFFFFFFFF: none) and the first position of the list in each
    const uint32_t tile = blockIdx.x;
    if (tile >= tstart[nlist]) return;  // (uniform)
    uint32_t l = 0;
    {  // the last list whose first tile is <= tile, and that has tiles (tstart is non-decreasing)
        uint32_t lo = 0, hi = nlist;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tstart[mid] <= tile) lo = mid;
            else hi = mid;
        }
        l = lo;
    }
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4;
    const uint32_t e0 = (tile - tstart[l]) * TQ, en = min(TQ, cnt[l] - e0);
    const uint32_t row0 = off[l], nrows = off[l + 1] - row0;
    const uint8_t *Cl = C + (uint64_t)row0 * d;  // the list's run
    if (tid < TQ) {
        uint32_t q = 0xFFFFFFFFu, p = 0;
        if (tid < en) {
            const uint32_t e = inv[lstart[l] + e0 + tid];
            q = e / nprobe;
            p = pref[(size_t)q * (nprobe + 1) + (e - q * nprobe)];
        }
        s_q[tid] = q;
        s_p[tid] = p;
    }
    __syncthreads();
    float qn[RQ];
    uint32_t lo[RQ], hi[RQ], qi[RQ];
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
        qi[a] = s_q[qg * RQ + a];
        qn[a] = (vq_is_cos(METRIC) && qi[a] != 0xFFFFFFFFu) ? qnorm[qi[a]] : 1.0f;
        lo[a] = 0xFFFFFFFFu;
        hi[a] = 0u;
    }
    const uint32_t nrt = (nrows + TR - 1) / TR;
    for (uint32_t rt = blockIdx.y; rt < nrt; rt += gridDim.y) {
        const uint32_t r0 = rt * TR;  // (within the list)
        float acc[RQ][RR];
#pragma unroll
        for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
            for (uint32_t b = 0; b < RR; ++b) acc[a][b] = -0.0f;
        for (uint32_t t0 = 0; t0 < d; t0 += KC) {
            const uint32_t tc = min(KC, d - t0);
            __syncthreads();  // the previous chunk's readers are done
#pragma unroll
            for (uint32_t e = 0; e < TQ * KC / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / KC, c = idx % KC;
                const uint32_t q = s_q[r];
                qs[c][r] = (q != 0xFFFFFFFFu && c < tc) ? Q[(size_t)q * d + t0 + c] : 0.0f;
            }
            if constexpr (LW == 16) {  // 64 rows x two 16-byte halves: the first 128 lanes
                if (tid < TR * KC / 16) {
                    const uint32_t r = tid >> 1, c0 = (tid & 1u) * 16;
                    const bool ok = r0 + r < nrows && c0 < tc;
                    uint4 w = make_uint4(0, 0, 0, 0);
                    if (ok) w = *reinterpret_cast<const uint4 *>(Cl + (uint64_t)(r0 + r) * d + t0 + c0);
                    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (uint32_t j = 0; j < 16; ++j)
                        rs[c0 + j][r] = ok ? sq_val((ws[j >> 2] >> (8 * (j & 3))) & 0xffu, mn, step) : 0.0f;
                }
            } else if constexpr (LW == 4) {  // 64 rows x eight dwords: two per lane
#pragma unroll
                for (uint32_t e = 0; e < TR * KC / 4 / 256; ++e) {
                    const uint32_t idx = tid + 256 * e, r = idx / (KC / 4), c0 = (idx % (KC / 4)) * 4;
                    const bool ok = r0 + r < nrows && c0 < tc;
                    uint32_t w = 0;
                    if (ok) w = *reinterpret_cast<const uint32_t *>(Cl + (uint64_t)(r0 + r) * d + t0 + c0);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) rs[c0 + j][r] = ok ? sq_val((w >> (8 * j)) & 0xffu, mn, step) : 0.0f;
                }
            } else {
#pragma unroll
                for (uint32_t e = 0; e < TR * KC / 256; ++e) {
                    const uint32_t idx = tid + 256 * e, r = idx / KC, c = idx % KC;
                    rs[c][r] = (r0 + r < nrows && c < tc) ? sq_val(Cl[(uint64_t)(r0 + r) * d + t0 + c], mn, step) : 0.0f;
                }
            }
            __syncthreads();
            auto advance = [&](uint32_t t) {
                const float4 qa = *reinterpret_cast<const float4 *>(&qs[t][qg * RQ]);
                const float4 qb = *reinterpret_cast<const float4 *>(&qs[t][qg * RQ + 4]);
                const float4 rv = *reinterpret_cast<const float4 *>(&rs[t][rg * RR]);
                const float qv[RQ] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                const float rr[RR] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
                    for (uint32_t b = 0; b < RR; ++b) acc[a][b] = knn_step<METRIC>(acc[a][b], qv[a], rr[b]);
            };
            if (tc == KC) {  // (unrolled by 8, as k_knn_dist: fully, the LDS reads cost a wave per SIMD)
#pragma unroll 8
                for (uint32_t t = 0; t < KC; ++t) advance(t);
            } else {
                for (uint32_t t = 0; t < tc; ++t) advance(t);
            }
        }
        const uint32_t rb = r0 + rg * RR;
        float rn[RR];
#pragma unroll
        for (uint32_t b = 0; b < RR; ++b) rn[b] = (vq_is_cos(METRIC) && rb + b < nrows) ? rnorm[(uint64_t)row0 + rb + b] : 1.0f;
#pragma unroll
        for (uint32_t a = 0; a < RQ; ++a) {
            if (qi[a] == 0xFFFFFFFFu) continue;
            float *wq = W + (size_t)qi[a] * wstride;
            const uint64_t p0 = (uint64_t)s_p[qg * RQ + a] + rb;
#pragma unroll
            for (uint32_t b = 0; b < RR; ++b) {
                if (rb + b >= nrows || p0 + b >= wstride) continue;
                const float dv = knn_finish<METRIC>(acc[a][b], qn[a], rn[b]);
                const uint32_t key = adc_key(dv);
                if (key != 0xFFFFFFFFu) {
                    lo[a] = min(lo[a], key);
                    hi[a] = max(hi[a], key);
                }
                wq[p0 + b] = dv;  // (a run starts at any position: no 16-byte stores)
            }
        }
    }
    // the 16 lanes of a query group (lane bits 0-3) hold all of the workgroup's rows for its 8 queries
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
#pragma unroll
        for (uint32_t o = 1; o < 16; o <<= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], (int)o));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], (int)o));
        }
        if (rg == 0 && qi[a] != 0xFFFFFFFFu && lo[a] <= hi[a]) {
            atomicMin(&kmin[qi[a]], lo[a]);
            atomicMax(&kmax[qi[a]], hi[a]);
        }
    }
}

// block (x = chunk of positions, y = query): the positions of the chunk whose list fewer than kIvffTileMin queries probe,
// one per lane and pass; the query's dimensions in LDS, kIvffQC at a time.  Items past |S(q)| leave at once.  W4: the
// codes start on a 4-byte boundary and d % 4 == 0, so every row does and is walked as dwords.
template <int METRIC, bool W4>
__global__ __launch_bounds__(256) void k_ivfsq_scan(const float *__restrict__ Q, const uint8_t *__restrict__ C, uint32_t d, float mn,
                                                    float step, const float *__restrict__ qnorm, const float *__restrict__ rnorm,
                                                    const uint32_t *__restrict__ probe, const uint32_t *__restrict__ cnt,
                                                    const uint32_t *__restrict__ pref, const uint32_t *__restrict__ seg,
                                                    uint32_t nprobe, uint32_t chunk, uint64_t wstride, float *__restrict__ W,
                                                    uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    __shared__ __attribute__((aligned(16))) float s_x[kIvffQC];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    const uint32_t *sq = seg + (size_t)q * nprobe;
    const uint32_t *lq = probe + (size_t)q * nprobe;
    const uint32_t total = (uint32_t)min((uint64_t)pq[nprobe], wstride);
    const uint64_t p0 = (uint64_t)blockIdx.x * chunk;
    if (p0 >= total) return;  // (uniform)
    const uint32_t p1 = (uint32_t)min((uint64_t)total, p0 + chunk);
    const float *x = Q + (size_t)q * d;
    const float qn = vq_is_cos(METRIC) ? qnorm[q] : 1.0f;
    const bool once = d <= kIvffQC;  // the whole query stays in LDS
    if (once) {
        for (uint32_t t = tid; t < d; t += 256) s_x[t] = x[t];
        __syncthreads();
    }
    float *wq = W + (size_t)q * wstride;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t base = (uint32_t)p0; base < p1; base += 256) {
        const uint32_t pos = base + tid;
        bool mine = false;
        uint64_t row = 0;
        if (pos < p1) {
            const uint32_t slot = ivf_slot(pq, nprobe, pos);
            mine = cnt[lq[slot]] < kIvffTileMin;  // (a position exists: its list is real)
            row = (uint64_t)sq[slot] + (pos - pq[slot]);
        }
        if (!__syncthreads_or(mine)) continue;  // (uniform)
        const uint8_t *r = C + row * d;
        float acc = -0.0f;
        for (uint32_t t0 = 0; t0 < d; t0 += kIvffQC) {
            const uint32_t tc = min(kIvffQC, d - t0);
            if (!once) {
                __syncthreads();
                for (uint32_t t = tid; t < tc; t += 256) s_x[t] = x[t0 + t];
                __syncthreads();
            }
            if (!mine) continue;
            sq_row_walk<W4>(r + t0, tc, mn, step, [&](uint32_t t, float v) { acc = knn_step<METRIC>(acc, s_x[t], v); });
        }
        if (mine) {
            const float dv = knn_finish<METRIC>(acc, qn, vq_is_cos(METRIC) ? rnorm[row] : 1.0f);
            const uint32_t key = adc_key(dv);
            if (key != 0xFFFFFFFFu) {
                lo = min(lo, key);
                hi = max(hi, key);
            }
            wq[pos] = dv;
        }
    }
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, (int)o));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, (int)o));
    }
    if ((tid & 63u) == 0 && lo <= hi) {
        atomicMin(&kmin[q], lo);
        atomicMax(&kmax[q], hi);
    }
}

// METRIC as a template argument of F (a generic lambda called with a tag)
template <class F>
int ivfsq_dispatch(int metric, F &&f) {
    switch (metric) {
        case VQHIP_SQUARED_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_SQUARED_EUCLIDEAN>());
        case VQHIP_EUCLIDEAN: return f(std::integral_constant<int, VQHIP_EUCLIDEAN>());
        case VQHIP_MANHATTAN: return f(std::integral_constant<int, VQHIP_MANHATTAN>());
        case VQHIP_COSINE: return f(std::integral_constant<int, VQHIP_COSINE>());
        case VQHIP_COSINE_UNCLAMPED: return f(std::integral_constant<int, VQHIP_COSINE_UNCLAMPED>());
    }
    return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
}

}  // namespace

// the two distance passes of a batch behind its plan: every D(q, i) of the probed lists into W, the key range into p
static int ivfsq_distances(const IvffPlan &p, int metric, const uint8_t *C, uint32_t d, float mn, float step, const float *rnorm,
                           const uint32_t *off, uint32_t nlist, const float *queries, const float *qnorm, const uint32_t *probe,
                           uint32_t nb, uint32_t nprobe, uint32_t chunk, uint64_t wstride, float *W, const uint32_t *pref,
                           const uint32_t *seg, const uint32_t *inv, hipStream_t stream) {
    const uint64_t items = (wstride + chunk - 1) / chunk;
    const int lw = sq_load_width(C, d);
    return ivfsq_dispatch(metric, [&](auto mtag) -> int {
        constexpr int M = decltype(mtag)::value;
        if (p.tiles_max > 0) {
            const dim3 grid((uint32_t)p.tiles_max, (uint32_t)p.cols);
            auto tile = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, queries, C, d, mn, step, qnorm, rnorm, off, nlist, p.cnt, p.lstart,
                                   p.tstart, inv, pref, nprobe, wstride, W, p.kmin, p.kmax);
            };
            if (lw == 16) tile(k_ivfsq_tile<M, 16>);
            else if (lw == 4) tile(k_ivfsq_tile<M, 4>);
            else tile(k_ivfsq_tile<M, 1>);
            VQ_LAUNCH_CHECK("k_ivfsq_tile");
        }
        if (items > 0) {
            auto scan = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3((uint32_t)items, nb), dim3(256), 0, stream, queries, C, d, mn, step, qnorm, rnorm, probe,
                                   p.cnt, pref, seg, nprobe, chunk, wstride, W, p.kmin, p.kmax);
            };
            if (lw >= 4) scan(k_ivfsq_scan<M, true>);
            else scan(k_ivfsq_scan<M, false>);
            VQ_LAUNCH_CHECK("k_ivfsq_scan");
        }
        return VQHIP_OK;
    });
}

// One batch of nb <= 1024 queries (queries [nb][d] f32, qnorm [nb] under the cosines) whose probe lists
// (probe [nb][nprobe], launch_knn_search) are on the device.  C / rnorm / ids / off: the index in list order, C [n][d]
// u8 with v(c) = mn + (float)c * step, rnorm from launch_sq_norms over C.  The workspaces are launch_ivfflat_search's.
// Results [nb][topk] on the device.
int launch_ivfsq_search(int metric, const uint8_t *C, uint32_t d, float mn, float step, const float *rnorm, const uint32_t *ids,
                        const uint32_t *off, uint32_t nlist, uint64_t max_list, const float *queries, const float *qnorm,
                        const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t topk, uint32_t chunk, uint64_t wstride,
                        float *W, uint32_t *pref, uint32_t *seg, uint32_t *inv, uint32_t *lists, void *state,
                        unsigned long long *cand, uint32_t *idx_out, float *dist_out, hipStream_t stream) {
    if (nb == 0) return VQHIP_OK;
    IvffPlan p;
    VQ_TRY(launch_ivff_plan(off, nlist, max_list, probe, nb, nprobe, topk, pref, seg, inv, lists, state, &p, stream));
    VQ_TRY(ivfsq_distances(p, metric, C, d, mn, step, rnorm, off, nlist, queries, qnorm, probe, nb, nprobe, chunk, wstride, W, pref, seg,
                           inv, stream));
    return launch_ivff_select(p, W, wstride, pref, seg, ids, nb, nprobe, topk, cand, idx_out, dist_out, stream);
}

// launch_ivfsq_search's batch with the range stage behind the distances (launch_ivff_range, k_ivfflat.hip): the arguments
// of launch_ivfflat_range with the rows as SQ codes.
int launch_ivfsq_range(int metric, const uint8_t *C, uint32_t d, float mn, float step, const float *rnorm, const uint32_t *ids, uint64_t n,
                       const uint32_t *off, uint32_t nlist, uint64_t max_list, const float *queries, const float *qnorm,
                       const uint32_t *probe, uint32_t nb, uint32_t nprobe, uint32_t chunk, uint64_t wstride, float *W, uint32_t *pref,
                       uint32_t *seg, uint32_t *inv, uint32_t *lists, void *state, uint32_t q0, const float *radii, void *range_ws,
                       DevBuf *stage, uint64_t max_results, RangeOut *out, hipStream_t stream) {
    if (nb == 0) return VQHIP_OK;
    IvffPlan p;
    VQ_TRY(launch_ivff_plan(off, nlist, max_list, probe, nb, nprobe, 1, pref, seg, inv, lists, state, &p, stream));
    VQ_TRY(ivfsq_distances(p, metric, C, d, mn, step, rnorm, off, nlist, queries, qnorm, probe, nb, nprobe, chunk, wstride, W, pref, seg,
                           inv, stream));
    return launch_ivff_range(W, wstride, pref, seg, ids, n, nb, nprobe, q0, radii, range_ws, stage, max_results, out, stream);
}

}  // namespace vqhip
