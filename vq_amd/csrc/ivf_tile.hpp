// ivf_tile.hpp -- the two distance passes of the inverted-file searches over rows (k_ivfflat.hip), SQ codes (k_ivfsq.hip)
// and, for the work item of a tile and its write-back, packed bits (k_ivfbin.hip); DESIGN.md section 14.  A list probed by
// at least kIvffTileMin queries of the batch goes through the tile kernel, the others through the scan kernel
// (ivf_plan.hpp); both run one pair's operations in one order (knn_tile.hpp), so the bits do not depend on which.
//   ivf_tile_open    the work item of a tile kernel's block: its list and the up to 128 queries of its tile
//   ivf_tile_store   the write-back of one row tile: every D into W[q][pref[q][slot] + r], the key range per lane
//   k_ivff_tile      knn_tile_pass over the rows of one list, the queries gathered through inv
//   k_ivff_scan      one query x one chunk of its positions, the query in LDS, one position per lane
//   PickedRows       a row source behind the view of a filtered call (ivf_view.hpp): row j of it is row pick[j] of X
//   ivff_distances   the host side of the two, templated on the row source as the kernels are
// Every including file gets its own copy (an anonymous namespace); each .hip instantiates what it launches.
#pragma once
#include "common.hpp"
#include "ivf_plan.hpp"
#include "kernels.hpp"
#include "knn_tile.hpp"

#pragma clang fp contract(off)

namespace vqhip {
namespace {

// The picked form of a row source ROWS, for the view of a filtered call (ivf_view.hpp): row j of the
// source is row pick[j] of X, and a list of the view is the run aoff[l] .. aoff[l + 1] of pick.  It holds no loader of its
// own: fill is ROWS::fill_rows with pick[row0 + r] as tile row r (a row's 32 dimensions of a chunk are still read by
// consecutive lanes), walk is ROWS::walk of row pick[row], and row(j), the index of a row's norm, is pick[j].  Row offsets
// stay 64-bit: (uint64_t)pick[j] * d.  The alignment conditions of ROWS rest on d and the base of X, so they hold for
// any row.  pick travels in Scale, so the kernels' parameter lists are those of the unpicked instantiations.
template <class S>
struct PickedScale {  // (one type per Scale: a source and its Walk share it)
    S sc;
    const uint32_t *pick;
};
template <class ROWS>
struct PickedRows {
    using Elem = typename ROWS::Elem;
    using Walk = PickedRows<typename ROWS::Walk>;
    using Scale = PickedScale<typename ROWS::Scale>;
    const Elem *X;
    uint32_t d;
    Scale sc;

    __device__ __forceinline__ void fill(float (&rs)[kKnnKC][kKnnTR + 4], uint64_t row0, uint32_t nvalid, uint32_t t0,
                                         uint32_t tc) const {
        const uint32_t *__restrict__ p = sc.pick + row0;
        ROWS{X, d, sc.sc}.fill_rows(rs, [&](uint32_t r) { return (uint64_t)p[r]; }, nvalid, t0, tc);
    }
    template <class F>
    __device__ __forceinline__ void walk(uint64_t row, uint32_t t0, uint32_t tc, bool vec, F &&f) const {
        ROWS{X, d, sc.sc}.walk((uint64_t)sc.pick[row], t0, tc, vec, f);
    }
    __device__ __forceinline__ uint64_t row(uint64_t j) const { return sc.pick[j]; }
};

// The work item of block x of a tile kernel: *row0 / *nrows the run of its list (the last list whose first tile is <=
// the block's, and that has tiles: tstart is non-decreasing), s_q the tile's queries (kKnnNone: none) and s_p the first
// position of the list in each; the caller synchronizes before it reads them.  false for the blocks past the last tile
// (uniform), which leave at once.
__device__ __forceinline__ bool ivf_tile_open(const uint32_t *__restrict__ off, uint32_t nlist, const uint32_t *__restrict__ cnt,
                                              const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ tstart,
                                              const uint32_t *__restrict__ inv, const uint32_t *__restrict__ pref, uint32_t nprobe,
                                              uint32_t (&s_q)[kKnnTQ], uint32_t (&s_p)[kKnnTQ], uint32_t *row0, uint32_t *nrows) {
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= tstart[nlist]) return false;
    uint32_t l = 0, hi = nlist;
    while (hi - l > 1) {
        const uint32_t mid = (l + hi) >> 1;
        if (tstart[mid] <= tile) l = mid;
        else hi = mid;
    }
    const uint32_t e0 = (tile - tstart[l]) * kKnnTQ, en = min(kKnnTQ, cnt[l] - e0);
    *row0 = off[l];
    *nrows = off[l + 1] - off[l];
    if (tid < kKnnTQ) {
        uint32_t q = kKnnNone, p = 0;
        if (tid < en) {
            const uint32_t e = inv[lstart[l] + e0 + tid];
            q = e / nprobe;
            p = pref[(size_t)q * (nprobe + 1) + (e - q * nprobe)];
        }
        s_q[tid] = q;
        s_p[tid] = p;
    }
    return true;
}

// The write-back of a lane's 8 x 4 pairs of one row tile: dist(a, b) of query qi[a] and row rb + b of the list goes to
// W[qi[a]][s_p + rb + b] (a run starts at any position: no 16-byte stores), its key into lo / hi [a] unless NaN.  Nothing
// is computed or written for a padded query, a row past the list or a position past wstride.
template <class DF>
__device__ __forceinline__ void ivf_tile_store(const uint32_t (&qi)[kKnnRQ], const uint32_t (&s_p)[kKnnTQ], uint32_t rb, uint32_t nrows,
                                               uint64_t wstride, float *__restrict__ W, uint32_t (&lo)[kKnnRQ], uint32_t (&hi)[kKnnRQ],
                                               DF &&dist) {
    const uint32_t qg = threadIdx.x >> 4;
#pragma unroll
    for (uint32_t a = 0; a < kKnnRQ; ++a) {
        if (qi[a] == kKnnNone) continue;
        float *wq = W + (size_t)qi[a] * wstride;
        const uint64_t p0 = (uint64_t)s_p[qg * kKnnRQ + a] + rb;
#pragma unroll
        for (uint32_t b = 0; b < kKnnRR; ++b) {
            if (rb + b >= nrows || p0 + b >= wstride) continue;
            const float dv = dist(a, b);
            const uint32_t key = adc_key(dv);
            if (key != 0xFFFFFFFFu) {
                lo[a] = min(lo[a], key);
                hi[a] = max(hi[a], key);
            }
            wq[p0 + b] = dv;
        }
    }
}

// block (x = query tile of the batch's tstart[nlist] tiles, y = column of row tiles): k_knn_dist's tile pass over the rows
// of one list and the up to 128 queries of one tile of its run of inv.  A row of list l is row off[l] + r of X, so the
// alignment conditions of a row source hold for every list.
template <int METRIC, class ROWS>
__global__ __launch_bounds__(256) void k_ivff_tile(const float *__restrict__ Q, const typename ROWS::Elem *__restrict__ X, uint32_t d,
                                                   typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                                   const float *__restrict__ rnorm, const uint32_t *__restrict__ off, uint32_t nlist,
                                                   const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ lstart,
                                                   const uint32_t *__restrict__ tstart, const uint32_t *__restrict__ inv,
                                                   const uint32_t *__restrict__ pref, uint32_t nprobe, uint64_t wstride,
                                                   float *__restrict__ W, uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, KC = kKnnKC;
    __shared__ __attribute__((aligned(16))) float qs[KC][TQ + 4];
    __shared__ __attribute__((aligned(16))) float rs[KC][TR + 4];
    __shared__ uint32_t s_q[TQ], s_p[TQ];
    uint32_t row0, nrows;
    if (!ivf_tile_open(off, nlist, cnt, lstart, tstart, inv, pref, nprobe, s_q, s_p, &row0, &nrows)) return;
    __syncthreads();
    const ROWS rows{X, d, sc};
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4;
    float qn[RQ];
    uint32_t lo[RQ], hi[RQ], qi[RQ];
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
        qi[a] = s_q[qg * RQ + a];
        qn[a] = (vq_is_cos(METRIC) && qi[a] != kKnnNone) ? qnorm[qi[a]] : 1.0f;
        lo[a] = 0xFFFFFFFFu;
        hi[a] = 0u;
    }
    const uint32_t nrt = (nrows + TR - 1) / TR;
    for (uint32_t rt = blockIdx.y; rt < nrt; rt += gridDim.y) {
        const uint32_t r0 = rt * TR;  // (within the list)
        float acc[RQ][RR];
        knn_tile_pass<METRIC>(acc, qs, rs, Q, [&](uint32_t slot) { return s_q[slot]; }, rows, (uint64_t)row0 + r0, nrows - r0);
        const uint32_t rb = r0 + rg * RR;
        float rn[RR];
#pragma unroll
        for (uint32_t b = 0; b < RR; ++b) rn[b] = (vq_is_cos(METRIC) && rb + b < nrows) ? rnorm[rows.row((uint64_t)row0 + rb + b)] : 1.0f;
        ivf_tile_store(qi, s_p, rb, nrows, wstride, W, lo, hi,
                       [&](uint32_t a, uint32_t b) { return knn_finish<METRIC>(acc[a][b], qn[a], rn[b]); });
    }
    knn_key_range(lo, hi, [&](uint32_t a) { return qi[a]; }, kmin, kmax);
}

// block (x = chunk of positions, y = query): the positions of the chunk whose list fewer than kIvffTileMin queries probe,
// one per lane and pass; the query's dimensions in LDS, kIvffQC at a time.  Items past |S(q)| leave at once.  Dense rows
// are walked four elements per load when d % 4 == 0.
template <int METRIC, class ROWS>
__global__ __launch_bounds__(256) void k_ivff_scan(const float *__restrict__ Q, const typename ROWS::Elem *__restrict__ X, uint32_t d,
                                                   typename ROWS::Scale sc, const float *__restrict__ qnorm,
                                                   const float *__restrict__ rnorm, const uint32_t *__restrict__ probe,
                                                   const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pref,
                                                   const uint32_t *__restrict__ seg, uint32_t nprobe, uint32_t chunk, uint64_t wstride,
                                                   float *__restrict__ W, uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax) {
    __shared__ __attribute__((aligned(16))) float s_x[kIvffQC];
    const ROWS rows{X, d, sc};
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
    const bool vec = (d & 3u) == 0;  // read by DenseRows::walk alone: SqRows takes its load width from its type
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
        float acc = -0.0f;
        for (uint32_t t0 = 0; t0 < d; t0 += kIvffQC) {
            const uint32_t tc = min(kIvffQC, d - t0);
            if (!once) {
                __syncthreads();
                for (uint32_t t = tid; t < tc; t += 256) s_x[t] = x[t0 + t];
                __syncthreads();
            }
            if (!mine) continue;
            rows.walk(row, t0, tc, vec, [&](uint32_t t, float v) { acc = knn_step<METRIC>(acc, s_x[t - t0], v); });
        }
        if (mine) {
            const float dv = knn_finish<METRIC>(acc, qn, vq_is_cos(METRIC) ? rnorm[rows.row(row)] : 1.0f);
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

// the two distance passes of a batch behind its plan: every D(q, i) of the probed lists into v.W, the key range into p
template <class ROWS>
int ivff_launch(const IvffPlan &p, const IvfBatchView &v, int metric, const ROWS &rows, const float *rnorm, const float *queries,
                   const float *qnorm, hipStream_t stream) {
    const uint64_t items = (v.wstride + v.chunk - 1) / v.chunk;
    return knn_metric_dispatch(metric, [&](auto mtag) -> int {
        constexpr int M = decltype(mtag)::value;
        if (p.tiles_max > 0) {
            hipLaunchKernelGGL((k_ivff_tile<M, ROWS>), dim3((uint32_t)p.tiles_max, (uint32_t)p.cols), dim3(256), 0, stream, queries,
                               rows.X, rows.d, rows.sc, qnorm, rnorm, v.off, v.nlist, p.cnt, p.lstart, p.tstart, v.inv, v.pref, v.nprobe,
                               v.wstride, v.W, p.kmin, p.kmax);
            VQ_LAUNCH_CHECK("k_ivff_tile");
        }
        if (items > 0) {
            hipLaunchKernelGGL((k_ivff_scan<M, typename ROWS::Walk>), dim3((uint32_t)items, v.nb), dim3(256), 0, stream, queries, rows.X,
                               rows.d, rows.sc, qnorm, rnorm, v.probe, p.cnt, v.pref, v.seg, v.nprobe, v.chunk, v.wstride, v.W, p.kmin,
                               p.kmax);
            VQ_LAUNCH_CHECK("k_ivff_scan");
        }
        return VQHIP_OK;
    });
}

// ivff_launch over the rows as they lie (v.pick NULL: the kernels of an unfiltered call, as they are) or over the view
// of a filtered call (PickedRows: v.off and v.ids are the view's, v.pick its positions in X)
template <class ROWS>
int ivff_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const ROWS &rows, const float *rnorm, const float *queries,
                   const float *qnorm, hipStream_t stream) {
    if (v.pick) return ivff_launch(p, v, metric, PickedRows<ROWS>{rows.X, rows.d, {rows.sc, v.pick}}, rnorm, queries, qnorm, stream);
    return ivff_launch(p, v, metric, rows, rnorm, queries, qnorm, stream);
}

}  // namespace
}  // namespace vqhip
