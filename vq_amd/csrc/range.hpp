// range.hpp -- the exact range stage behind vqhip_flat_range_search (k_knn.hip), vqhip_sqindex_range_search
// (k_sqindex.hip) and, with a sort behind it, the inverted-file range searches (ivf_range.hpp): a deterministic threshold
// compaction over the f32 distances a batch's distance kernels left -- dense [nb][n], or the ragged W[q][0 .. |S(q)|) of the
// inverted files -- with a variable-length result.  The two passes exist once, over a position source (RangeRows below).
// Every including file gets its own copy of the kernels (an anonymous namespace: no relocatable device code).  Semantics
// (include/vqhip.h): position i is a hit of query q iff i < count(q) and dist[q][i] <= radii[q] as an f32 comparison (NaN
// never hits, -0.0 <= 0.0 holds); the hits of a query come out in ascending position.
//   k_range_count   grid (ceil(stride / 4096), nb): the hits among a block's 4096 positions -> cnt[q][blk].  Ballots and a
//                   sum of four wave counts through LDS: no atomics; a block past a ragged query's positions writes 0
//   k_range_scan    one workgroup: the exclusive scan of cnt in query-major order -> off[q][blk] (u64, from the batch's
//                   first hit), the batch's end of every query into lims, the batch total
//   (host)          reads the batch total (8 bytes, one stream wait), holds it against max_results and grows the result
//                   buffers where they are too small (geometrically, device-to-device copy of what is there)
//   k_range_fill    the count's grid: a block with hits recomputes the predicate and every lane writes its hits, (id of the
//                   position, distance), at off[q][blk] + (hits of the block in front of it) behind the batch's first hit
// Positions of a block per lane: the block is four strides of 1024 positions, and in a stride lane t owns the four
// consecutive positions 4 t .. 4 t + 3 (one float4 where stride % 4 == 0: then q * stride + position is a multiple of 4 and
// a float4 is whole or outside).  Ascending position is therefore the order (stride, wave, lane, element), and the rank of
// a hit in its block is
//   the hits of earlier strides and of earlier waves of its stride (16 wave totals through LDS)
//   + the hits of lower lanes of its wave in the stride (four ballots, masked below the lane)
//   + the lane's own earlier elements.
// Both passes read the distances once, the traffic of k_knn_hist + k_adc_collect; the fill skips a block without hits
// before it reads anything.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "topk.hpp"

#include <algorithm>

namespace vqhip {
namespace {

constexpr uint32_t kRangeThreads = 256;                               // four waves
constexpr uint32_t kRangeStrides = 4;                                 // strides of kRangeThreads * 4 rows
constexpr uint32_t kRangeRows = kRangeThreads * 4 * kRangeStrides;  // rows per workgroup: 4096, 16 per lane
// hits the result buffers hold at first; they double (at least) from there.  Small on purpose: 8 KB serve the common
// call of a few hits per query, and tests/test_gpu_range.py reaches two growths with a few thousand hits.
constexpr uint64_t kRangeInitCap = 1024;

// What the two passes read, as the kernels' arguments: dist [nb][stride] f32, and for a ragged source (IvffRows,
// ivf_plan.hpp) the batch's plan and the index's row ids.  The source SRC is built from them inside the kernel
// (SRC::rows) and says, for the opened query: where its distances start (row()), how many positions count (count(); the
// positions from there to `stride` are read but never hit) and the id of a position (id()).  SRC::kRagged: count() may be
// below `stride`; the dense source (TopkRows, topk.hpp) has count() == stride and pays for no bound per element.
struct RangeRows {
    const float *dist;
    uint64_t stride;
    const uint32_t *pref = nullptr, *seg = nullptr, *ids = nullptr;
    uint32_t nprobe = 0;
};

// the four positions r0 .. r0 + 3 of a query's distances dq[0 .. n): v, and bit j of the result set where position
// r0 + j is a hit.  VEC: stride % 4 == 0 and r0 % 4 == 0, so q * stride + r0 is a multiple of 4 and a float4 at r0 < n
// lies inside the query's row; RAGGED: n may be anything up to the stride, and what lies behind it is an earlier batch's
template <bool VEC, bool RAGGED>
__device__ __forceinline__ uint32_t range_load(const float *__restrict__ dq, uint64_t n, uint64_t r0, float rad, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0f;
    uint32_t hits = 0;
    if constexpr (VEC) {
        if (r0 < n) {
            const float4 a = *reinterpret_cast<const float4 *>(dq + r0);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) hits |= (((!RAGGED || r0 + j < n) && v[j] <= rad) ? 1u : 0u) << j;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (r0 + j < n) {
                v[j] = dq[r0 + j];
                hits |= (v[j] <= rad ? 1u : 0u) << j;
            }
    }
    return hits;
}

// range_load for the source SRC: under a row mask (MaskedRows, topk.hpp) the four positions' mask bits come first, a
// group without an allowed position is not loaded, and a disallowed position never hits, whatever its slot holds
template <bool VEC, class SRC>
__device__ __forceinline__ uint32_t range_hits(const SRC &src, const float *__restrict__ dq, uint64_t n, uint64_t r0, float rad,
                                               float (&v)[4]) {
    if constexpr (topk_masked<SRC>::value) {
        const uint32_t ok = r0 < n ? src.allowed4(r0) : 0u;
        if (ok == 0) {
            v[0] = v[1] = v[2] = v[3] = 0.0f;
            return 0;
        }
        return range_load<VEC, SRC::kRagged>(dq, n, r0, rad, v) & ok;
    } else {
        return range_load<VEC, SRC::kRagged>(dq, n, r0, rad, v);
    }
}

template <bool VEC, class SRC>
__global__ __launch_bounds__(kRangeThreads) void k_range_count(const float *__restrict__ dist, uint64_t stride,
                                                               const uint32_t *__restrict__ pref, const uint32_t *__restrict__ seg,
                                                               const uint32_t *__restrict__ ids, uint32_t nprobe,
                                                               const float *__restrict__ radii, uint32_t nblk,
                                                               uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[kRangeThreads / 64];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    SRC src = SRC::rows(dist, stride, pref, seg, ids, nprobe);
    src.open(q);
    const uint64_t n = src.count(), row0 = (uint64_t)blockIdx.x * kRangeRows;
    if constexpr (SRC::kRagged)
        if (row0 >= n) {  // (uniform) past the query's positions
            if (tid == 0) cnt[(size_t)q * nblk + blockIdx.x] = 0u;
            return;
        }
    const float rad = radii[q];
    const float *dq = src.row();
    uint32_t c = 0;  // the wave's hits (uniform)
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        float v[4];
        const uint32_t hits = range_hits<VEC>(src, dq, n, row0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4, rad, v);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) c += (uint32_t)__popcll(__ballot((hits >> j) & 1u));
    }
    if ((tid & 63u) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) cnt[(size_t)q * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Exclusive scan of cnt[0 .. nb * nblk) by one workgroup, 1024 entries at a time with a running carry.  That is enough:
// knn_query_batch keeps nb * n <= 2^28 whenever nb > 1, so a batch of several queries has at most
// nb * ceil(n / 4096) <= 2^16 + nb entries (66 passes), and a single-query batch over n < 2^32 rows has at most 2^20
// (1024 passes of two barriers each, beside a distance pass over 2^32 rows).
// off[e]: the hits in front of entry e, from the batch's first; lims[q] = base + the hits up to the end of query q of the
// batch (the caller passes the result's lims at the batch's first query + 1); *total = the batch's hits.
__attribute__((unused)) __global__ __launch_bounds__(1024) void k_range_scan(const uint32_t *__restrict__ cnt, uint32_t nb,
                                                                             uint32_t nblk, unsigned long long base,
                                                                             unsigned long long *__restrict__ off,
                                                                             unsigned long long *__restrict__ lims,
                                                                             unsigned long long *__restrict__ total) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t entries = (uint64_t)nb * nblk;
    unsigned long long carry = 0;  // replicated in every thread (uniform updates)
    for (uint64_t e0 = 0; e0 < entries; e0 += 1024) {
        const uint64_t e = e0 + tid;
        const uint32_t c = e < entries ? cnt[e] : 0u;
        uint32_t x = c;  // inclusive scan within the wave: at most 64 * 4096
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        unsigned long long before = carry, chunk = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wv) before += wsum[w];
            chunk += wsum[w];
        }
        if (e < entries) {
            off[e] = before + x - c;
            if ((e + 1) % nblk == 0) lims[e / nblk] = base + before + x;
        }
        carry += chunk;
        __syncthreads();  // wsum is rewritten by the next pass
    }
    if (tid == 0) *total = carry;
}

// slot = off[q][blk] + the block's hits in front, counted from the batch's first hit: idx_out / dist_out point at it (the
// result at out->total, or a staging area of the batch)
template <bool VEC, class SRC>
__global__ __launch_bounds__(kRangeThreads) void k_range_fill(const float *__restrict__ dist, uint64_t stride,
                                                              const uint32_t *__restrict__ pref, const uint32_t *__restrict__ seg,
                                                              const uint32_t *__restrict__ ids, uint32_t nprobe,
                                                              const float *__restrict__ radii, uint32_t nblk,
                                                              const uint32_t *__restrict__ cnt,
                                                              const unsigned long long *__restrict__ off,
                                                              uint32_t *__restrict__ idx_out, float *__restrict__ dist_out) {
    __shared__ uint32_t wsum[kRangeStrides][kRangeThreads / 64];
    const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const size_t entry = (size_t)q * nblk + blockIdx.x;
    if (cnt[entry] == 0) return;  // (uniform) nothing to write: the distances are not read again
    SRC src = SRC::rows(dist, stride, pref, seg, ids, nprobe);
    src.open(q);
    const uint64_t n = src.count();
    const float rad = radii[q];
    const float *dq = src.row();
    const uint64_t row0 = (uint64_t)blockIdx.x * kRangeRows;
    const unsigned long long below = (1ull << lane) - 1ull;
    float v[kRangeStrides][4];
    uint32_t hits[kRangeStrides], pre[kRangeStrides];  // pre: the stride's hits in lower lanes of this wave
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        hits[s] = range_hits<VEC>(src, dq, n, row0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4, rad, v[s]);
        uint32_t p = 0, t = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const unsigned long long m = __ballot((hits[s] >> j) & 1u);
            p += (uint32_t)__popcll(m & below);
            t += (uint32_t)__popcll(m);
        }
        pre[s] = p;
        if (lane == 0) wsum[s][wv] = t;
    }
    __syncthreads();
    const unsigned long long at = off[entry];  // the block's first slot: 64-bit throughout
    uint32_t run = 0;                          // the block's hits in front of (stride s, wave w), in position order
#pragma unroll
    for (uint32_t s = 0; s < kRangeStrides; ++s) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t w = 0; w < kRangeThreads / 64; ++w) {
            if (w == wv) mine = run;
            run += wsum[s][w];
        }
        unsigned long long slot = at + mine + pre[s];
        const uint64_t r0 = row0 + (uint64_t)s * (kRangeThreads * 4) + tid * 4;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if ((hits[s] >> j) & 1u) {  // (a hit is below count())
                idx_out[slot] = src.id((typename SRC::Pos)(r0 + j));
                dist_out[slot] = v[s][j];
                ++slot;
            }
    }
}

// The stage's workspace for batches of up to qb queries of nblk count entries each: total | off [qb][nblk] u64 | cnt
// [qb][nblk] u32 (the entries of the dense and the ragged form are blocks of kRangeRows positions)
struct RangeWs {
    unsigned long long *total, *off;
    uint32_t *cnt;
};
inline size_t range_ws_entries(size_t entries) { return 16 + entries * 12; }
inline RangeWs range_ws(void *ws, uint32_t qb, uint32_t nblk) {
    unsigned long long *total = reinterpret_cast<unsigned long long *>(ws);
    return {total, total + 2, reinterpret_cast<uint32_t *>(total + 2 + (size_t)qb * nblk)};
}
inline uint32_t range_blocks(uint64_t n) { return (uint32_t)((n + kRangeRows - 1) / kRangeRows); }
inline size_t range_ws_size(uint64_t n, uint32_t qb) { return range_ws_entries((size_t)qb * range_blocks(n)); }

// the first lines of a range driver: an empty result for nq queries (lims[0] = 0, room for min(kRangeInitCap, max_results))
inline int range_begin(RangeOut *out, uint32_t nq, uint64_t max_results, hipStream_t stream) {
    out->nq = nq;
    out->total = 0;
    out->cap = std::min<uint64_t>(kRangeInitCap, max_results);
    VQ_TRY(out->lims.alloc(((size_t)nq + 1) * 8));
    VQ_TRY(out->idx.alloc((size_t)out->cap * 4));
    VQ_TRY(out->dist.alloc((size_t)out->cap * 4));
    VQ_HIP(hipMemsetAsync(out->lims.p, 0, 8, stream));
    return VQHIP_OK;
}

// room for `need` hits: at least twice the old room (never past max_results), what is there copied device to device
inline int range_grow(RangeOut *out, uint64_t need, uint64_t max_results, hipStream_t stream) {
    if (need <= out->cap) return VQHIP_OK;
    const uint64_t cap = std::max<uint64_t>(need, std::min<uint64_t>(out->cap * 2, max_results));
    DevBuf idx, dist;
    VQ_TRY(idx.alloc((size_t)cap * 4));
    VQ_TRY(dist.alloc((size_t)cap * 4));
    if (out->total) {
        VQ_HIP(hipMemcpyAsync(idx.p, out->idx.p, (size_t)out->total * 4, hipMemcpyDeviceToDevice, stream));
        VQ_HIP(hipMemcpyAsync(dist.p, out->dist.p, (size_t)out->total * 4, hipMemcpyDeviceToDevice, stream));
        VQ_HIP(hipStreamSynchronize(stream));  // the old buffers are freed below
    }
    std::swap(out->idx.p, idx.p), std::swap(out->idx.bytes, idx.bytes);
    std::swap(out->dist.p, dist.p), std::swap(out->dist.bytes, dist.bytes);
    out->cap = cap;
    return VQHIP_OK;
}

// The steps between a batch's count and its fill: k_range_scan over the nb * nblk counts of w (queries q0 .. q0 + nb of
// the result), then the host reads the batch total (8 bytes, one stream wait) into *got, holds the result with it against
// max_results (past it: VQHIP_ERR_UNSUPPORTED) and makes room for it.  out->total is the caller's to advance once the
// batch's hits are written.
inline int range_scan_room(const RangeWs &w, uint32_t nb, uint32_t nblk, uint32_t q0, uint64_t max_results, RangeOut *out, uint64_t *got,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(1024), 0, stream, w.cnt, nb, nblk, (unsigned long long)out->total, w.off,
                       out->lims.as<unsigned long long>() + q0 + 1, w.total);
    VQ_LAUNCH_CHECK("k_range_scan");
    unsigned long long g = 0;
    VQ_HIP(hipMemcpyAsync(&g, w.total, 8, hipMemcpyDeviceToHost, stream));
    VQ_HIP(hipStreamSynchronize(stream));
    *got = g;
    const uint64_t need = out->total + g;
    if (need > max_results)
        return fail(VQHIP_ERR_UNSUPPORTED, "range search reached %llu hits after %u of %u queries: more than max_results = %llu",
                    (unsigned long long)need, q0 + nb, out->nq, (unsigned long long)max_results);
    return g ? range_grow(out, need, max_results, stream) : VQHIP_OK;
}

// f(std::true_type or std::false_type): whether the passes read a float4 per lane and stride (stride % 4 == 0)
template <class F>
int range_vec(uint64_t stride, F &&f) {
    return (stride & 3u) == 0 ? f(std::true_type()) : f(std::false_type());
}

// The passes over one batch of nb queries (q0 the batch's first query in the result) whose distances `in` describes
// (queued on `stream`): count, scan, room, and -- where the batch has hits, *got of them -- the fill into the place
// target(got, &idx, &dist) names for the batch's first hit.  radii [nb] on the device, ws >= range_ws_entries(nb *
// range_blocks(in.stride)).  Waits for the stream once.  out->total is the caller's to advance.
template <class SRC, class TARGET>
int range_passes(const RangeRows &in, uint32_t nb, uint32_t q0, const float *radii, void *ws, uint64_t max_results, RangeOut *out,
                 uint64_t *got, hipStream_t stream, TARGET &&target) {
    const uint32_t nblk = range_blocks(in.stride);
    const RangeWs w = range_ws(ws, nb, nblk);
    const dim3 grid(nblk, nb), block(kRangeThreads);
    return range_vec(in.stride, [&](auto vec) -> int {
        constexpr bool VEC = decltype(vec)::value;
        hipLaunchKernelGGL((k_range_count<VEC, SRC>), grid, block, 0, stream, in.dist, in.stride, in.pref, in.seg, in.ids, in.nprobe, radii,
                           nblk, w.cnt);
        VQ_LAUNCH_CHECK("k_range_count");
        VQ_TRY(range_scan_room(w, nb, nblk, q0, max_results, out, got, stream));
        if (*got == 0) return VQHIP_OK;
        uint32_t *idx = nullptr;
        float *dist = nullptr;
        VQ_TRY(target(*got, &idx, &dist));
        hipLaunchKernelGGL((k_range_fill<VEC, SRC>), grid, block, 0, stream, in.dist, in.stride, in.pref, in.seg, in.ids, in.nprobe, radii,
                           nblk, w.cnt, w.off, idx, dist);
        VQ_LAUNCH_CHECK("k_range_fill");
        return VQHIP_OK;
    });
}

// The stage over one batch of dense distances: dist [nb][n] on the device (queued on `stream`), radii [nb] on the
// device, ws >= range_ws_size(n, nb), q0 the batch's first query in the result.  Waits for the stream once.  A batch that
// takes the result past max_results is VQHIP_ERR_UNSUPPORTED.  mask: the row mask of a filtered call on the device
// (ceil(n / 32) words), NULL for every row.
inline int range_batch(const float *dist, uint64_t n, uint32_t nb, uint32_t q0, const float *radii, void *ws, uint64_t max_results,
                       RangeOut *out, hipStream_t stream, const uint32_t *mask = nullptr) {
    uint64_t got = 0;
    auto target = [&](uint64_t, uint32_t **idx, float **d) {
        *idx = out->idx.as<uint32_t>() + out->total;  // (the result's buffers as range_scan_room left them)
        *d = out->dist.as<float>() + out->total;
        return VQHIP_OK;
    };
    if (mask) VQ_TRY(range_passes<MaskedRows>({dist, n, nullptr, nullptr, mask, 0}, nb, q0, radii, ws, max_results, out, &got, stream, target));
    else VQ_TRY(range_passes<TopkRows>({dist, n}, nb, q0, radii, ws, max_results, out, &got, stream, target));
    out->total += got;
    return VQHIP_OK;
}

}  // namespace
}  // namespace vqhip
