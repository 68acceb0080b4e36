// ivf_plan.hpp -- the per-query plan the inverted-file searches share (k_ivf.hip over PQ codes, k_ivfflat.hip over rows,
// k_ivfsq.hip over SQ codes):
// S(q) as ONE sequence of positions, probe slot 0's list first; pref[q][slot] the first position of a slot, seg[q][slot]
// the first row (in list order) of its list.  Every including file gets its own copy (an anonymous namespace).
#pragma once
#include "common.hpp"

namespace vqhip {
namespace {

// the searches over rows and over SQ codes (k_ivfflat.hip, k_ivfsq.hip) switch per list and batch between two kernels
constexpr uint32_t kIvffTileMin = 16;  // queries of a batch probing a list from which the tile kernel takes it
constexpr uint32_t kIvffQC = 1024;     // query dimensions the scan kernels hold in LDS at a time

// pref[q][0..nprobe] and seg[q][0..nprobe) of the block's query q = blockIdx.x (1024 threads); returns slot t's length
__device__ __forceinline__ uint32_t ivf_plan_prefix(const uint32_t *__restrict__ probe, uint32_t nprobe, uint32_t nlist,
                                                    const uint32_t *__restrict__ off, uint32_t *__restrict__ pref,
                                                    uint32_t *__restrict__ seg) {
    __shared__ uint32_t s_len[1024];
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    uint32_t len = 0;
    if (t < nprobe) {
        const uint32_t l = probe[(size_t)q * nprobe + t];  // (< nlist: the flat search returns real rows; an empty slot else)
        const uint32_t o = l < nlist ? off[l] : 0u;
        len = l < nlist ? off[l + 1] - o : 0u;
        seg[(size_t)q * nprobe + t] = o;
    }
    s_len[t] = len;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive scan
        const uint32_t v = t >= d ? s_len[t - d] : 0u;
        __syncthreads();
        s_len[t] += v;
        __syncthreads();
    }
    uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    if (t < nprobe) pq[t + 1] = s_len[t];
    if (t == 0) pq[0] = 0u;
    return len;
}

// the probe slot of position pos: the last slot whose first position is <= pos (pq[0] = 0 <= pos < pq[nprobe])
__device__ __forceinline__ uint32_t ivf_slot(const uint32_t *__restrict__ pq, uint32_t nprobe, uint32_t pos) {
    uint32_t lo = 0, hi = nprobe;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pq[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the row (in list order) behind position pos of a query
__device__ __forceinline__ uint32_t ivf_row(const uint32_t *__restrict__ pq, const uint32_t *__restrict__ sq, uint32_t nprobe,
                                            uint32_t pos) {
    const uint32_t slot = ivf_slot(pq, nprobe, pos);
    return sq[slot] + (pos - pq[slot]);
}


// The distances the inverted-file distance kernels leave, W[q][0 .. |S(q)|), as a position source of the selection stage
// (topk.hpp; IvffSource, k_ivfflat.hip, adds the key bins) and of the range stage (range.hpp): a query's positions in
// probe-slot order, the id of a position through the plan and the index's ids in list order.
struct IvffRows {
    using Pos = uint32_t;
    static constexpr bool kRagged = true;  // count() <= wstride: what lies behind it is an earlier batch's
    const float *W;
    uint64_t wstride;
    const uint32_t *pref, *seg, *ids;
    uint32_t nprobe;
    uint32_t total = 0;  // (device: of the opened query)
    static __device__ IvffRows rows(const float *W, uint64_t wstride, const uint32_t *pref, const uint32_t *seg, const uint32_t *ids,
                                    uint32_t nprobe) {
        return {W, wstride, pref, seg, ids, nprobe};
    }
    __device__ void open(uint32_t q) {
        W += (size_t)q * wstride;
        pref += (size_t)q * (nprobe + 1);
        seg += (size_t)q * nprobe;
        total = (uint32_t)min((uint64_t)pref[nprobe], wstride);
    }
    __device__ Pos count() const { return total; }
    __device__ const float *row() const { return W; }
    __device__ float at(Pos pos) const { return W[pos]; }
    __device__ uint32_t id(Pos pos) const { return ids[ivf_row(pref, seg, nprobe, pos)]; }
};

}  // namespace
}  // namespace vqhip
