// k_ivf_remove.hip -- removing rows from an inverted file on the device (include/vqhip.h, "removing rows from an inverted
// file").  The view of the surviving rows (launch_ivf_view: pick / aids / aoff) is their inverted
// file with the old ids; two kernels make it the index's own state --
//   k_ivf_take      row j of dst is row pick[j] of src, j < na: the destination is one run of na * upr units of 16, 4 or 1
//                   bytes (compact.hpp), a workgroup takes kIvfTakeBlock consecutive units, a wave's store is 64
//                   consecutive units; pick ascends, so the loads are runs of whole rows.  Once for the payload and once
//                   with rb = 4 for the rows' norms.
//   k_ivf_renumber  ids[j] = aids[j] - below(aids[j]): the exclusive prefix popcount of the remove mask per word (from the
//                   host) plus one masked popcount (ivf_remove.hpp).  The remove mask is the complement of the view's.
// No atomics: the same call gives the same bytes on every run.  Out of place: src and dst never overlap.
#include "ivf_remove.hpp"
#include "kernels.hpp"

namespace vqhip {
namespace {

// U: the unit (uint4, uint32_t or uint8_t); rb is a multiple of sizeof(U) and src and dst are aligned to it.  units =
// na * upr; block0: the first workgroup of this launch (a grid is at most 2^31 - 1 workgroups).
template <class U>
__global__ __launch_bounds__(kIvfTakeThreads) void k_ivf_take(const uint32_t *__restrict__ pick, uint64_t units, uint64_t upr, uint64_t rb,
                                                              uint64_t block0, const U *__restrict__ src, U *__restrict__ dst) {
#pragma unroll
    for (uint32_t s = 0; s < kIvfTakePasses; ++s) {
        const uint64_t u = ivf_take_unit(block0 + blockIdx.x, s, threadIdx.x);
        if (u >= units) return;  // (later passes lie further on)
        uint32_t j;
        uint64_t within;
        ivf_take_row(u, upr, &j, &within);  // (j < na: u < na * upr)
        dst[ivf_take_dst_offset(u, (uint32_t)sizeof(U)) / sizeof(U)] =
            src[ivf_take_src_offset(pick[j], rb, within, (uint32_t)sizeof(U)) / sizeof(U)];
    }
}

template <class U>
int take_launch(const uint32_t *pick, uint64_t na, const void *src, void *dst, uint64_t rb, hipStream_t stream) {
    const uint64_t upr = compact_units_per_row(rb, (uint32_t)sizeof(U)), units = na * upr;
    const uint64_t blocks = ivf_take_blocks(units), per = 1ull << 30;
    for (uint64_t b0 = 0; b0 < blocks; b0 += per) {
        hipLaunchKernelGGL(k_ivf_take<U>, dim3((uint32_t)std::min(per, blocks - b0)), dim3(kIvfTakeThreads), 0, stream, pick, units, upr,
                           rb, b0, static_cast<const U *>(src), static_cast<U *>(dst));
        VQ_LAUNCH_CHECK("k_ivf_take");
    }
    return VQHIP_OK;
}

// allowed: the view's mask (bit set: the row stays), so word w of the remove mask is ~allowed[w]; an id is below n and
// only the bits under it are counted
__global__ __launch_bounds__(256) void k_ivf_renumber(const uint32_t *__restrict__ aids, uint32_t na, const uint32_t *__restrict__ allowed,
                                                      const uint32_t *__restrict__ prefix, uint32_t *__restrict__ ids) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= na) return;
    const uint32_t i = aids[j], w = i >> 5;
    ids[j] = ivf_new_id(prefix[w], ~allowed[w], i);
}

}  // namespace

int launch_ivf_take(const uint32_t *pick, uint64_t na, const void *src, void *dst, uint64_t rb, hipStream_t stream) {
    if (na == 0 || rb == 0) return VQHIP_OK;
    switch (compact_unit(rb, reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst))) {
        case 16: return take_launch<uint4>(pick, na, src, dst, rb, stream);
        case 4: return take_launch<uint32_t>(pick, na, src, dst, rb, stream);
        default: return take_launch<uint8_t>(pick, na, src, dst, rb, stream);
    }
}

int launch_ivf_renumber(const uint32_t *aids, uint64_t na, const uint32_t *allowed, const uint32_t *prefix, uint32_t *ids,
                        hipStream_t stream) {
    if (na == 0) return VQHIP_OK;
    hipLaunchKernelGGL(k_ivf_renumber, dim3((uint32_t)((na + 255) / 256)), dim3(256), 0, stream, aids, (uint32_t)na, allowed, prefix, ids);
    VQ_LAUNCH_CHECK("k_ivf_renumber");
    return VQHIP_OK;
}

}  // namespace vqhip
