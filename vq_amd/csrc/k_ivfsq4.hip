// Inverted-file search over 4-bit SQ codes (include/vqhip.h, vqhip_ivfsq4_*): k_ivfsq.hip's search
// with the row side read as one u32 word per eight dimensions and decoded where it leaves global memory, as
// k_sq4index.hip decodes it:
//   v(c)    = mn + (float)c * step for every nibble value c = 0 .. 15 (nibble_decode.hpp: two roundings, never fused),
//   D(q, i) = the flat index's distance over the decoded row (knn_tile.hpp: knn_step from -0.0 over ascending
//             dimensions, knn_finish), so every result equals IVFScalarIndex over the unpacked codes and IVFFlatIndex
//             over the dequantized rows in the same lists.
// The index keeps its words in list order: list l is the run P[off[l] * W .. off[l + 1] * W) of one buffer the index
// owns, W = ceil(d / 8) words a row, so every row of every list starts on a 4-byte boundary -- all NibbleRows asks for.
// Schedule of one batch: section 14's, step for step, with launch_ivfsq4_distances as its distance passes --
//   launch_ivff_plan    k_ivff_plan, k_ivff_lists, k_ivff_invert (k_ivfflat.hip): pref / seg, cnt, the inverted probe table
//   ivff_distances      k_ivff_tile and k_ivff_scan (ivf_tile.hpp) instantiated with the row source NibbleRows
//                       (nibble_decode.hpp), which is its own Walk: the tile's chunk of 32 dimensions is four words of a
//                       row, one per lane (nib_fill_lane); the scan walks a row a word at a time from chunks that start
//                       at multiples of kIvffQC = 1024, a multiple of 8 as NibbleRows::walk requires
//   launch_ivff_select  k_ivff_hist and the selection stage over IvffSource (k_ivfflat.hip)
// Which kernel computes a pair depends on the batch; both run one pair's operations in one order, so the bits do not.
// Row numbers into nib_word_offset are 64-bit on both paths: (uint64_t)row0 + r of a list, (uint64_t)pick[j] of a view.
// A range search puts the range stage (launch_ivff_range) behind the same plan and distance
// passes.
// A filtered call runs the same passes over the view of its allowed rows: v.pick set, the kernels
// instantiated over PickedRows<NibbleRows> (ivf_tile.hpp).  The four waves of a fill hold the four words of the same 64
// tile rows, so they read the same 64 entries of pick.
#include "common.hpp"
#include "ivf_tile.hpp"
#include "kernels.hpp"
#include "nibble_decode.hpp"

#pragma clang fp contract(off)

namespace vqhip {

static_assert(kIvffQC % kNibWordDims == 0, "the scan kernel's chunks of the query must start on a word of NibbleRows::walk");

// The distance passes of a batch (kernels.hpp): ivff_distances over the row source NibbleRows.
int launch_ivfsq4_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint32_t *words, uint32_t d, float mn, float step,
                            const float *rnorm, const float *queries, const float *qnorm, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    return ivff_distances(p, v, metric, NibbleRows{words, d, {mn, step}}, rnorm, queries, qnorm, stream);
}

}  // namespace vqhip
