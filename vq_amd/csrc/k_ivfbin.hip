// Inverted-file search over packed BQ bits (include/vqhip.h, vqhip_ivfbin_*): section 14's probe
// and schedule over section 12's codes.  The index keeps its words in list order: list l is the run
// P[off[l] * W .. off[l + 1] * W) of one buffer the index owns (W = ceil(d / 32) words a row, pad bits zero), so a row
// of any list starts on the alignment of the base and of W words.
//   H(q, i) = popcount(bits(q) xor words[i]) over the W words, an integer: no order of operations to keep,
//   D(q, i) = S[H] (binary_table), sqrtf(S[H]) under Euclidean -- the form k_ivff_tile stores for the metric, so the
//             selection stage orders and reports it unchanged; S and its root are strictly increasing, so (D, row id)
//             orders like (H, row id).
// Schedule of one batch: section 14's, step for step, with launch_ivfbin_distances as its distance passes --
//   launch_ivff_plan    k_ivff_plan, k_ivff_lists, k_ivff_invert (k_ivfflat.hip): pref / seg, cnt, the inverted probe table
//   launch_bq_pack      the batch's queries as words Q [nb][W] (k_binary.hip; the caller's, in front of the two passes)
//   k_ivfbin_tile       k_ivff_tile's work item and write-back (ivf_tile_open, ivf_tile_store, knn_key_range) with both sides
//                       as words: an 8 x 4 register block of H over chunks of 32 words in LDS, three 16-byte LDS reads per
//                       64 VALU operations
//   k_ivfbin_scan       the lists probed by fewer than kIvffTileMin queries: one query x one chunk of positions, the
//                       query's words in LDS, one position per lane
//   launch_ivff_select  k_ivff_hist and the selection stage over IvffSource (k_ivfflat.hip)
// Which kernel computes a pair depends on the batch; H is an integer and both look D up in one table, so the bits do not.
// A Hamming-radius range search puts the range stage (launch_ivff_range; DESIGN.md sections 17 and 19) behind the same
// two distance passes, with radii [nb] f32 the reported distance of each query's Hamming radius, so that D <= radius iff
// H <= that radius.
// LW = words per load of the row loader (4, 2 or 1: 16, 8 or 4 bytes), chosen per launch from W and the base pointer.
// A filtered call (DESIGN.md sections 23 and 24) runs the same passes over the view of its allowed rows: v.off and v.ids are
// the view's, and row j of the view is row v.pick[j] of P.  The two kernels take pick as an optional last argument (PICK:
// no type, or const uint32_t *), so the unpicked instantiations are the kernels of an unfiltered call with their
// arguments.  Row offsets stay 64-bit, (uint64_t)pick[j] * W, and the loaders' alignment rests on W and the base of P, so
// it holds for any picked row.  No other stage knows.
#include "common.hpp"
#include "ivf_tile.hpp"
#include "kernels.hpp"

namespace vqhip {
namespace {

constexpr uint32_t kBinWC = 32;  // words (1024 dimensions) per LDS chunk of the tile kernel

// LW consecutive words from p (LW-word aligned)
template <int LW>
__device__ __forceinline__ void bin_load(const uint32_t *__restrict__ p, uint32_t (&w)[LW]) {
    if constexpr (LW == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if constexpr (LW == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        w[0] = v.x, w[1] = v.y;
    } else {
        w[0] = *p;
    }
}

// S [d + 1] into LDS as the reported distance of every H
__device__ __forceinline__ void bin_table_load(float *s_tab, const float *__restrict__ S, uint32_t d, int root) {
    for (uint32_t h = threadIdx.x; h <= d; h += 256) s_tab[h] = root ? sqrtf(S[h]) : S[h];
}

// block (x = query tile of the batch's tstart[nlist] tiles, y = column of row tiles): H of the rows of one list against
// the up to 128 queries of one tile of its run of inv.  Blocks past the last tile leave at once.  A chunk of a row starts
// at word (off[l] + r) * W + t0 with t0 a multiple of 32, so W % LW == 0 and an LW-word-aligned base align every load; a
// load is issued only where its row is inside the list and its first word below tc (a multiple of LW).  Padded rows,
// queries and words are 0 in the tile and never reach a result.
// Picked: row0 is a position of the view, so the rows of a tile are P[pick[row0 + r0 + r]]; the tile's 64 pick words go
// into LDS once per row tile (s_pick), not once per chunk and load.  They are written before the first chunk's opening
// barrier; their last readers, the previous tile's loads, lie before that tile's closing barrier.
template <int LW, class... PICK>
__global__ __launch_bounds__(256) void k_ivfbin_tile(const uint32_t *__restrict__ Q, const uint32_t *__restrict__ P, uint32_t Wn,
                                                     uint32_t d, const float *__restrict__ S, int root,
                                                     const uint32_t *__restrict__ off, uint32_t nlist, const uint32_t *__restrict__ cnt,
                                                     const uint32_t *__restrict__ lstart, const uint32_t *__restrict__ tstart,
                                                     const uint32_t *__restrict__ inv, const uint32_t *__restrict__ pref,
                                                     uint32_t nprobe, uint64_t wstride, float *__restrict__ W,
                                                     uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax, PICK... pick_arg) {
    constexpr uint32_t RQ = kKnnRQ, RR = kKnnRR, TQ = kKnnTQ, TR = kKnnTR, WC = kBinWC;
    constexpr bool PICKED = sizeof...(PICK) == 1;
    static_assert(sizeof...(PICK) <= 1, "one pick array at most");
    extern __shared__ float s_tab[];  // [d + 1]
    __shared__ __attribute__((aligned(16))) uint32_t qs[WC][TQ + 4];
    __shared__ __attribute__((aligned(16))) uint32_t rs[WC][TR + 4];
    __shared__ uint32_t s_q[TQ], s_p[TQ];
    __shared__ uint32_t s_pick[PICKED ? TR : 1];  // picked: the row tile's rows in P
    [[maybe_unused]] const uint32_t *pick = nullptr;
    if constexpr (PICKED) pick = (pick_arg, ...);
    uint32_t row0, nrows;
    if (!ivf_tile_open(off, nlist, cnt, lstart, tstart, inv, pref, nprobe, s_q, s_p, &row0, &nrows)) return;
    const uint32_t tid = threadIdx.x, rg = tid & 15u, qg = tid >> 4;
    [[maybe_unused]] const uint32_t *Pl = P + (uint64_t)row0 * Wn;  // the list's run (unpicked: row0 is a row of P)
    bin_table_load(s_tab, S, d, root);
    __syncthreads();
    uint32_t lo[RQ], hi[RQ], qi[RQ];
#pragma unroll
    for (uint32_t a = 0; a < RQ; ++a) {
        qi[a] = s_q[qg * RQ + a];
        lo[a] = 0xFFFFFFFFu;
        hi[a] = 0u;
    }
    const uint32_t nrt = (nrows + TR - 1) / TR;
    for (uint32_t rt = blockIdx.y; rt < nrt; rt += gridDim.y) {
        const uint32_t r0 = rt * TR;  // (within the list)
        if constexpr (PICKED) {
            if (tid < TR) s_pick[tid] = r0 + tid < nrows ? pick[(uint64_t)row0 + r0 + tid] : 0u;
        }
        uint32_t acc[RQ][RR];
#pragma unroll
        for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
            for (uint32_t b = 0; b < RR; ++b) acc[a][b] = 0u;
        for (uint32_t t0 = 0; t0 < Wn; t0 += WC) {
            const uint32_t tc = min(WC, Wn - t0);
            __syncthreads();  // the previous chunk's readers are done
#pragma unroll
            for (uint32_t e = 0; e < TQ * WC / 256; ++e) {
                const uint32_t idx = tid + 256 * e, r = idx / WC, c = idx % WC;
                const uint32_t q = s_q[r];
                qs[c][r] = (q != kKnnNone && c < tc) ? Q[(size_t)q * Wn + t0 + c] : 0u;
            }
#pragma unroll
            for (uint32_t e = 0; e < TR * WC / LW / 256; ++e) {  // (64 rows x 32 / LW loads: 2, 4 or 8 per lane)
                const uint32_t idx = tid + 256 * e, r = idx / (WC / LW), c0 = (idx % (WC / LW)) * LW;
                const bool ok = r0 + r < nrows && c0 < tc;
                uint32_t w[LW];
#pragma unroll
                for (uint32_t j = 0; j < LW; ++j) w[j] = 0u;
                if constexpr (PICKED) {
                    if (ok) bin_load<LW>(P + (uint64_t)s_pick[r] * Wn + t0 + c0, w);
                } else {
                    if (ok) bin_load<LW>(Pl + (uint64_t)(r0 + r) * Wn + t0 + c0, w);
                }
#pragma unroll
                for (uint32_t j = 0; j < LW; ++j) rs[c0 + j][r] = w[j];
            }
            __syncthreads();
            auto advance = [&](uint32_t t) {
                const uint4 qa = *reinterpret_cast<const uint4 *>(&qs[t][qg * RQ]);
                const uint4 qb = *reinterpret_cast<const uint4 *>(&qs[t][qg * RQ + 4]);
                const uint4 rv = *reinterpret_cast<const uint4 *>(&rs[t][rg * RR]);
                const uint32_t qv[RQ] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
                const uint32_t rr[RR] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
                for (uint32_t a = 0; a < RQ; ++a)
#pragma unroll
                    for (uint32_t b = 0; b < RR; ++b) acc[a][b] = __builtin_popcount(qv[a] ^ rr[b]) + acc[a][b];
            };
            if (tc == WC) {
#pragma unroll 8
                for (uint32_t t = 0; t < WC; ++t) advance(t);
            } else {
                for (uint32_t t = 0; t < tc; ++t) advance(t);
            }
        }
        const uint32_t rb = r0 + rg * RR;
        // (H <= d: the pad bits of both sides are zero)
        ivf_tile_store(qi, s_p, rb, nrows, wstride, W, lo, hi, [&](uint32_t a, uint32_t b) { return s_tab[min(acc[a][b], d)]; });
    }
    knn_key_range(lo, hi, [&](uint32_t a) { return qi[a]; }, kmin, kmax);
}

// block (x = chunk of positions, y = query): the positions of the chunk whose list fewer than kIvffTileMin queries probe,
// one per lane and pass; the query's W <= 256 words in LDS.  Items past |S(q)| leave at once.  Picked: seg is a position
// of the view, and the row is pick[that position].
template <int LW, class... PICK>
__global__ __launch_bounds__(256) void k_ivfbin_scan(const uint32_t *__restrict__ Q, const uint32_t *__restrict__ P, uint32_t Wn,
                                                     uint32_t d, const float *__restrict__ S, int root,
                                                     const uint32_t *__restrict__ probe, const uint32_t *__restrict__ cnt,
                                                     const uint32_t *__restrict__ pref, const uint32_t *__restrict__ seg,
                                                     uint32_t nprobe, uint32_t chunk, uint64_t wstride, float *__restrict__ W,
                                                     uint32_t *__restrict__ kmin, uint32_t *__restrict__ kmax, PICK... pick_arg) {
    constexpr bool PICKED = sizeof...(PICK) == 1;
    static_assert(sizeof...(PICK) <= 1, "one pick array at most");
    [[maybe_unused]] const uint32_t *pick = nullptr;
    if constexpr (PICKED) pick = (pick_arg, ...);
    extern __shared__ float s_tab[];  // [d + 1]
    __shared__ __attribute__((aligned(16))) uint32_t s_x[VQHIP_BINARY_MAX_DIM / 32];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint32_t *pq = pref + (size_t)q * (nprobe + 1);
    const uint32_t *sq = seg + (size_t)q * nprobe;
    const uint32_t *lq = probe + (size_t)q * nprobe;
    const uint32_t total = (uint32_t)min((uint64_t)pq[nprobe], wstride);
    const uint64_t p0 = (uint64_t)blockIdx.x * chunk;
    if (p0 >= total) return;  // (uniform)
    const uint32_t p1 = (uint32_t)min((uint64_t)total, p0 + chunk);
    for (uint32_t t = tid; t < Wn; t += 256) s_x[t] = Q[(size_t)q * Wn + t];
    bin_table_load(s_tab, S, d, root);
    __syncthreads();
    float *wq = W + (size_t)q * wstride;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t base = (uint32_t)p0; base < p1; base += 256) {
        const uint32_t pos = base + tid;
        if (pos >= p1) continue;
        const uint32_t slot = ivf_slot(pq, nprobe, pos);
        if (cnt[lq[slot]] >= kIvffTileMin) continue;  // (a position exists: its list is real; the tile kernel has it)
        uint64_t row = (uint64_t)sq[slot] + (pos - pq[slot]);
        if constexpr (PICKED) row = pick[row];
        const uint32_t *r = P + row * Wn;
        uint32_t h = 0;
        for (uint32_t t = 0; t < Wn; t += LW) {
            uint32_t w[LW];
            bin_load<LW>(r + t, w);
#pragma unroll
            for (uint32_t j = 0; j < LW; ++j) h = __builtin_popcount(w[j] ^ s_x[t + j]) + h;
        }
        const float dv = s_tab[min(h, d)];
        const uint32_t key = adc_key(dv);
        if (key != 0xFFFFFFFFu) {
            lo = min(lo, key);
            hi = max(hi, key);
        }
        wq[pos] = dv;
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

}  // namespace

// words per load of the row loaders: 4 (16 bytes), 2 (8 bytes) or 1, from the words of a row and the base of the buffer
int bin_load_width(const uint32_t *P, uint32_t W) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(P);
    if (W % 4 == 0 && a % 16 == 0) return 4;
    if (W % 2 == 0 && a % 8 == 0) return 2;
    return 1;
}

// The two distance passes of a batch behind its plan (kernels.hpp): every D(q, i) of the probed lists into v.W, the key
// range into p.  Q [nb][bin_words(d)]: the batch's queries, packed (launch_bq_pack).  v.pick: over the view of a filtered
// call, the picked kernels.
int launch_ivfbin_distances(const IvffPlan &p, const IvfBatchView &v, int metric, const uint32_t *P, uint32_t d, const float *S,
                            const uint32_t *Q, hipStream_t stream) {
    if (v.nb == 0) return VQHIP_OK;
    if (d == 0 || d > VQHIP_BINARY_MAX_DIM) return fail(VQHIP_ERR_INVALID_INPUT, "d %u must be in [1, 8192]", d);
    const uint32_t Wn = bin_words(d);
    const int lw = bin_load_width(P, Wn), root = metric == VQHIP_EUCLIDEAN ? 1 : 0;
    const size_t lds = ((size_t)d + 1) * 4;
    const uint64_t items = (v.wstride + v.chunk - 1) / v.chunk;
    if (p.tiles_max > 0) {
        const dim3 grid((uint32_t)p.tiles_max, (uint32_t)p.cols);
        auto tile = [&](auto kernel, auto... pick) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, Q, P, Wn, d, S, root, v.off, v.nlist, p.cnt, p.lstart, p.tstart, v.inv,
                               v.pref, v.nprobe, v.wstride, v.W, p.kmin, p.kmax, pick...);
        };
        if (v.pick) {
            if (lw == 4) tile(k_ivfbin_tile<4, const uint32_t *>, v.pick);
            else if (lw == 2) tile(k_ivfbin_tile<2, const uint32_t *>, v.pick);
            else tile(k_ivfbin_tile<1, const uint32_t *>, v.pick);
        } else if (lw == 4) tile(k_ivfbin_tile<4>);
        else if (lw == 2) tile(k_ivfbin_tile<2>);
        else tile(k_ivfbin_tile<1>);
        VQ_LAUNCH_CHECK("k_ivfbin_tile");
    }
    if (items > 0) {
        auto scan = [&](auto kernel, auto... pick) {
            hipLaunchKernelGGL(kernel, dim3((uint32_t)items, v.nb), dim3(256), lds, stream, Q, P, Wn, d, S, root, v.probe, p.cnt, v.pref,
                               v.seg, v.nprobe, v.chunk, v.wstride, v.W, p.kmin, p.kmax, pick...);
        };
        if (v.pick) {
            if (lw == 4) scan(k_ivfbin_scan<4, const uint32_t *>, v.pick);
            else if (lw == 2) scan(k_ivfbin_scan<2, const uint32_t *>, v.pick);
            else scan(k_ivfbin_scan<1, const uint32_t *>, v.pick);
        } else if (lw == 4) scan(k_ivfbin_scan<4>);
        else if (lw == 2) scan(k_ivfbin_scan<2>);
        else scan(k_ivfbin_scan<1>);
        VQ_LAUNCH_CHECK("k_ivfbin_scan");
    }
    return VQHIP_OK;
}

}  // namespace vqhip
