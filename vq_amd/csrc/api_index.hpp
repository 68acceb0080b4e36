// api_index.hpp -- what the two files of index entry points share (api_resident.hip, api_ivf.hip): the checks and the
// host-row staging of every index, the row mask's scope, the flat index (an inverted file's coarse quantizer is one)
// and the range result with its front.  A new index's entry points include this header.
#pragma once
#include <algorithm>
#include <memory>
#include <type_traits>

#include "api_common.hpp"

using namespace vqhip;

// What vqhip_flat, vqhip_sqindex and vqhip_binary have in common: the rows stay on the device from create on, a search
// takes [nq][d] f32 queries to [nq][topk] results, and every call locks the handle and runs on the calling thread's stream.
struct Resident {
    HandleSync sync;
    uint64_t n = 0;
    uint32_t d = 0;
    int metric = VQHIP_EUCLIDEAN;
    DevBuf q, cand, idx, out;  // per-call workspaces
    DevBuf compact_ws;         // a removal's block counts and starts (k_compact.hip)
    uint32_t width() const { return d; }     // floats of a query
    int on_device() { return VQHIP_OK; }     // (the rows stay where create put them: no device of its own to check)
};

// The indexes of exact distances.  T (vqhip_flat, vqhip_sqindex, vqhip_abin, vqhip_sq4index) keeps its rows and the three launcher calls that
// read them: launch_search, launch_rerank and launch_range.
template <class T>
struct ExactResident : Resident {
    DevBuf rnorm;               // |row| for cosine
    DevBuf qnorm, dist, state;  // per-call workspaces
    DevBuf rr_cand, rr_err;     // rerank: candidate ids, the out-of-range flag
    DevBuf radii, range_ws;     // range search: the radii, the stage's counts and offsets
    DevBuf mask_ws;             // a filtered host call's row mask on the device
    const uint32_t *mask = nullptr;  // the row mask of the filtered call that holds the lock (MaskScope), NULL otherwise

    size_t mask_bytes() const { return (size_t)((n + 31) / 32) * 4; }
    DevBuf *norm_buf() { return vq_is_cos(metric) ? &rnorm : nullptr; }
    // a host form's mask, ceil(n / 32) words, up into mask_ws
    int stage_mask(const uint32_t *allowed, hipStream_t s) {
        VQ_TRY(mask_ws.ensure(mask_bytes()));
        VQ_HIP(hipMemcpyAsync(mask_ws.p, allowed, mask_bytes(), hipMemcpyHostToDevice, s));
        return VQHIP_OK;
    }

    // the query norms of a cosine index into qnorm (NULL otherwise)
    int qnorms(const float *queries_dev, uint32_t nq, const float **qn, hipStream_t s) {
        *qn = nullptr;
        if (!vq_is_cos(metric)) return VQHIP_OK;
        VQ_TRY(qnorm.ensure((size_t)nq * 4));
        VQ_TRY(launch_knn_norms(queries_dev, 0, nq, d, qnorm.as<float>(), s));
        *qn = qnorm.as<float>();
        return VQHIP_OK;
    }

    // queries_dev [nq][d] f32 on the device -> [nq][topk] results on the device, enqueued on s
    int search_enqueue(const float *queries_dev, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev, hipStream_t s) {
        const uint32_t qb = knn_query_batch(n, nq);
        VQ_TRY(dist.ensure((size_t)qb * n * 4));
        VQ_TRY(state.ensure(knn_state_bytes(qb)));
        VQ_TRY(cand.ensure(topk_cand_bytes(qb)));
        const float *qn = nullptr;
        VQ_TRY(qnorms(queries_dev, nq, &qn, s));
        return static_cast<T *>(this)->launch_search(queries_dev, qn, nq, topk, idx_dev, dist_dev, s);
    }
};

// The row mask of a filtered call for the launches it makes on the handle: set under the handle's lock, cleared on every
// exit, so that a call without a mask finds NULL and takes the unmasked kernels.
struct MaskScope {
    const uint32_t *&slot;
    MaskScope(const uint32_t *&s, const uint32_t *m) : slot(s) { slot = m; }
    ~MaskScope() { slot = nullptr; }
    MaskScope(const MaskScope &) = delete;
    MaskScope &operator=(const MaskScope &) = delete;
};
inline int check_mask_aligned(const void *dev_allowed) {
    if (reinterpret_cast<uintptr_t>(dev_allowed) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "the row mask is not 4-byte aligned");
    return VQHIP_OK;
}

// every create takes 1 <= n < 2^32 rows and a metric of include/vqhip.h (two checks: each create has its own between them)
inline int check_rows(uint64_t n) {
    if (n == 0 || n >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "n must be in [1, 2^32)");
    return VQHIP_OK;
}
inline int check_metric(int metric) {
    if (metric < VQHIP_SQUARED_EUCLIDEAN || metric > VQHIP_COSINE_UNCLAMPED) return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    return VQHIP_OK;
}

// every index's search takes 1 <= topk <= min(n, 1024)
inline int check_topk(uint64_t n, uint32_t topk) {
    if (topk == 0 || topk > 1024 || topk > n)
        return fail(VQHIP_ERR_INVALID_INPUT, "topk %u must be in [1, min(n, 1024)] (n = %llu)", topk, (unsigned long long)n);
    return VQHIP_OK;
}

// Host rows that only pass through the device: n rows of row_b bytes at src go up through a staging buffer of at most
// kStageBytes, and piece(device piece, first row, row count) queues the work on each.  Every piece has been waited for.
constexpr size_t kStageBytes = 256u << 20;

template <class F>
static int staged_rows(const void *src, uint64_t n, size_t row_b, hipStream_t s, F &&piece) {
    const uint64_t per = std::max<uint64_t>(1, kStageBytes / row_b);
    DevBuf stage;
    VQ_TRY(stage.alloc((size_t)std::min<uint64_t>(per, n) * row_b));
    for (uint64_t r0 = 0; r0 < n; r0 += per) {
        const uint64_t rn = std::min<uint64_t>(per, n - r0);
        VQ_HIP(hipMemcpyAsync(stage.p, static_cast<const char *>(src) + r0 * row_b, (size_t)rn * row_b, hipMemcpyHostToDevice, s));
        VQ_TRY(piece(stage.p, r0, rn));
        VQ_HIP(hipStreamSynchronize(s));  // (the staging buffer is filled again)
    }
    return VQHIP_OK;
}

// The host form of a search: nq rows of `width` floats go up into q, `enqueue` queues the device form over q / idx / out
// on s, and the [nq][rw] results come down into idx_out and dist_out after one wait.  out and dist_out NULL: a search with
// one result array (the probe).
template <class F>
static int host_search(Entry &in, hipStream_t s, DevBuf &q, DevBuf &idx, DevBuf *out, const float *queries, uint32_t nq,
                       uint32_t width, uint32_t rw, uint32_t *idx_out, float *dist_out, F &&enqueue) {
    const size_t res_b = (size_t)nq * rw * 4;
    VQ_TRY(q.ensure((size_t)nq * width * 4));
    VQ_TRY(idx.ensure(res_b));
    if (out) VQ_TRY(out->ensure(res_b));
    VQ_HIP(hipMemcpyAsync(q.p, queries, (size_t)nq * width * 4, hipMemcpyHostToDevice, s));
    VQ_TRY(enqueue());
    VQ_HIP(hipMemcpyAsync(idx_out, idx.p, res_b, hipMemcpyDeviceToHost, s));
    if (out) VQ_HIP(hipMemcpyAsync(dist_out, out->p, res_b, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
}

inline void swap_buf(DevBuf &a, DevBuf &b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

struct vqhip_flat : ExactResident<vqhip_flat> {
    int dtype = 0;
    DevBuf rows;  // [n][d] f32 or f16 bits; `bytes` is the capacity (an add grows it)

    DevBuf &payload() { return rows; }
    size_t row_bytes() const { return (size_t)d * (dtype == 1 ? 2 : 4); }
    int norms_enqueue(const void *X, uint64_t count, float *out, hipStream_t s) { return launch_knn_norms(X, dtype, count, d, out, s); }
    int launch_search(const float *queries_dev, const float *qn, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                      hipStream_t s) {
        return launch_knn_search(metric, rows.p, dtype, n, d, rnorm.as<float>(), queries_dev, qn, nq, topk, dist.as<float>(), state.p,
                                 cand.as<unsigned long long>(), idx_dev, dist_dev, mask, s);
    }
    int launch_rerank(const float *qn, uint32_t nq, uint32_t c, uint32_t topk, hipStream_t s) {
        return launch_knn_rerank(metric, rows.p, dtype, n, d, rnorm.as<float>(), q.as<float>(), qn, nq, rr_cand.as<uint32_t>(), c, topk,
                                 idx.as<uint32_t>(), out.as<float>(), rr_err.as<uint32_t>(), s);
    }
    int launch_range(const float *queries_dev, const float *qn, uint32_t nq, uint64_t max_results, RangeOut *r, hipStream_t s) {
        return launch_knn_range(metric, rows.p, dtype, n, d, rnorm.as<float>(), queries_dev, qn, nq, radii.as<float>(), max_results,
                                dist.as<float>(), state.p, range_ws.p, r, mask, s);
    }
};

namespace vqhip {
int flat_create(const void *src, hipMemcpyKind kind, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out);  // api_resident.hip
}  // namespace vqhip

struct vqhip_range {
    RangeOut r;
};

// What a range call checks without a device or an index: the pointers it reads and writes, max_results, the radii
// (f32 distances; u32 Hamming radii of the binary indexes, where every value is one).
template <class R>
static int range_args(const void *queries, const R *radii, uint32_t nq, uint64_t max_results, vqhip_range **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (nq && (!queries || !radii)) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (max_results == 0) return fail(VQHIP_ERR_INVALID_INPUT, "max_results must be at least 1");
    if constexpr (std::is_floating_point<R>::value) {
        for (uint32_t q = 0; q < nq; ++q)
            if (radii[q] != radii[q]) return fail(VQHIP_ERR_INVALID_INPUT, "the radius of query %u is NaN", q);
    }
    return VQHIP_OK;
}

// The front of every range call on a handle h (a Resident or an IvfLists), in the order every entry point checks:
// range_args (no device, no index), the handle, the alignment of a device form's queries, the handle's lock, `checks`
// (the index's own, of what changes under add), the device, the index's device, the calling thread's stream.  Then the
// result object, a host form's queries up through h->q, and body(queries on the device, the result, s) for nq > 0, which
// leaves the result complete and has waited for s on every exit; no queries: the empty result, lims = [0].
template <class H, class R, class C, class F>
static int range_enter(H *h, const void *queries, bool host, uint32_t nq, const R *radii, uint64_t max_results, vqhip_range **out,
                       C &&checks, F &&body) {
    VQ_TRY(range_args(queries, radii, nq, max_results, out));
    if (!h) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (!host && (reinterpret_cast<uintptr_t>(queries) & 3)) return fail(VQHIP_ERR_INVALID_INPUT, "queries are not 4-byte aligned");
    Entry in(h->sync);  // (an inverted file's n changes under add: read under the lock)
    VQ_TRY(checks());
    VQ_TRY(require_gfx950());
    VQ_TRY(h->on_device());
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    std::unique_ptr<vqhip_range> r(new vqhip_range());
    if (nq) {
        const float *qdev = reinterpret_cast<const float *>(queries);
        if (host) {
            VQ_TRY(h->q.ensure((size_t)nq * h->width() * 4));
            VQ_HIP(hipMemcpyAsync(h->q.p, queries, (size_t)nq * h->width() * 4, hipMemcpyHostToDevice, s));
            qdev = h->q.template as<float>();
        }
        VQ_TRY(body(qdev, &r->r, s));
    } else {
        VQ_TRY(launch_range_begin(&r->r, 0, max_results, s));
        VQ_HIP(hipStreamSynchronize(s));
    }
    in.synced();
    *out = r.release();
    return VQHIP_OK;
}
