// api_resident.hip -- extern "C" entry points of the resident indexes (vqhip_flat, vqhip_sqindex, vqhip_binary, vqhip_abin, vqhip_sq4index) and
// their host layer: searches, reranks, range searches, adding and removing rows.  Host-side orchestration only.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "api_index.hpp"
#include "compact.hpp"

// ------------------------------------------------------------------ resident indexes: the shared host layer ----
// The front of every search, rerank and read-back of a resident handle h, in the order every entry point checks: the
// pointers, `checks` (the call's own, of its counts), nothing to do for nq == 0 (a read-back passes 1), the alignment of a
// device form's queries (NULL: a host form), the device, the handle's lock and the calling thread's stream -- then
// body(in, s).
template <class H, class C, class F>
static int resident_enter(H *h, bool args, C &&checks, uint32_t nq, const void *dev_queries, F &&body) {
    if (!h || !args) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> held(h->sync.mu);  // `checks` reads n, which an add or a removal on another thread changes
    VQ_TRY(checks());
    if (nq == 0) return VQHIP_OK;
    if (reinterpret_cast<uintptr_t>(dev_queries) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "queries are not 4-byte aligned");
    VQ_TRY(require_gfx950());
    Entry in(h->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    return body(in, s);
}
static int no_checks() { return VQHIP_OK; }

// the two search entry points of every resident index, over its search_enqueue(...)
template <class T>
static int resident_search(T *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    return resident_enter(x, queries && idx_out && dist_out, [&] { return check_topk(x->n, topk); }, nq, nullptr, [&](Entry &in, hipStream_t s) {
        return host_search(in, s, x->q, x->idx, &x->out, queries, nq, x->d, topk, idx_out, dist_out, [&] {
            return x->search_enqueue(x->q.template as<float>(), nq, topk, x->idx.template as<uint32_t>(), x->out.template as<float>(), s);
        });
    });
}
template <class T>
static int resident_search_device(T *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx, void *dev_dist) {
    return resident_enter(x, dev_queries && dev_idx && dev_dist, [&] { return check_topk(x->n, topk); }, nq, dev_queries, [&](Entry &, hipStream_t s) {
        return x->search_enqueue(reinterpret_cast<const float *>(dev_queries), nq, topk, reinterpret_cast<uint32_t *>(dev_idx),
                                 reinterpret_cast<float *>(dev_dist), s);
    });
}

// the two filtered search entry points of a flat, a scalar or a binary index: resident_search / _device with the row mask `allowed`
// (host: ceil(n / 32) words staged into mask_ws; device: a 4-byte aligned pointer) in force for the launches
template <class T>
static int exact_search_masked(T *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed, uint32_t *idx_out,
                               float *dist_out) {
    return resident_enter(x, queries && idx_out && dist_out && allowed, [&] { return check_topk(x->n, topk); }, nq, nullptr,
                          [&](Entry &in, hipStream_t s) -> int {
        VQ_TRY(x->stage_mask(allowed, s));
        MaskScope scope(x->mask, x->mask_ws.template as<uint32_t>());
        return host_search(in, s, x->q, x->idx, &x->out, queries, nq, x->d, topk, idx_out, dist_out, [&] {
            return x->search_enqueue(x->q.template as<float>(), nq, topk, x->idx.template as<uint32_t>(), x->out.template as<float>(), s);
        });
    });
}
template <class T>
static int exact_search_masked_device(T *x, const void *dev_queries, uint32_t nq, uint32_t topk, const uint32_t *dev_allowed,
                                      void *dev_idx, void *dev_dist) {
    if (!dev_queries || !dev_idx || !dev_dist || !dev_allowed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(check_mask_aligned(dev_allowed));
    return resident_enter(x, true, [&] { return check_topk(x->n, topk); }, nq, dev_queries, [&](Entry &, hipStream_t s) {
        MaskScope scope(x->mask, dev_allowed);
        return x->search_enqueue(reinterpret_cast<const float *>(dev_queries), nq, topk, reinterpret_cast<uint32_t *>(dev_idx),
                                 reinterpret_cast<float *>(dev_dist), s);
    });
}

// the exact rerank of cand [nq][c] on a flat or a scalar index
template <class T>
static int exact_rerank(T *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk, uint32_t *idx_out,
                        float *dist_out) {
    auto checks = [&]() -> int {
        if (c == 0 || c > 4096) return fail(VQHIP_ERR_INVALID_INPUT, "candidates per query %u must be in [1, 4096]", c);
        if (topk == 0 || topk > c) return fail(VQHIP_ERR_INVALID_INPUT, "topk %u must be in [1, candidates = %u]", topk, c);
        return VQHIP_OK;
    };
    return resident_enter(x, queries && cand && idx_out && dist_out, checks, nq, nullptr, [&](Entry &in, hipStream_t s) -> int {
        const size_t q_b = (size_t)nq * x->d * 4, cand_b = (size_t)nq * c * 4, res_b = (size_t)nq * topk * 4;
        VQ_TRY(x->q.ensure(q_b));
        VQ_TRY(x->rr_cand.ensure(cand_b));
        VQ_TRY(x->idx.ensure(res_b));
        VQ_TRY(x->out.ensure(res_b));
        VQ_TRY(x->rr_err.ensure(4));
        VQ_HIP(hipMemcpyAsync(x->q.p, queries, q_b, hipMemcpyHostToDevice, s));
        VQ_HIP(hipMemcpyAsync(x->rr_cand.p, cand, cand_b, hipMemcpyHostToDevice, s));
        VQ_HIP(hipMemsetAsync(x->rr_err.p, 0, 4, s));
        const float *qn = nullptr;
        VQ_TRY(x->qnorms(x->q.template as<float>(), nq, &qn, s));
        VQ_TRY(x->launch_rerank(qn, nq, c, topk, s));
        uint32_t err = 0;
        VQ_HIP(hipMemcpyAsync(&err, x->rr_err.p, 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipMemcpyAsync(idx_out, x->idx.p, res_b, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipMemcpyAsync(dist_out, x->out.p, res_b, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        if (err) return fail(VQHIP_ERR_INVALID_INPUT, "a candidate row id is >= n = %llu", (unsigned long long)x->n);
        return VQHIP_OK;
    });
}

// ------------------------------------------------------------------ adding and removing rows (k_compact.hip) ----
// include/vqhip.h, "adding and removing rows"; DESIGN.md section 26.  What a handle T offers for it: payload() (the DevBuf
// of its rows, whose `bytes` is the capacity), row_bytes(), norm_buf() (rnorm under the cosines, else NULL) and
// norms_enqueue(rows, count, out), the launcher its create uses over `count` rows.
// Room for `total` rows of rb bytes where cur holds n: cur itself where its capacity reaches, else `grown`, a new buffer
// of max(needed, 1.5 x capacity) bytes with the n rows copied in (queued on s).  *base: row 0 of whichever it is.
static int grow_rows(DevBuf &cur, uint64_t n, uint64_t total, size_t rb, DevBuf &grown, char **base, hipStream_t s) {
    const size_t need = (size_t)total * rb;
    if (cur.p && cur.bytes >= need) {
        *base = cur.as<char>();
        return VQHIP_OK;
    }
    VQ_TRY(grown.alloc(std::max(need, cur.bytes + (cur.bytes + 1) / 2)));
    VQ_HIP(hipMemcpyAsync(grown.p, cur.p, (size_t)n * rb, hipMemcpyDeviceToDevice, s));
    *base = grown.as<char>();
    return VQHIP_OK;
}

// R' = R ++ B: store(dst, s) writes the payload of the n_add new rows at dst (device memory behind row n - 1) and is the
// last step that can fail; n, the payload and the norms change behind it.
template <class T, class Store>
static int resident_add(T *x, const void *src, uint64_t n_add, Store &&store) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    auto checks = [&]() -> int {
        if (n_add >= (1ull << 32) || x->n + n_add >= (1ull << 32))
            return fail(VQHIP_ERR_INVALID_INPUT, "n + n_add = %llu + %llu must stay below 2^32", (unsigned long long)x->n,
                        (unsigned long long)n_add);
        return VQHIP_OK;
    };
    return resident_enter(x, src != nullptr, checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        const uint64_t n = x->n, total = n + n_add;
        const size_t rb = x->row_bytes();
        DevBuf grown, grown_norm;  // (freed here where the call fails)
        char *base = nullptr, *nbase = nullptr;
        DevBuf *norm = x->norm_buf();
        int rc = grow_rows(x->payload(), n, total, rb, grown, &base, s);
        if (rc == VQHIP_OK && norm) rc = grow_rows(*norm, n, total, 4, grown_norm, &nbase, s);
        if (rc == VQHIP_OK) rc = store(base + n * rb, s);
        if (rc == VQHIP_OK && norm) rc = x->norms_enqueue(base + n * rb, n_add, reinterpret_cast<float *>(nbase) + n, s);
        // the old buffers are freed below and a failed call frees the grown ones: nothing may still run on either
        const hipError_t e = hipStreamSynchronize(s);
        in.synced();
        VQ_TRY(rc);
        VQ_HIP(e);
        if (grown.p) swap_buf(x->payload(), grown);
        if (grown_norm.p) swap_buf(*norm, grown_norm);
        x->n = total;
        return VQHIP_OK;
    });
}

// R' = R without the rows of the mask `remove` (ceil(n / 32) words; host: staged into mask_ws), the order kept
template <class T>
static int resident_remove(T *x, const uint32_t *remove, bool host, uint64_t *removed) {
    if (!x || !remove || !removed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *removed = 0;
    std::lock_guard<std::recursive_mutex> held(x->sync.mu);
    if (host) {  // what the device would count: an empty removal and one of every row end here, without a device
        uint64_t kept = 0;
        for (uint64_t w = 0; w < (x->n + 31) / 32; ++w) kept += compact_popc32(compact_keep_word(remove[w], w, x->n));
        if (kept == x->n) return VQHIP_OK;
        if (kept == 0) return fail(VQHIP_ERR_INVALID_INPUT, "the removal would leave no row (n = %llu)", (unsigned long long)x->n);
    } else {
        VQ_TRY(check_mask_aligned(remove));
    }
    return resident_enter(x, true, no_checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        const uint64_t n = x->n;
        const size_t rb = x->row_bytes();
        const uint32_t *mask = remove;
        if (host) {
            VQ_TRY(x->stage_mask(remove, s));
            mask = x->mask_ws.template as<uint32_t>();
        }
        VQ_TRY(x->compact_ws.ensure(compact_ws_bytes(n)));
        VQ_TRY(launch_compact_plan(mask, n, x->compact_ws.p, s));
        uint32_t na = 0;
        VQ_HIP(hipMemcpyAsync(&na, compact_survivors(x->compact_ws.p, n), 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        if (na == n) return VQHIP_OK;
        if (na == 0) return fail(VQHIP_ERR_INVALID_INPUT, "the removal would leave no row (n = %llu)", (unsigned long long)n);
        DevBuf rows, norms;  // sized for the survivors; the old buffers leave with them
        DevBuf *norm = x->norm_buf();
        VQ_TRY(rows.alloc((size_t)na * rb));
        if (norm) VQ_TRY(norms.alloc((size_t)na * 4));
        int rc = launch_compact_move(mask, n, x->compact_ws.p, x->payload().p, rows.p, rb, s);
        if (rc == VQHIP_OK && norm) rc = launch_compact_move(mask, n, x->compact_ws.p, norm->p, norms.p, 4, s);
        const hipError_t e = hipStreamSynchronize(s);  // before either side is freed
        VQ_TRY(rc);
        VQ_HIP(e);
        swap_buf(x->payload(), rows);
        if (norm) swap_buf(*norm, norms);
        x->n = na;
        *removed = n - na;
        return VQHIP_OK;
    });
}

// ------------------------------------------------------------------ exact k-NN (k_knn.hip) ----
namespace vqhip {
// rows from host (kind = H2D) or device (D2D) memory into a new index
int flat_create(const void *src, hipMemcpyKind kind, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "rows is NULL");
    if (d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "d must be at least 1");
    VQ_TRY(check_rows(n));
    if (dtype != 0 && dtype != 1) return fail(VQHIP_ERR_INVALID_INPUT, "dtype must be 0 (f32) or 1 (f16), not %d", dtype);
    VQ_TRY(check_metric(metric));
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_flat> f(new vqhip_flat());
    f->n = n;
    f->d = d;
    f->dtype = dtype;
    f->metric = metric;
    const size_t bytes = (size_t)n * d * (dtype == 1 ? 2 : 4);
    VQ_TRY(f->rows.alloc(bytes));
    VQ_HIP(hipMemcpyAsync(f->rows.p, src, bytes, kind, s));
    if (vq_is_cos(metric)) {
        VQ_TRY(f->rnorm.alloc((size_t)n * 4));
        VQ_TRY(launch_knn_norms(f->rows.p, dtype, n, d, f->rnorm.as<float>(), s));
    }
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its rows once this returns
    *out = f.release();
    return VQHIP_OK;
}
}  // namespace vqhip

// n_add rows in the index's dtype, from host (kind = H2D) or device (D2D) memory, behind the last row
static int flat_add(vqhip_flat *f, const void *src, hipMemcpyKind kind, uint64_t n_add) {
    return resident_add(f, src, n_add, [&](char *dst, hipStream_t s) -> int {
        VQ_HIP(hipMemcpyAsync(dst, src, (size_t)n_add * f->row_bytes(), kind, s));
        return VQHIP_OK;
    });
}

extern "C" {

int vqhip_flat_create(const void *rows, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out) {
    VQ_API_BEGIN
    return flat_create(rows, hipMemcpyHostToDevice, n, d, dtype, metric, out);
    VQ_API_END
}

int vqhip_flat_create_device(const void *dev_rows, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out) {
    VQ_API_BEGIN
    return flat_create(dev_rows, hipMemcpyDeviceToDevice, n, d, dtype, metric, out);
    VQ_API_END
}

int vqhip_flat_destroy(vqhip_flat *f) {
    delete f;
    return VQHIP_OK;
}

int vqhip_flat_info(const vqhip_flat *f, uint64_t *n, uint32_t *d, int *dtype, int *metric) {
    if (!f) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n) *n = f->n;
    if (d) *d = f->d;
    if (dtype) *dtype = f->dtype;
    if (metric) *metric = f->metric;
    return VQHIP_OK;
}

int vqhip_flat_search(vqhip_flat *f, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return resident_search(f, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_flat_search_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return resident_search_device(f, dev_queries, nq, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_flat_search_masked(vqhip_flat *f, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                             uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_search_masked(f, queries, nq, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_flat_search_masked_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, uint32_t topk, const uint32_t *dev_allowed,
                                    void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return exact_search_masked_device(f, dev_queries, nq, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_flat_rerank(vqhip_flat *f, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk,
                      uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_rerank(f, queries, nq, cand, c, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_flat_add(vqhip_flat *f, const void *rows, uint64_t n_add) {
    VQ_API_BEGIN
    return flat_add(f, rows, hipMemcpyHostToDevice, n_add);
    VQ_API_END
}

int vqhip_flat_add_device(vqhip_flat *f, const void *dev_rows, uint64_t n_add) {
    VQ_API_BEGIN
    return flat_add(f, dev_rows, hipMemcpyDeviceToDevice, n_add);
    VQ_API_END
}

int vqhip_flat_remove(vqhip_flat *f, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(f, remove_words, true, removed);
    VQ_API_END
}

int vqhip_flat_remove_device(vqhip_flat *f, const uint32_t *dev_remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(f, dev_remove_words, false, removed);
    VQ_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ scalar index (k_sqindex.hip) ----
struct vqhip_sqindex : ExactResident<vqhip_sqindex> {
    uint32_t levels = 0;
    float mn = 0, mx = 0, step = 0;
    DevBuf codes;  // [n][d] u8; `bytes` is the capacity (an add grows it)

    DevBuf &payload() { return codes; }
    size_t row_bytes() const { return d; }
    int norms_enqueue(const void *C, uint64_t count, float *out, hipStream_t s) {
        return launch_sq_norms(static_cast<const uint8_t *>(C), count, d, mn, step, out, s);
    }
    int launch_search(const float *queries_dev, const float *qn, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                      hipStream_t s) {
        return launch_sq_search(metric, codes.as<uint8_t>(), n, d, mn, step, rnorm.as<float>(), queries_dev, qn, nq, topk, dist.as<float>(),
                                state.p, cand.as<unsigned long long>(), idx_dev, dist_dev, mask, s);
    }
    int launch_rerank(const float *qn, uint32_t nq, uint32_t c, uint32_t topk, hipStream_t s) {
        return launch_sq_rerank(metric, codes.as<uint8_t>(), n, d, mn, step, rnorm.as<float>(), q.as<float>(), qn, nq, rr_cand.as<uint32_t>(),
                                c, topk, idx.as<uint32_t>(), out.as<float>(), rr_err.as<uint32_t>(), s);
    }
    int launch_range(const float *queries_dev, const float *qn, uint32_t nq, uint64_t max_results, RangeOut *r, hipStream_t s) {
        return launch_sq_range(metric, codes.as<uint8_t>(), n, d, mn, step, rnorm.as<float>(), queries_dev, qn, nq, radii.as<float>(),
                               max_results, dist.as<float>(), state.p, range_ws.p, r, mask, s);
    }
};

// src: u8 codes [n][d] (rows == false) or f32 rows [n][d] to encode (rows == true), in host (kind = H2D) or device memory
static int sqindex_create(const void *src, hipMemcpyKind kind, bool rows, float mn, float mx, uint32_t levels, uint64_t n,
                          uint32_t d, int metric, vqhip_sqindex **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    SqbqEncodeOp op;
    float step = 0;
    VQ_TRY(sq_check(mn, mx, levels, &step));
    if (!src) return fail(VQHIP_ERR_NULL_PTR, rows ? "rows is NULL" : "codes is NULL");
    if (d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "d must be at least 1");
    VQ_TRY(check_rows(n));
    VQ_TRY(check_metric(metric));
    if (rows && kind == hipMemcpyDeviceToDevice && (reinterpret_cast<uintptr_t>(src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, "rows are not 4-byte aligned");
    if (rows) VQ_TRY(sq_encode_op(mn, mx, levels, &op));
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_sqindex> x(new vqhip_sqindex());
    x->n = n, x->d = d, x->levels = levels, x->mn = mn, x->mx = mx, x->step = step, x->metric = metric;
    const size_t bytes = (size_t)n * d;
    VQ_TRY(x->codes.alloc(bytes));
    if (!rows) {
        VQ_HIP(hipMemcpyAsync(x->codes.p, src, bytes, kind, s));
    } else if (kind == hipMemcpyDeviceToDevice) {
        VQ_TRY(launch_sqbq_encode(op, static_cast<const float *>(src), bytes, x->codes.as<uint8_t>(), s));
    } else {  // host rows are encoded a piece at a time, so that only the codes stay
        VQ_TRY(staged_rows(src, n, (size_t)d * 4, s, [&](const void *piece, uint64_t r0, uint64_t rn) {
            return launch_sqbq_encode(op, static_cast<const float *>(piece), rn * d, x->codes.as<uint8_t>() + r0 * d, s);
        }));
    }
    if (vq_is_cos(metric)) {
        VQ_TRY(x->rnorm.alloc((size_t)n * 4));
        VQ_TRY(launch_sq_norms(x->codes.as<uint8_t>(), n, d, mn, step, x->rnorm.as<float>(), s));
    }
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its source once this returns
    *out = x.release();
    return VQHIP_OK;
}

// n_add rows behind the last: u8 codes as given (rows == false) or f32 rows through the encode of sqindex_create
static int sqindex_add(vqhip_sqindex *x, const void *src, hipMemcpyKind kind, bool rows, uint64_t n_add) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    SqbqEncodeOp op;
    if (rows) {
        if (kind == hipMemcpyDeviceToDevice && (reinterpret_cast<uintptr_t>(src) & 3))
            return fail(VQHIP_ERR_INVALID_INPUT, "rows are not 4-byte aligned");
        VQ_TRY(sq_encode_op(x->mn, x->mx, x->levels, &op));
    }
    return resident_add(x, src, n_add, [&](char *dst, hipStream_t s) -> int {
        const uint32_t d = x->d;
        uint8_t *codes = reinterpret_cast<uint8_t *>(dst);
        if (!rows) {
            VQ_HIP(hipMemcpyAsync(codes, src, (size_t)n_add * d, kind, s));
            return VQHIP_OK;
        }
        if (kind == hipMemcpyDeviceToDevice) return launch_sqbq_encode(op, static_cast<const float *>(src), n_add * d, codes, s);
        return staged_rows(src, n_add, (size_t)d * 4, s, [&](const void *piece, uint64_t r0, uint64_t rn) {
            return launch_sqbq_encode(op, static_cast<const float *>(piece), rn * d, codes + r0 * d, s);
        });
    });
}

extern "C" {

int vqhip_sqindex_create(float min, float max, uint32_t levels, const uint8_t *codes, uint64_t n, uint32_t d, int metric,
                         vqhip_sqindex **out) {
    VQ_API_BEGIN
    return sqindex_create(codes, hipMemcpyHostToDevice, false, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sqindex_create_device(float min, float max, uint32_t levels, const void *dev_codes, uint64_t n, uint32_t d, int metric,
                                vqhip_sqindex **out) {
    VQ_API_BEGIN
    return sqindex_create(dev_codes, hipMemcpyDeviceToDevice, false, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sqindex_create_rows(float min, float max, uint32_t levels, const float *rows, uint64_t n, uint32_t d, int metric,
                              vqhip_sqindex **out) {
    VQ_API_BEGIN
    return sqindex_create(rows, hipMemcpyHostToDevice, true, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sqindex_create_rows_device(float min, float max, uint32_t levels, const void *dev_rows, uint64_t n, uint32_t d,
                                     int metric, vqhip_sqindex **out) {
    VQ_API_BEGIN
    return sqindex_create(dev_rows, hipMemcpyDeviceToDevice, true, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sqindex_destroy(vqhip_sqindex *x) {
    delete x;
    return VQHIP_OK;
}

int vqhip_sqindex_info(const vqhip_sqindex *x, uint64_t *n, uint32_t *d, int *metric, float *min, float *max, uint32_t *levels) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n) *n = x->n;
    if (d) *d = x->d;
    if (metric) *metric = x->metric;
    if (min) *min = x->mn;
    if (max) *max = x->mx;
    if (levels) *levels = x->levels;
    return VQHIP_OK;
}

int vqhip_sqindex_add_codes(vqhip_sqindex *x, const uint8_t *codes, uint64_t n_add) {
    VQ_API_BEGIN
    return sqindex_add(x, codes, hipMemcpyHostToDevice, false, n_add);
    VQ_API_END
}

int vqhip_sqindex_add_codes_device(vqhip_sqindex *x, const void *dev_codes, uint64_t n_add) {
    VQ_API_BEGIN
    return sqindex_add(x, dev_codes, hipMemcpyDeviceToDevice, false, n_add);
    VQ_API_END
}

int vqhip_sqindex_add_rows(vqhip_sqindex *x, const float *rows, uint64_t n_add) {
    VQ_API_BEGIN
    return sqindex_add(x, rows, hipMemcpyHostToDevice, true, n_add);
    VQ_API_END
}

int vqhip_sqindex_add_rows_device(vqhip_sqindex *x, const void *dev_rows, uint64_t n_add) {
    VQ_API_BEGIN
    return sqindex_add(x, dev_rows, hipMemcpyDeviceToDevice, true, n_add);
    VQ_API_END
}

int vqhip_sqindex_remove(vqhip_sqindex *x, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, remove_words, true, removed);
    VQ_API_END
}

int vqhip_sqindex_remove_device(vqhip_sqindex *x, const uint32_t *dev_remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, dev_remove_words, false, removed);
    VQ_API_END
}

int vqhip_sqindex_codes(vqhip_sqindex *x, uint8_t *codes) {
    VQ_API_BEGIN
    return resident_enter(x, codes != nullptr, no_checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        VQ_HIP(hipMemcpyAsync(codes, x->codes.p, (size_t)x->n * x->d, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_sqindex_search(vqhip_sqindex *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return resident_search(x, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_sqindex_search_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                                void *dev_dist) {
    VQ_API_BEGIN
    return resident_search_device(x, dev_queries, nq, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_sqindex_search_masked(vqhip_sqindex *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                                uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_search_masked(x, queries, nq, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_sqindex_search_masked_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, uint32_t topk,
                                       const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return exact_search_masked_device(x, dev_queries, nq, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_sqindex_rerank(vqhip_sqindex *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk,
                         uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_rerank(x, queries, nq, cand, c, topk, idx_out, dist_out);
    VQ_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ range search (range.hpp) ----
// One range call on a flat or a scalar index h: the radii go up, and the index's driver, h->launch_range, leaves the
// result complete.  masked: a filtered call under the row mask `allowed` (a host form's is staged into mask_ws, a device
// form's is 4-byte aligned); its pointer is checked behind range_args and, like them, before the handle.
template <class H>
static int range_search(H *h, const void *queries, bool host, uint32_t nq, const float *radii, uint64_t max_results,
                        vqhip_range **out, bool masked = false, const uint32_t *allowed = nullptr) {
    if (masked) {
        VQ_TRY(range_args(queries, radii, nq, max_results, out));
        if (!allowed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
        if (!host) VQ_TRY(check_mask_aligned(allowed));
    }
    return range_enter(h, queries, host, nq, radii, max_results, out, no_checks, [&](const float *qdev, RangeOut *r, hipStream_t s) -> int {
        if (masked && host) VQ_TRY(h->stage_mask(allowed, s));
        MaskScope scope(h->mask, !masked ? nullptr : host ? h->mask_ws.template as<uint32_t>() : allowed);
        VQ_TRY(h->radii.ensure((size_t)nq * 4));
        VQ_HIP(hipMemcpyAsync(h->radii.p, radii, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        VQ_TRY(h->dist.ensure((size_t)knn_query_batch(h->n, nq) * h->n * 4));
        VQ_TRY(h->state.ensure(knn_state_bytes(knn_query_batch(h->n, nq))));
        VQ_TRY(h->range_ws.ensure(range_ws_bytes(h->n, nq)));
        const float *qn = nullptr;
        VQ_TRY(h->qnorms(qdev, nq, &qn, s));
        return h->launch_range(qdev, qn, nq, max_results, r, s);
    });
}

extern "C" {

int vqhip_flat_range_search(vqhip_flat *f, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                            vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(f, queries, true, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_flat_range_search_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(f, dev_queries, false, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_sqindex_range_search(vqhip_sqindex *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                               vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_sqindex_range_search_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, const float *radii,
                                      uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_flat_range_search_masked(vqhip_flat *f, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(f, queries, true, nq, radii, max_results, out, true, allowed);
    VQ_API_END
}

int vqhip_flat_range_search_masked_device(vqhip_flat *f, const void *dev_queries, uint32_t nq, const float *radii,
                                          uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(f, dev_queries, false, nq, radii, max_results, out, true, dev_allowed);
    VQ_API_END
}

int vqhip_sqindex_range_search_masked(vqhip_sqindex *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                      const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out, true, allowed);
    VQ_API_END
}

int vqhip_sqindex_range_search_masked_device(vqhip_sqindex *x, const void *dev_queries, uint32_t nq, const float *radii,
                                             uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out, true, dev_allowed);
    VQ_API_END
}

int vqhip_range_info(const vqhip_range *r, uint32_t *nq, uint64_t *total) {
    if (!r) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (nq) *nq = r->r.nq;
    if (total) *total = r->r.total;
    return VQHIP_OK;
}

int vqhip_range_read(const vqhip_range *r, uint64_t *lims, uint32_t *idx, float *dist) {
    VQ_API_BEGIN
    if (!r) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    if (lims) VQ_HIP(hipMemcpyAsync(lims, r->r.lims.p, ((size_t)r->r.nq + 1) * 8, hipMemcpyDeviceToHost, s));
    if (idx && r->r.total) VQ_HIP(hipMemcpyAsync(idx, r->r.idx.p, (size_t)r->r.total * 4, hipMemcpyDeviceToHost, s));
    if (dist && r->r.total) VQ_HIP(hipMemcpyAsync(dist, r->r.dist.p, (size_t)r->r.total * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_range_device(const vqhip_range *r, const void **dev_lims, const void **dev_idx, const void **dev_dist) {
    if (!r) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (dev_lims) *dev_lims = r->r.lims.p;
    if (dev_idx) *dev_idx = r->r.idx.p;
    if (dev_dist) *dev_dist = r->r.dist.p;
    return VQHIP_OK;
}

int vqhip_range_destroy(vqhip_range *r) {
    delete r;
    return VQHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ binary index (k_binary.hip) ----
static constexpr uint32_t kBinaryBatch = 1024;  // queries per internal batch

struct vqhip_binary : Resident {
    uint32_t W = 0, low = 0, high = 1;
    float thr = 0;
    DevBuf words, table;                 // [n][W] packed rows, S [d + 1]
    DevBuf qw, hist, sel, adc_sel, cnt;  // per-call workspaces
    DevBuf hcut, range_ws;               // range search: the clamped radii, the stage's counts and offsets
    std::vector<uint32_t> h_hcut;        // the host side of hcut (the source of an asynchronous copy)
    DevBuf mask_ws;                      // a filtered host call's row mask on the device
    const uint32_t *mask = nullptr;      // the row mask of the filtered call that holds the lock (MaskScope), NULL otherwise

    DevBuf &payload() { return words; }  // (`bytes` is the capacity: an add grows it)
    size_t row_bytes() const { return (size_t)W * 4; }
    DevBuf *norm_buf() { return nullptr; }
    int norms_enqueue(const void *, uint64_t, float *, hipStream_t) { return VQHIP_OK; }

    // a host form's mask, ceil(n / 32) words, up into mask_ws
    int stage_mask(const uint32_t *allowed, hipStream_t s) {
        const size_t mask_b = (size_t)((n + 31) / 32) * 4;
        VQ_TRY(mask_ws.ensure(mask_b));
        VQ_HIP(hipMemcpyAsync(mask_ws.p, allowed, mask_b, hipMemcpyHostToDevice, s));
        return VQHIP_OK;
    }

    // queries_dev [nq][d] f32 on the device -> [nq][topk] results on the device, enqueued on s in batches of 1024
    int search_enqueue(const float *queries_dev, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev, hipStream_t s) {
        const uint32_t qb = std::min(nq, kBinaryBatch);
        VQ_TRY(qw.ensure((size_t)qb * W * 4));
        VQ_TRY(hist.ensure(binary_hist_bytes(qb, d)));
        VQ_TRY(sel.ensure((size_t)qb * sizeof(BinSel)));
        VQ_TRY(adc_sel.ensure((size_t)qb * 8));
        VQ_TRY(cnt.ensure((size_t)qb * 4));
        VQ_TRY(cand.ensure(topk_cand_bytes(qb)));
        for (uint32_t q0 = 0; q0 < nq; q0 += qb) {
            const uint32_t nb = std::min(qb, nq - q0);
            VQ_TRY(launch_bq_pack(queries_dev + (size_t)q0 * d, VQHIP_BINARY_F32, nb, d, thr, high, qw.as<uint32_t>(), s));
            VQ_TRY(launch_binary_search(words.as<uint32_t>(), n, d, metric, table.as<float>(), qw.as<uint32_t>(), nb, topk,
                                        hist.as<uint32_t>(), sel.as<BinSel>(), adc_sel.as<uint32_t>(), cnt.as<uint32_t>(),
                                        cand.as<unsigned long long>(), idx_dev + (size_t)q0 * topk, dist_dev + (size_t)q0 * topk, s, mask));
        }
        return VQHIP_OK;
    }
};

// One Hamming-radius range call on a binary index: the radii, clamped to d and padded by a query group, go up, and
// launch_binary_range leaves the result complete.  masked: a filtered call under the row mask `allowed`, as range_search
// takes it (a host form's is staged into mask_ws; the pointer is checked behind range_args and before the handle).
static int binary_range(vqhip_binary *b, const void *queries, bool host, uint32_t nq, const uint32_t *hradii, uint64_t max_results,
                        vqhip_range **out, bool masked = false, const uint32_t *allowed = nullptr) {
    if (masked) {
        VQ_TRY(range_args(queries, hradii, nq, max_results, out));
        if (!allowed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
        if (!host) VQ_TRY(check_mask_aligned(allowed));
    }
    return range_enter(b, queries, host, nq, hradii, max_results, out, no_checks, [&](const float *qdev, RangeOut *r, hipStream_t s) -> int {
        if (masked && host) VQ_TRY(b->stage_mask(allowed, s));
        MaskScope scope(b->mask, !masked ? nullptr : host ? b->mask_ws.as<uint32_t>() : allowed);
        b->h_hcut.assign((size_t)nq + 32, 0u);
        for (uint32_t q = 0; q < nq; ++q) b->h_hcut[q] = std::min(hradii[q], b->d);
        VQ_TRY(b->hcut.ensure(b->h_hcut.size() * 4));
        VQ_HIP(hipMemcpyAsync(b->hcut.p, b->h_hcut.data(), b->h_hcut.size() * 4, hipMemcpyHostToDevice, s));
        VQ_TRY(b->qw.ensure((size_t)binary_range_batch(b->n, b->d, nq) * b->W * 4));
        VQ_TRY(b->range_ws.ensure(binary_range_ws_bytes(b->n, b->d, nq)));
        return launch_binary_range(b->words.as<uint32_t>(), b->n, b->d, b->metric, b->table.as<float>(), qdev, b->thr, b->high, nq,
                                   b->hcut.as<uint32_t>(), max_results, b->qw.as<uint32_t>(), b->range_ws.p, r, s, b->mask);
    });
}

// ---- the three source kinds of packed rows (vqhip_binary's and vqhip_abin's create and add) ----
static int bits_check_kind(int kind) {
    if (kind != VQHIP_BINARY_F32 && kind != VQHIP_BINARY_U8 && kind != VQHIP_BINARY_PACKED)
        return fail(VQHIP_ERR_INVALID_INPUT, "source kind must be 0 (f32), 1 (u8 codes) or 2 (packed words), not %d", kind);
    return VQHIP_OK;
}

// a device source of f32 rows or packed words is read as dwords
static int bits_check_aligned(const void *dev_src, int kind) {
    if (kind == VQHIP_BINARY_F32 && (reinterpret_cast<uintptr_t>(dev_src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, "rows are not 4-byte aligned");
    if (kind == VQHIP_BINARY_PACKED && (reinterpret_cast<uintptr_t>(dev_src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, "words are not 4-byte aligned");
    return VQHIP_OK;
}

// host words [n][W]: no pad bit may be set (added: the rows of an add, named so in the message)
static int bits_check_pad(const void *src, uint64_t n, uint32_t d, bool added) {
    if (d % 32 == 0) return VQHIP_OK;
    const uint32_t W = bin_words(d);
    const uint32_t *w = static_cast<const uint32_t *>(src), mask = (1u << (d % 32)) - 1u;
    for (uint64_t i = 0; i < n; ++i)
        if (w[i * W + W - 1] & ~mask)
            return fail(VQHIP_ERR_INVALID_INPUT, added ? "added row %llu has a pad bit set" : "row %llu has a pad bit set", (unsigned long long)i);
    return VQHIP_OK;
}

// n rows of `kind` from host (kind_copy = H2D) or device memory as packed words at dst [n][W] on the device: words are
// copied (a device source's pad bits checked behind the copy, which waits for s), rows and codes packed by the bit rule
// (thr, high) -- host ones a piece at a time
static int bits_store(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n, uint32_t d, float thr, uint32_t high,
                      uint32_t *dst, bool added, hipStream_t s) {
    const uint32_t W = bin_words(d);
    if (kind == VQHIP_BINARY_PACKED) {
        VQ_HIP(hipMemcpyAsync(dst, src, (size_t)n * W * 4, kind_copy, s));
        if (kind_copy == hipMemcpyDeviceToDevice && d % 32) {
            DevBuf bad;
            uint32_t h_bad = 0;
            VQ_TRY(bad.alloc(4));
            VQ_HIP(hipMemsetAsync(bad.p, 0, 4, s));
            VQ_TRY(launch_bin_padcheck(dst, n, d, bad.as<uint32_t>(), s));
            VQ_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
            VQ_HIP(hipStreamSynchronize(s));
            if (h_bad) return fail(VQHIP_ERR_INVALID_INPUT, added ? "an added packed row has a pad bit set" : "a packed row has a pad bit set");
        }
        return VQHIP_OK;
    }
    if (kind_copy == hipMemcpyDeviceToDevice) return launch_bq_pack(src, kind, n, d, thr, high, dst, s);
    return staged_rows(src, n, (size_t)d * (kind == VQHIP_BINARY_U8 ? 1 : 4), s, [&](const void *piece, uint64_t r0, uint64_t rn) {
        return launch_bq_pack(piece, kind, rn, d, thr, high, dst + r0 * W, s);
    });
}

// what an add checks of its source before the handle's lock: the kind, a device source's alignment, a host source's pad bits
static int bits_check_add(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n_add, uint32_t d) {
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    VQ_TRY(bits_check_kind(kind));
    const bool dev = kind_copy == hipMemcpyDeviceToDevice;
    if (dev) VQ_TRY(bits_check_aligned(src, kind));
    if (kind == VQHIP_BINARY_PACKED && !dev) VQ_TRY(bits_check_pad(src, n_add, d, true));
    return VQHIP_OK;
}

static int binary_check(int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high, int metric) {
    VQ_TRY(bits_check_kind(kind));
    if (d == 0 || d > VQHIP_BINARY_MAX_DIM) return fail(VQHIP_ERR_INVALID_INPUT, "d %u must be in [1, 8192]", d);
    VQ_TRY(check_rows(n));
    VQ_TRY(bq_check(threshold, low, high));
    if (vq_is_cos(metric)) return fail(VQHIP_ERR_UNSUPPORTED, "cosine is not a function of the Hamming distance alone");
    return check_metric(metric);
}

static int binary_create(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n, uint32_t d, float threshold,
                         uint32_t low, uint32_t high, int metric, vqhip_binary **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    VQ_TRY(binary_check(kind, n, d, threshold, low, high, metric));
    const uint32_t W = bin_words(d);
    if (kind == VQHIP_BINARY_PACKED && kind_copy == hipMemcpyHostToDevice) VQ_TRY(bits_check_pad(src, n, d, false));
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_binary> b(new vqhip_binary());
    b->n = n, b->d = d, b->W = W, b->low = low, b->high = high, b->thr = threshold, b->metric = metric;
    std::vector<float> S(d + 1);
    binary_table(d, low, high, metric, S.data());
    VQ_TRY(b->table.alloc((size_t)(d + 1) * 4));
    VQ_HIP(hipMemcpyAsync(b->table.p, S.data(), (size_t)(d + 1) * 4, hipMemcpyHostToDevice, s));
    VQ_TRY(b->words.alloc((size_t)n * W * 4));
    VQ_TRY(bits_store(src, kind_copy, kind, n, d, threshold, high, b->words.as<uint32_t>(), false, s));
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its source once this returns
    *out = b.release();
    return VQHIP_OK;
}

// n_add rows of `kind` (vqhip_binary_create's three) behind the last, with create's checks of the source
static int binary_add(vqhip_binary *b, const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n_add) {
    if (!b) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    VQ_TRY(bits_check_add(src, kind_copy, kind, n_add, b->d));  // (d is fixed at create)
    return resident_add(b, src, n_add, [&](char *dst, hipStream_t s) -> int {
        return bits_store(src, kind_copy, kind, n_add, b->d, b->thr, b->high, reinterpret_cast<uint32_t *>(dst), true, s);
    });
}

extern "C" {

int vqhip_bq_pack(float threshold, const float *x, uint64_t n, uint32_t d, uint32_t *words) {
    VQ_API_BEGIN
    VQ_TRY(bq_check(threshold, 0, 1));
    if (n == 0) return VQHIP_OK;
    if (d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "d must be at least 1");
    if (!x || !words) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    const uint32_t W = bin_words(d);
    const size_t row_b = (size_t)d * 4;
    DevBuf dw;
    VQ_TRY(dw.alloc((size_t)std::min<uint64_t>(std::max<uint64_t>(1, kStageBytes / row_b), n) * W * 4));
    return staged_rows(x, n, row_b, s, [&](const void *piece, uint64_t r0, uint64_t rn) -> int {
        VQ_TRY(launch_bq_pack(piece, VQHIP_BINARY_F32, rn, d, threshold, 1, dw.as<uint32_t>(), s));
        VQ_HIP(hipMemcpyAsync(words + r0 * W, dw.p, (size_t)rn * W * 4, hipMemcpyDeviceToHost, s));
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_bq_pack_device(float threshold, const void *dev_x, uint64_t n, uint32_t d, void *dev_words) {
    VQ_API_BEGIN
    VQ_TRY(bq_check(threshold, 0, 1));
    if (n == 0) return VQHIP_OK;
    if (d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "d must be at least 1");
    if (!dev_x || !dev_words) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (reinterpret_cast<uintptr_t>(dev_x) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "x is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_words) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "words is not 4-byte aligned");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    return launch_bq_pack(dev_x, VQHIP_BINARY_F32, n, d, threshold, 1, static_cast<uint32_t *>(dev_words), s);
    VQ_API_END
}

int vqhip_binary_create(const void *src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high,
                        int metric, vqhip_binary **out) {
    VQ_API_BEGIN
    return binary_create(src, hipMemcpyHostToDevice, kind, n, d, threshold, low, high, metric, out);
    VQ_API_END
}

int vqhip_binary_create_device(const void *dev_src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low,
                               uint32_t high, int metric, vqhip_binary **out) {
    VQ_API_BEGIN
    VQ_TRY(bits_check_aligned(dev_src, kind));
    return binary_create(dev_src, hipMemcpyDeviceToDevice, kind, n, d, threshold, low, high, metric, out);
    VQ_API_END
}

int vqhip_binary_destroy(vqhip_binary *b) {
    delete b;
    return VQHIP_OK;
}

int vqhip_binary_info(const vqhip_binary *b, uint64_t *n, uint32_t *d, float *threshold, uint32_t *low, uint32_t *high,
                      int *metric) {
    if (!b) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n) *n = b->n;
    if (d) *d = b->d;
    if (threshold) *threshold = b->thr;
    if (low) *low = b->low;
    if (high) *high = b->high;
    if (metric) *metric = b->metric;
    return VQHIP_OK;
}

int vqhip_binary_add(vqhip_binary *b, const void *src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return binary_add(b, src, hipMemcpyHostToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_binary_add_device(vqhip_binary *b, const void *dev_src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return binary_add(b, dev_src, hipMemcpyDeviceToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_binary_remove(vqhip_binary *b, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(b, remove_words, true, removed);
    VQ_API_END
}

int vqhip_binary_remove_device(vqhip_binary *b, const uint32_t *dev_remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(b, dev_remove_words, false, removed);
    VQ_API_END
}

int vqhip_binary_packed(vqhip_binary *b, uint32_t *words) {
    VQ_API_BEGIN
    return resident_enter(b, words != nullptr, no_checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        VQ_HIP(hipMemcpyAsync(words, b->words.p, (size_t)b->n * b->W * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_binary_search(vqhip_binary *b, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return resident_search(b, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_binary_search_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return resident_search_device(b, dev_queries, nq, topk, dev_idx, dev_dist);
    VQ_API_END
}

uint64_t vqhip_binary_masked_slice(uint64_t n, uint32_t groups) { return n ? binary_masked_slice(n, groups) : 0; }

int vqhip_binary_search_masked(vqhip_binary *b, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                               uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_search_masked(b, queries, nq, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_binary_search_masked_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return exact_search_masked_device(b, dev_queries, nq, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_binary_range_search_masked(vqhip_binary *b, const float *queries, uint32_t nq, const uint32_t *hradii,
                                     uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return binary_range(b, queries, true, nq, hradii, max_results, out, true, allowed);
    VQ_API_END
}

int vqhip_binary_range_search_masked_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, const uint32_t *hradii,
                                            uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return binary_range(b, dev_queries, false, nq, hradii, max_results, out, true, dev_allowed);
    VQ_API_END
}

int vqhip_binary_range_search(vqhip_binary *b, const float *queries, uint32_t nq, const uint32_t *hradii, uint64_t max_results,
                              vqhip_range **out) {
    VQ_API_BEGIN
    return binary_range(b, queries, true, nq, hradii, max_results, out);
    VQ_API_END
}

int vqhip_binary_range_search_device(vqhip_binary *b, const void *dev_queries, uint32_t nq, const uint32_t *hradii,
                                     uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return binary_range(b, dev_queries, false, nq, hradii, max_results, out);
    VQ_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ asymmetric binary index (k_abin.hip) ----
// The binary index's packed rows under the exact distances of the flat and the scalar index: f32 queries against
// v(bit) = bit ? high : low.  The third member of ExactResident.
struct vqhip_abin : ExactResident<vqhip_abin> {
    uint32_t W = 0, low = 0, high = 1;
    float thr = 0;
    DevBuf words;  // [n][W] packed rows; `bytes` is the capacity (an add grows it)

    float lo() const { return (float)low; }
    float hi() const { return (float)high; }
    DevBuf &payload() { return words; }
    size_t row_bytes() const { return (size_t)W * 4; }
    int norms_enqueue(const void *P, uint64_t count, float *out, hipStream_t s) {
        return launch_abin_norms(static_cast<const uint32_t *>(P), count, d, lo(), hi(), out, s);
    }
    int launch_search(const float *queries_dev, const float *qn, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                      hipStream_t s) {
        return launch_abin_search(metric, words.as<uint32_t>(), n, d, lo(), hi(), rnorm.as<float>(), queries_dev, qn, nq, topk,
                                  dist.as<float>(), state.p, cand.as<unsigned long long>(), idx_dev, dist_dev, mask, s);
    }
    int launch_rerank(const float *qn, uint32_t nq, uint32_t c, uint32_t topk, hipStream_t s) {
        return launch_abin_rerank(metric, words.as<uint32_t>(), n, d, lo(), hi(), rnorm.as<float>(), q.as<float>(), qn, nq,
                                  rr_cand.as<uint32_t>(), c, topk, idx.as<uint32_t>(), out.as<float>(), rr_err.as<uint32_t>(), s);
    }
    int launch_range(const float *queries_dev, const float *qn, uint32_t nq, uint64_t max_results, RangeOut *r, hipStream_t s) {
        return launch_abin_range(metric, words.as<uint32_t>(), n, d, lo(), hi(), rnorm.as<float>(), queries_dev, qn, nq, radii.as<float>(),
                                 max_results, dist.as<float>(), state.p, range_ws.p, r, mask, s);
    }
};

// vqhip_binary_create's sources and checks, but for the metric: every one of the five, cosine included
static int abin_create(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low,
                       uint32_t high, int metric, vqhip_abin **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    VQ_TRY(bits_check_kind(kind));
    if (d == 0 || d > VQHIP_BINARY_MAX_DIM) return fail(VQHIP_ERR_INVALID_INPUT, "d %u must be in [1, 8192]", d);
    VQ_TRY(check_rows(n));
    VQ_TRY(bq_check(threshold, low, high));
    VQ_TRY(check_metric(metric));
    if (kind == VQHIP_BINARY_PACKED && kind_copy == hipMemcpyHostToDevice) VQ_TRY(bits_check_pad(src, n, d, false));
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_abin> x(new vqhip_abin());
    x->n = n, x->d = d, x->W = bin_words(d), x->low = low, x->high = high, x->thr = threshold, x->metric = metric;
    VQ_TRY(x->words.alloc((size_t)n * x->W * 4));
    VQ_TRY(bits_store(src, kind_copy, kind, n, d, threshold, high, x->words.as<uint32_t>(), false, s));
    if (vq_is_cos(metric)) {
        VQ_TRY(x->rnorm.alloc((size_t)n * 4));
        VQ_TRY(x->norms_enqueue(x->words.p, n, x->rnorm.as<float>(), s));
    }
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its source once this returns
    *out = x.release();
    return VQHIP_OK;
}

// n_add rows of `kind` behind the last, with create's checks of the source
static int abin_add(vqhip_abin *x, const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n_add) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    VQ_TRY(bits_check_add(src, kind_copy, kind, n_add, x->d));  // (d is fixed at create)
    return resident_add(x, src, n_add, [&](char *dst, hipStream_t s) -> int {
        return bits_store(src, kind_copy, kind, n_add, x->d, x->thr, x->high, reinterpret_cast<uint32_t *>(dst), true, s);
    });
}

extern "C" {

int vqhip_abin_create(const void *src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high, int metric,
                      vqhip_abin **out) {
    VQ_API_BEGIN
    return abin_create(src, hipMemcpyHostToDevice, kind, n, d, threshold, low, high, metric, out);
    VQ_API_END
}

int vqhip_abin_create_device(const void *dev_src, int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high,
                             int metric, vqhip_abin **out) {
    VQ_API_BEGIN
    VQ_TRY(bits_check_aligned(dev_src, kind));
    return abin_create(dev_src, hipMemcpyDeviceToDevice, kind, n, d, threshold, low, high, metric, out);
    VQ_API_END
}

int vqhip_abin_destroy(vqhip_abin *x) {
    delete x;
    return VQHIP_OK;
}

int vqhip_abin_info(const vqhip_abin *x, uint64_t *n, uint32_t *d, float *threshold, uint32_t *low, uint32_t *high, int *metric) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n) *n = x->n;
    if (d) *d = x->d;
    if (threshold) *threshold = x->thr;
    if (low) *low = x->low;
    if (high) *high = x->high;
    if (metric) *metric = x->metric;
    return VQHIP_OK;
}

int vqhip_abin_packed(vqhip_abin *x, uint32_t *words) {
    VQ_API_BEGIN
    return resident_enter(x, words != nullptr, no_checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        VQ_HIP(hipMemcpyAsync(words, x->words.p, (size_t)x->n * x->W * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_abin_search(vqhip_abin *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return resident_search(x, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_abin_search_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return resident_search_device(x, dev_queries, nq, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_abin_search_masked(vqhip_abin *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                             uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_search_masked(x, queries, nq, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_abin_search_masked_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, uint32_t topk, const uint32_t *dev_allowed,
                                    void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return exact_search_masked_device(x, dev_queries, nq, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_abin_rerank(vqhip_abin *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk,
                      uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_rerank(x, queries, nq, cand, c, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_abin_range_search(vqhip_abin *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                            vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_abin_range_search_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_abin_range_search_masked(vqhip_abin *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                   const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out, true, allowed);
    VQ_API_END
}

int vqhip_abin_range_search_masked_device(vqhip_abin *x, const void *dev_queries, uint32_t nq, const float *radii,
                                          uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out, true, dev_allowed);
    VQ_API_END
}

int vqhip_abin_add(vqhip_abin *x, const void *src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return abin_add(x, src, hipMemcpyHostToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_abin_add_device(vqhip_abin *x, const void *dev_src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return abin_add(x, dev_src, hipMemcpyDeviceToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_abin_remove(vqhip_abin *x, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, remove_words, true, removed);
    VQ_API_END
}

int vqhip_abin_remove_device(vqhip_abin *x, const uint32_t *dev_remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, dev_remove_words, false, removed);
    VQ_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ 4-bit scalar index (k_sq4index.hip) ----
// The scalar index's codes at four bits a dimension, eight to a word, under the same exact distances: f32 queries against
// v(c) = min + (float)c * step.  The fourth member of ExactResident.
struct vqhip_sq4index : ExactResident<vqhip_sq4index> {
    uint32_t W = 0, levels = 0;
    float mn = 0, mx = 0, step = 0;
    DevBuf words;  // [n][W] packed rows; `bytes` is the capacity (an add grows it)

    DevBuf &payload() { return words; }
    size_t row_bytes() const { return (size_t)W * 4; }
    int norms_enqueue(const void *P, uint64_t count, float *out, hipStream_t s) {
        return launch_sq4_norms(static_cast<const uint32_t *>(P), count, d, mn, step, out, s);
    }
    int launch_search(const float *queries_dev, const float *qn, uint32_t nq, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                      hipStream_t s) {
        return launch_sq4_search(metric, words.as<uint32_t>(), n, d, mn, step, rnorm.as<float>(), queries_dev, qn, nq, topk,
                                 dist.as<float>(), state.p, cand.as<unsigned long long>(), idx_dev, dist_dev, mask, s);
    }
    int launch_rerank(const float *qn, uint32_t nq, uint32_t c, uint32_t topk, hipStream_t s) {
        return launch_sq4_rerank(metric, words.as<uint32_t>(), n, d, mn, step, rnorm.as<float>(), q.as<float>(), qn, nq,
                                 rr_cand.as<uint32_t>(), c, topk, idx.as<uint32_t>(), out.as<float>(), rr_err.as<uint32_t>(), s);
    }
    int launch_range(const float *queries_dev, const float *qn, uint32_t nq, uint64_t max_results, RangeOut *r, hipStream_t s) {
        return launch_sq4_range(metric, words.as<uint32_t>(), n, d, mn, step, rnorm.as<float>(), queries_dev, qn, nq, radii.as<float>(),
                                max_results, dist.as<float>(), state.p, range_ws.p, r, mask, s);
    }
};

static int sq4_check_levels(uint32_t levels) {
    if (levels > 16) return fail(VQHIP_ERR_INVALID_INPUT, "levels %u: a 4-bit index holds at most 16", levels);
    return VQHIP_OK;
}

// What create and add check of their source without a device: the pointer, the kind, a device source's alignment (f32
// rows and words are read as dwords), a host source's codes (at most 15) and pad nibbles (zero).
static int sq4_check_source(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n, uint32_t d, bool added) {
    if (kind != VQHIP_SQ4_F32 && kind != VQHIP_SQ4_U8 && kind != VQHIP_SQ4_PACKED)
        return fail(VQHIP_ERR_INVALID_INPUT, "source kind must be 0 (f32), 1 (u8 codes) or 2 (packed words), not %d", kind);
    if (kind_copy == hipMemcpyDeviceToDevice) {
        if (kind == VQHIP_SQ4_F32 && (reinterpret_cast<uintptr_t>(src) & 3)) return fail(VQHIP_ERR_INVALID_INPUT, "rows are not 4-byte aligned");
        if (kind == VQHIP_SQ4_PACKED && (reinterpret_cast<uintptr_t>(src) & 3))
            return fail(VQHIP_ERR_INVALID_INPUT, "words are not 4-byte aligned");
        return VQHIP_OK;
    }
    if (kind == VQHIP_SQ4_U8) {
        const uint8_t *c = static_cast<const uint8_t *>(src);
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t t = 0; t < d; ++t)
                if (c[i * d + t] > 15)
                    return fail(VQHIP_ERR_INVALID_INPUT, added ? "added row %llu holds code %u: a 4-bit code is at most 15" : "row %llu holds code %u: a 4-bit code is at most 15",
                                (unsigned long long)i, (unsigned)c[i * d + t]);
    } else if (kind == VQHIP_SQ4_PACKED && d % 8) {
        const uint32_t W = sq4_words(d);
        const uint32_t *w = static_cast<const uint32_t *>(src), keep = (1u << (4 * (d % 8))) - 1u;
        for (uint64_t i = 0; i < n; ++i)
            if (w[i * W + W - 1] & ~keep)
                return fail(VQHIP_ERR_INVALID_INPUT, added ? "added row %llu has a pad nibble set" : "row %llu has a pad nibble set", (unsigned long long)i);
    }
    return VQHIP_OK;
}

// n rows of `kind` from host (kind_copy = H2D) or device memory as packed words at dst [n][W] on the device.  Words are
// copied; codes are packed; f32 rows are encoded a piece at a time into a buffer of codes and packed from there, so that
// only the words stay.  A device source of codes or words is checked behind the pack / the copy with a flag word read
// back (which waits for s).
static int sq4_store(const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n, uint32_t d, const SqbqEncodeOp &op, uint32_t *dst,
                     bool added, hipStream_t s) {
    const uint32_t W = sq4_words(d);
    const bool dev = kind_copy == hipMemcpyDeviceToDevice;
    DevBuf bad;
    VQ_TRY(bad.alloc(4));
    VQ_HIP(hipMemsetAsync(bad.p, 0, 4, s));
    if (kind == VQHIP_SQ4_PACKED) {
        VQ_HIP(hipMemcpyAsync(dst, src, (size_t)n * W * 4, kind_copy, s));
        if (dev) VQ_TRY(launch_sq4_padcheck(dst, n, d, bad.as<uint32_t>(), s));
    } else if (kind == VQHIP_SQ4_U8) {
        if (dev) {
            VQ_TRY(launch_sq4_pack(static_cast<const uint8_t *>(src), n, d, dst, bad.as<uint32_t>(), s));
        } else {
            VQ_TRY(staged_rows(src, n, (size_t)d, s, [&](const void *piece, uint64_t r0, uint64_t rn) {
                return launch_sq4_pack(static_cast<const uint8_t *>(piece), rn, d, dst + r0 * W, bad.as<uint32_t>(), s);
            }));
        }
    } else {
        const uint64_t per = std::max<uint64_t>(1, kStageBytes / ((size_t)d * 4));  // (staged_rows' piece for rows of 4 d bytes)
        DevBuf codes;
        VQ_TRY(codes.alloc((size_t)std::min<uint64_t>(per, n) * d));
        auto piece = [&](const void *rows, uint64_t r0, uint64_t rn) -> int {
            VQ_TRY(launch_sqbq_encode(op, static_cast<const float *>(rows), rn * d, codes.as<uint8_t>(), s));
            return launch_sq4_pack(codes.as<uint8_t>(), rn, d, dst + r0 * W, bad.as<uint32_t>(), s);
        };
        if (dev) {
            for (uint64_t r0 = 0; r0 < n; r0 += per)  // (in stream order: the codes of a piece are packed before the next encode)
                VQ_TRY(piece(static_cast<const float *>(src) + r0 * d, r0, std::min<uint64_t>(per, n - r0)));
            VQ_HIP(hipStreamSynchronize(s));  // before `codes` is freed
        } else {
            VQ_TRY(staged_rows(src, n, (size_t)d * 4, s, piece));
        }
    }
    if (dev && kind != VQHIP_SQ4_F32) {
        uint32_t h_bad = 0;
        VQ_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        if (h_bad && kind == VQHIP_SQ4_U8)
            return fail(VQHIP_ERR_INVALID_INPUT, added ? "an added row holds a code above 15" : "a row holds a code above 15");
        if (h_bad) return fail(VQHIP_ERR_INVALID_INPUT, added ? "an added packed row has a pad nibble set" : "a packed row has a pad nibble set");
    }
    VQ_HIP(hipStreamSynchronize(s));  // before `bad` is freed
    return VQHIP_OK;
}

static int sq4index_create(const void *src, hipMemcpyKind kind_copy, int kind, float mn, float mx, uint32_t levels, uint64_t n,
                           uint32_t d, int metric, vqhip_sq4index **out) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    SqbqEncodeOp op;
    float step = 0;
    VQ_TRY(sq_check(mn, mx, levels, &step));
    VQ_TRY(sq4_check_levels(levels));
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    if (d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "d must be at least 1");
    VQ_TRY(check_rows(n));
    VQ_TRY(check_metric(metric));
    VQ_TRY(sq4_check_source(src, kind_copy, kind, n, d, false));
    VQ_TRY(sq_encode_op(mn, mx, levels, &op));
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_sq4index> x(new vqhip_sq4index());
    x->n = n, x->d = d, x->W = sq4_words(d), x->levels = levels, x->mn = mn, x->mx = mx, x->step = step, x->metric = metric;
    VQ_TRY(x->words.alloc((size_t)n * x->W * 4));
    VQ_TRY(sq4_store(src, kind_copy, kind, n, d, op, x->words.as<uint32_t>(), false, s));
    if (vq_is_cos(metric)) {
        VQ_TRY(x->rnorm.alloc((size_t)n * 4));
        VQ_TRY(x->norms_enqueue(x->words.p, n, x->rnorm.as<float>(), s));
    }
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its source once this returns
    *out = x.release();
    return VQHIP_OK;
}

// n_add rows of `kind` behind the last, with create's checks of the source
static int sq4index_add(vqhip_sq4index *x, const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n_add) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    VQ_TRY(sq4_check_source(src, kind_copy, kind, n_add, x->d, true));  // (d and the quantizer are fixed at create)
    SqbqEncodeOp op;
    VQ_TRY(sq_encode_op(x->mn, x->mx, x->levels, &op));
    return resident_add(x, src, n_add, [&](char *dst, hipStream_t s) -> int {
        return sq4_store(src, kind_copy, kind, n_add, x->d, op, reinterpret_cast<uint32_t *>(dst), true, s);
    });
}

extern "C" {

int vqhip_sq4index_create(float min, float max, uint32_t levels, const void *src, int kind, uint64_t n, uint32_t d, int metric,
                          vqhip_sq4index **out) {
    VQ_API_BEGIN
    return sq4index_create(src, hipMemcpyHostToDevice, kind, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sq4index_create_device(float min, float max, uint32_t levels, const void *dev_src, int kind, uint64_t n, uint32_t d,
                                 int metric, vqhip_sq4index **out) {
    VQ_API_BEGIN
    return sq4index_create(dev_src, hipMemcpyDeviceToDevice, kind, min, max, levels, n, d, metric, out);
    VQ_API_END
}

int vqhip_sq4index_destroy(vqhip_sq4index *x) {
    delete x;
    return VQHIP_OK;
}

int vqhip_sq4index_info(const vqhip_sq4index *x, uint64_t *n, uint32_t *d, int *metric, float *min, float *max, uint32_t *levels) {
    if (!x) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n) *n = x->n;
    if (d) *d = x->d;
    if (metric) *metric = x->metric;
    if (min) *min = x->mn;
    if (max) *max = x->mx;
    if (levels) *levels = x->levels;
    return VQHIP_OK;
}

int vqhip_sq4index_packed(vqhip_sq4index *x, uint32_t *words) {
    VQ_API_BEGIN
    return resident_enter(x, words != nullptr, no_checks, 1, nullptr, [&](Entry &in, hipStream_t s) -> int {
        VQ_HIP(hipMemcpyAsync(words, x->words.p, (size_t)x->n * x->W * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_sq4index_search(vqhip_sq4index *x, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return resident_search(x, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_sq4index_search_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, uint32_t topk, void *dev_idx,
                                 void *dev_dist) {
    VQ_API_BEGIN
    return resident_search_device(x, dev_queries, nq, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_sq4index_search_masked(vqhip_sq4index *x, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                                 uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_search_masked(x, queries, nq, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_sq4index_search_masked_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, uint32_t topk,
                                        const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return exact_search_masked_device(x, dev_queries, nq, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_sq4index_rerank(vqhip_sq4index *x, const float *queries, uint32_t nq, const uint32_t *cand, uint32_t c, uint32_t topk,
                          uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return exact_rerank(x, queries, nq, cand, c, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_sq4index_range_search(vqhip_sq4index *x, const float *queries, uint32_t nq, const float *radii, uint64_t max_results,
                                vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_sq4index_range_search_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, const float *radii,
                                       uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out);
    VQ_API_END
}

int vqhip_sq4index_range_search_masked(vqhip_sq4index *x, const float *queries, uint32_t nq, const float *radii,
                                       uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, queries, true, nq, radii, max_results, out, true, allowed);
    VQ_API_END
}

int vqhip_sq4index_range_search_masked_device(vqhip_sq4index *x, const void *dev_queries, uint32_t nq, const float *radii,
                                              uint64_t max_results, const uint32_t *dev_allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return range_search(x, dev_queries, false, nq, radii, max_results, out, true, dev_allowed);
    VQ_API_END
}

int vqhip_sq4index_add(vqhip_sq4index *x, const void *src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return sq4index_add(x, src, hipMemcpyHostToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_sq4index_add_device(vqhip_sq4index *x, const void *dev_src, int kind, uint64_t n_add) {
    VQ_API_BEGIN
    return sq4index_add(x, dev_src, hipMemcpyDeviceToDevice, kind, n_add);
    VQ_API_END
}

int vqhip_sq4index_remove(vqhip_sq4index *x, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, remove_words, true, removed);
    VQ_API_END
}

int vqhip_sq4index_remove_device(vqhip_sq4index *x, const uint32_t *dev_remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return resident_remove(x, dev_remove_words, false, removed);
    VQ_API_END
}

}  // extern "C"
