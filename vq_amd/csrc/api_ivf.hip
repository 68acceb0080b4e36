// api_ivf.hip -- extern "C" entry points of the inverted-file indexes (vqhip_ivfpq, vqhip_ivfflat, vqhip_ivfsq,
// vqhip_ivfsq4, vqhip_ivfbin) and their host layer: the inverted lists, probe, search, range search, add and remove.  Host-side
// orchestration only.
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "adc_plan.hpp"
#include "api_index.hpp"
#include "ivf_remove.hpp"

// ------------------------------------------------------------------ inverted lists: the shared host layer ----
// What vqhip_ivfpq, vqhip_ivfflat, vqhip_ivfsq, vqhip_ivfsq4 and vqhip_ivfbin have in common.  Host state: the coarse centroids and every added
// row's list id and payload (PQ codes, f32 / f16 elements, SQ codes, packed 4-bit SQ words or packed BQ words) in add order.  The device state -- a flat index
// over the centroids and the rows in list order (off / ids / payload) -- is built on the current device by the first
// probe or search and rebuilt there after an add: a host counting sort gives the order (O(n) per rebuild), and the
// payload goes up through a staging buffer of at most kIvfflatStage bytes, list order gathered a piece at a time.
constexpr size_t kIvfflatStage = 64u << 20;

struct IvfLists {
    HandleSync sync;
    uint32_t nlist = 0, dim = 0;
    int metric = VQHIP_EUCLIDEAN;
    int probe_metric = VQHIP_EUCLIDEAN;  // of the flat index over the centroids: `metric`, but for vqhip_ivfbin's coarse metric
    size_t row_b = 0;                // bytes of one row's payload (each index sets it at create)
    std::vector<float> coarse;       // [nlist][dim]
    std::vector<uint32_t> row_list;  // [n] list id of each row
    std::vector<uint8_t> payload;    // [n][row_b] in add order
    std::vector<uint64_t> sizes;     // [nlist] rows per list
    uint64_t n = 0, max_list = 0;
    bool dirty = true;                     // rows added since the last upload
    uint64_t uploads = 0;                  // times ivf_ready has built the device state from the host rows
    int dev = -1;                          // the device of the index's state: current at create (-1: create saw no device;
                                           // then the first probe or search takes the current one)
    std::vector<uint64_t> largest_prefix;  // [nlist + 1] sums of the largest list sizes (the bound on |S(q)|)
    vqhip_flat *flat = nullptr;            // the coarse centroids on the device
    DevBuf d_off, d_ids, d_payload;        // (d_payload is the index's own buffer: the loaders' alignment rests on its base)
    DevBuf q, probe, probe_dist, pref, seg, W, state, cand, idx, out;  // per-call workspaces
    ~IvfLists() { delete flat; }
    uint32_t width() const { return dim; }  // floats of a query
    // every device call runs on the index's device
    int on_device() {
        int cur = 0;
        VQ_HIP(hipGetDevice(&cur));
        if (dev < 0) dev = cur;
        if (cur != dev) return fail(VQHIP_ERR_INVALID_INPUT, "the index lives on device %d, but device %d is current", dev, cur);
        return VQHIP_OK;
    }
};

// the checks every create shares (each create keeps its own between them, in its documented order) and the shared fields
static int ivf_check_lists(const void *coarse, uint32_t nlist) {
    if (!coarse) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (nlist == 0 || nlist > 65536) return fail(VQHIP_ERR_INVALID_INPUT, "nlist %u must be in [1, 65536]", nlist);
    return VQHIP_OK;
}
static void ivf_init(IvfLists *ix, const float *coarse, uint32_t nlist, uint32_t dim, int metric, size_t row_b) {
    ix->nlist = nlist;
    ix->dim = dim;
    ix->metric = metric;
    ix->probe_metric = metric;
    ix->row_b = row_b;
    ix->coarse.assign(coarse, coarse + (size_t)nlist * dim);
    ix->sizes.assign(nlist, 0);
    int ndev = 0, cur = -1;  // (the device is named, not touched: the state is built by the first probe or search)
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipGetDevice(&cur) == hipSuccess) ix->dev = cur;
}

static int ivf_check_probe(const IvfLists *ix, uint32_t nprobe) {
    const uint32_t hi = std::min<uint32_t>(ix->nlist, 1024);
    if (nprobe == 0 || nprobe > hi) return fail(VQHIP_ERR_INVALID_INPUT, "nprobe %u must be in [1, min(nlist, 1024)] = [1, %u]", nprobe, hi);
    return VQHIP_OK;
}

// An add: the checks (before anything is stored), `store` appending the n rows to ix->payload -- or leaving it as it
// was and returning the error -- and the bookkeeping once they are there.
template <class F>
static int ivf_add(IvfLists *ix, const uint32_t *list_ids, const void *data, uint64_t n, F &&store) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n == 0) return VQHIP_OK;
    if (!list_ids || !data) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    if (n >= (1ull << 32) - ix->n)
        return fail(VQHIP_ERR_INVALID_INPUT, "the index would hold %llu + %llu rows: at most 2^32 - 1", (unsigned long long)ix->n,
                    (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (list_ids[i] >= ix->nlist)
            return fail(VQHIP_ERR_INVALID_INPUT, "list id %u of row %llu is outside [0, %u)", list_ids[i], (unsigned long long)i, ix->nlist);
    VQ_TRY(store());
    ix->row_list.insert(ix->row_list.end(), list_ids, list_ids + n);
    for (uint64_t i = 0; i < n; ++i) ++ix->sizes[list_ids[i]];
    ix->n += n;
    ix->dirty = true;
    return VQHIP_OK;
}
static int ivf_append(IvfLists *ix, const void *data, uint64_t n) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(data);
    ix->payload.insert(ix->payload.end(), p, p + (size_t)n * ix->row_b);
    return VQHIP_OK;
}

static int ivf_list_sizes(IvfLists *ix, uint64_t *sizes) {
    if (!ix || !sizes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    memcpy(sizes, ix->sizes.data(), ix->sizes.size() * 8);
    return VQHIP_OK;
}

// what the batches of a search are sized by, from the list sizes: the largest list and the sums of the largest ones
static void ivf_bounds(IvfLists *ix) {
    std::vector<uint64_t> sorted(ix->sizes);
    std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
    ix->max_list = sorted[0];
    ix->largest_prefix.assign(ix->nlist + 1, 0);
    for (uint32_t l = 0; l < ix->nlist; ++l) ix->largest_prefix[l + 1] = ix->largest_prefix[l] + sorted[l];
}

// The device state, current with the host's rows (enqueued on s and waited for: host buffers are the copies' sources).
// `first` runs once, after the coarse centroids are resident (an index's own tables); `resident` after every upload of a
// non-empty payload (what an index derives from it on the device).
template <class First, class Resident>
static int ivf_ready(IvfLists *ix, hipStream_t s, First &&first, Resident &&resident) {
    if (!ix->flat) {
        VQ_TRY(flat_create(ix->coarse.data(), hipMemcpyHostToDevice, ix->nlist, ix->dim, 0, ix->probe_metric, &ix->flat));
        VQ_TRY(first());
    }
    if (!ix->dirty) return VQHIP_OK;
    const size_t row_b = ix->row_b;
    std::vector<uint32_t> off(ix->nlist + 1, 0), at(ix->nlist), ids(ix->n);
    for (uint32_t l = 0; l < ix->nlist; ++l) off[l + 1] = off[l] + (uint32_t)ix->sizes[l];
    std::copy(off.begin(), off.end() - 1, at.begin());
    for (uint64_t i = 0; i < ix->n; ++i) ids[at[ix->row_list[i]]++] = (uint32_t)i;  // ascending row ids within each list
    VQ_TRY(ix->d_off.alloc(off.size() * 4));
    VQ_TRY(ix->d_ids.alloc(ids.size() * 4));
    VQ_TRY(ix->d_payload.alloc((size_t)ix->n * row_b));
    VQ_HIP(hipMemcpyAsync(ix->d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
    if (ix->n) {
        VQ_HIP(hipMemcpyAsync(ix->d_ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, s));
        const uint64_t per = std::max<uint64_t>(1, kIvfflatStage / row_b);
        std::vector<uint8_t> stage((size_t)std::min<uint64_t>(per, ix->n) * row_b);
        for (uint64_t p0 = 0; p0 < ix->n; p0 += per) {
            const uint64_t pn = std::min<uint64_t>(per, ix->n - p0);
            for (uint64_t p = 0; p < pn; ++p) memcpy(stage.data() + (size_t)p * row_b, ix->payload.data() + (size_t)ids[p0 + p] * row_b, row_b);
            VQ_HIP(hipMemcpyAsync(ix->d_payload.as<uint8_t>() + (size_t)p0 * row_b, stage.data(), (size_t)pn * row_b, hipMemcpyHostToDevice, s));
            VQ_HIP(hipStreamSynchronize(s));  // (the staging buffer is filled again)
        }
        VQ_TRY(resident());
    }
    VQ_HIP(hipStreamSynchronize(s));
    ivf_bounds(ix);
    ix->dirty = false;
    ++ix->uploads;
    return VQHIP_OK;
}
static int ivf_no_hook() { return VQHIP_OK; }

// queries_dev [nq][dim] f32 -> probe lists [nq][nprobe] on the device
static int ivf_probe_enqueue(IvfLists *ix, const float *queries_dev, uint32_t nq, uint32_t nprobe, uint32_t *lists_dev, hipStream_t s) {
    VQ_TRY(ix->probe_dist.ensure((size_t)nq * nprobe * 4));
    return ix->flat->search_enqueue(queries_dev, nq, nprobe, lists_dev, ix->probe_dist.as<float>(), s);
}

// Batches of queries bound a search's workspace: the distances of a batch (4 bytes per position of S(q), sized by the
// nprobe largest lists) under 1 GB -- or one query's when that alone is more -- its tables (query_bytes each, if any)
// under 256 MB -- or one query's -- and at most 1024 queries.  Sizes the workspaces every index has, `state` apart.
struct IvfBatch {
    uint64_t wstride;  // floats of W per query
    uint32_t nb_max;   // queries per batch
    uint64_t per_q;    // expected positions per query: the mean list size times nprobe
};
static int ivf_batch(IvfLists *ix, uint32_t nq, uint32_t nprobe, uint64_t query_bytes, IvfBatch *b) {
    b->wstride = std::max<uint64_t>(ix->largest_prefix[nprobe], 1);
    uint64_t qb = std::min<uint64_t>({(uint64_t)nq, 1024, std::max<uint64_t>(1, (1ull << 30) / (4 * b->wstride))});
    if (query_bytes) qb = std::min(qb, std::max<uint64_t>(1, (256ull << 20) / query_bytes));
    b->nb_max = (uint32_t)qb;
    b->per_q = std::max<uint64_t>(1, (uint64_t)((double)ix->n * nprobe / ix->nlist));
    VQ_TRY(ix->probe.ensure((size_t)b->nb_max * nprobe * 4));
    VQ_TRY(ix->pref.ensure((size_t)b->nb_max * (nprobe + 1) * 4));
    VQ_TRY(ix->seg.ensure((size_t)b->nb_max * nprobe * 4));
    VQ_TRY(ix->W.ensure((size_t)b->nb_max * b->wstride * 4));
    VQ_TRY(ix->cand.ensure(topk_cand_bytes(b->nb_max)));
    return VQHIP_OK;
}

// IvfView: the inverted file of a filtered call's allowed rows on the device (ivf_view.hpp; launch_ivf_view) -- what a
// batch's view takes in place of d_off / d_ids, and the positions of its rows in the payload.  All NULL: every row.
struct IvfView {
    const uint32_t *pick = nullptr, *aids = nullptr, *aoff = nullptr;
};

// IvfLists with a filtered call's view (DESIGN.md sections 23 to 25): what vqhip_ivfpq and IvfOverW's three share.
struct IvfFiltered : IvfLists {
    DevBuf mask_ws;                       // a filtered host call's row mask on the device
    DevBuf v_pick, v_aids, v_aoff, v_ws;  // a filtered call's view (8 bytes per row) and the workspace of its scan
    DevBuf rm_prefix;                     // a removal's removed rows below every mask word (ivf_remove)
    DevBuf *norm_buf() { return nullptr; }  // the rows' norms on the device, where an index keeps them

    // The view of a filtered call, built once per call: after ready(s), under the handle's lock, enqueued on s.  allowed:
    // the row mask, ceil(n / 32) words for the n of this call -- a host form's goes up into mask_ws first.
    int filtered(const uint32_t *allowed, bool host, hipStream_t s, IvfView *view) {
        const uint64_t n = this->n;
        if (host) {
            const size_t mask_b = (size_t)((n + 31) / 32) * 4;
            VQ_TRY(mask_ws.ensure(mask_b));
            if (mask_b) VQ_HIP(hipMemcpyAsync(mask_ws.p, allowed, mask_b, hipMemcpyHostToDevice, s));
            allowed = mask_ws.as<uint32_t>();
        }
        VQ_TRY(v_pick.ensure((size_t)n * 4));
        VQ_TRY(v_aids.ensure((size_t)n * 4));
        VQ_TRY(v_aoff.ensure(((size_t)this->nlist + 1) * 4));
        VQ_TRY(v_ws.ensure(ivf_view_ws_bytes(n)));
        VQ_TRY(launch_ivf_view(allowed, this->d_ids.template as<uint32_t>(), n, this->d_off.template as<uint32_t>(), this->nlist, v_ws.p,
                               v_pick.as<uint32_t>(), v_aids.as<uint32_t>(), v_aoff.as<uint32_t>(), s));
        *view = IvfView{v_pick.as<uint32_t>(), v_aids.as<uint32_t>(), v_aoff.as<uint32_t>()};
        return VQHIP_OK;
    }
};

// the host rows without the removed ones, in place and in order: row_list, payload, sizes, n.  Nothing here can fail.
static void ivf_remove_host(IvfLists *ix, const uint32_t *remove, uint64_t na) {
    const size_t row_b = ix->row_b;
    uint64_t j = 0;
    for (uint64_t i = 0; i < ix->n; ++i) {
        if ((remove[i >> 5] >> (i & 31)) & 1u) {
            --ix->sizes[ix->row_list[i]];
            continue;
        }
        if (j != i) {
            ix->row_list[j] = ix->row_list[i];
            memcpy(ix->payload.data() + (size_t)j * row_b, ix->payload.data() + (size_t)i * row_b, row_b);  // (j < i: no overlap)
        }
        ++j;
    }
    ix->row_list.resize(na);
    ix->payload.resize((size_t)na * row_b);
    ix->n = na;
}

// A removal (include/vqhip.h, "removing rows from an inverted file"): `remove` is a host mask of
// ceil(n / 32) words.  Without a current device state the host rows are compacted and no device is touched.  With one,
// the state stays current: the view of the surviving rows (launch_ivf_view over the complement of the mask) is their
// inverted file with the old ids, k_ivf_take moves the payload (and the norms, T::norm_buf()) behind its `pick` into new
// allocations, k_ivf_renumber gives the ids their new numbers, and the buffers are swapped in once everything that can
// fail has run; the host rows follow.  The host knows the survivors' count and every list's size: nothing is read back.
template <class T>
static int ivf_remove(T *ix, const uint32_t *remove, uint64_t *removed) {
    if (!ix || !remove || !removed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *removed = 0;
    Entry in(ix->sync);
    const uint64_t n = ix->n, words = (n + 31) / 32;
    if (!ix->flat || ix->dirty) {  // no device state to keep current
        uint64_t na = 0;
        for (uint64_t w = 0; w < words; ++w) na += compact_popc32(compact_keep_word(remove[w], w, n));
        if (na != n) ivf_remove_host(ix, remove, na);
        *removed = n - na;
        return VQHIP_OK;
    }
    std::vector<uint32_t> prefix(words), allowed(words);
    const uint64_t gone = ivf_below_prefix(remove, n, prefix.data());
    if (gone == 0) return VQHIP_OK;
    const uint64_t na = n - gone;
    for (uint64_t w = 0; w < words; ++w) allowed[w] = ~remove[w];  // (the view reads the bits of rows below n only)
    VQ_TRY(require_gfx950());
    VQ_TRY(ix->on_device());
    hipStream_t s;
    VQ_TRY(in.stream(&s));  // behind whatever the handle still has queued on another stream
    DevBuf payload, ids, off, norms;  // the survivors' state; the old buffers leave with them (freed here where the call fails)
    DevBuf *norm = ix->norm_buf();
    auto enqueue = [&]() -> int {
        VQ_TRY(ix->rm_prefix.ensure(words * 4));
        IvfView v;
        VQ_TRY(ix->filtered(allowed.data(), true, s, &v));
        VQ_HIP(hipMemcpyAsync(ix->rm_prefix.p, prefix.data(), words * 4, hipMemcpyHostToDevice, s));
        VQ_TRY(payload.alloc((size_t)na * ix->row_b));
        VQ_TRY(ids.alloc((size_t)na * 4));
        VQ_TRY(off.alloc(((size_t)ix->nlist + 1) * 4));
        if (norm) VQ_TRY(norms.alloc((size_t)na * 4));
        VQ_TRY(launch_ivf_take(v.pick, na, ix->d_payload.p, payload.p, ix->row_b, s));
        if (norm) VQ_TRY(launch_ivf_take(v.pick, na, norm->p, norms.p, 4, s));
        VQ_TRY(launch_ivf_renumber(v.aids, na, ix->mask_ws.template as<uint32_t>(), ix->rm_prefix.template as<uint32_t>(),
                                   ids.template as<uint32_t>(), s));
        VQ_HIP(hipMemcpyAsync(off.p, v.aoff, ((size_t)ix->nlist + 1) * 4, hipMemcpyDeviceToDevice, s));  // (v_aoff is a per-call workspace)
        return VQHIP_OK;
    };
    const int rc = enqueue();
    const hipError_t e = hipStreamSynchronize(s);  // before either side is freed; the host arrays were the copies' sources
    in.synced();
    VQ_TRY(rc);
    VQ_HIP(e);
    swap_buf(ix->d_payload, payload);
    swap_buf(ix->d_ids, ids);
    swap_buf(ix->d_off, off);
    if (norm) swap_buf(*norm, norms);
    ivf_remove_host(ix, remove, na);
    ivf_bounds(ix);
    *removed = gone;
    return VQHIP_OK;
}

static int ivf_uploads(const IvfLists *ix, uint64_t *uploads) {
    if (!ix || !uploads) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<IvfLists *>(ix)->sync.mu);
    *uploads = ix->uploads;
    return VQHIP_OK;
}

// The front of every probe and search (T: an index with ready(s)): the checks in their order, the index's device, the
// calling thread's stream, the device state -- then body(in, s).  topk NULL: a probe.
template <class T, class F>
static int ivf_enter(T *ix, bool args, uint32_t nq, uint32_t nprobe, const uint32_t *topk, F &&body) {
    if (!ix || !args) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);  // (n changes under add: read under the lock)
    VQ_TRY(ivf_check_probe(ix, nprobe));
    if (topk) VQ_TRY(check_topk(ix->n, *topk));
    if (nq == 0) return VQHIP_OK;
    VQ_TRY(require_gfx950());
    VQ_TRY(ix->on_device());
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_TRY(ix->ready(s));
    return body(in, s);
}

// the three entry points of every index, over its ready(s) and search_enqueue(...)
template <class T>
static int ivf_probe(T *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    return ivf_enter(ix, queries && lists_out, nq, nprobe, nullptr, [&](Entry &in, hipStream_t s) {
        return host_search(in, s, ix->q, ix->idx, nullptr, queries, nq, ix->dim, nprobe, lists_out, nullptr, [&] {
            return ivf_probe_enqueue(ix, ix->q.template as<float>(), nq, nprobe, ix->idx.template as<uint32_t>(), s);
        });
    });
}
template <class T>
static int ivf_search(T *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    return ivf_enter(ix, queries && idx_out && dist_out, nq, nprobe, &topk, [&](Entry &in, hipStream_t s) {
        return host_search(in, s, ix->q, ix->idx, &ix->out, queries, nq, ix->dim, topk, idx_out, dist_out, [&] {
            return ix->search_enqueue(ix->q.template as<float>(), nq, nprobe, topk, ix->idx.template as<uint32_t>(),
                                      ix->out.template as<float>(), s);
        });
    });
}
template <class T>
static int ivf_search_device(T *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk, void *dev_idx, void *dev_dist) {
    return ivf_enter(ix, dev_queries && dev_idx && dev_dist, nq, nprobe, &topk, [&](Entry &, hipStream_t s) {
        return ix->search_enqueue(reinterpret_cast<const float *>(dev_queries), nq, nprobe, topk, reinterpret_cast<uint32_t *>(dev_idx),
                                  reinterpret_cast<float *>(dev_dist), s);
    });
}

// The filtered forms of the two (vqhip_ivfpq, vqhip_ivfflat, vqhip_ivfsq and vqhip_ivfbin, IvfFiltered above): the row mask `allowed` (host: ceil(n /
// 32) words, staged on the handle; device: a 4-byte aligned pointer) becomes the call's view once, after ready(s) and
// under the handle's lock (ix->filtered), and the search runs over it.  A NULL mask is reported before a device is touched.
template <class T>
static int ivf_search_masked(T *ix, const void *queries, bool host, uint32_t nq, uint32_t nprobe, uint32_t topk, const uint32_t *allowed,
                             void *idx_out, void *dist_out) {
    if (!queries || !idx_out || !dist_out || !allowed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (!host) VQ_TRY(check_mask_aligned(allowed));  // (like the pointers, before the handle is looked at)
    return ivf_enter(ix, true, nq, nprobe, &topk, [&](Entry &in, hipStream_t s) -> int {
        IvfView view;
        VQ_TRY(ix->filtered(allowed, host, s, &view));
        if (!host)
            return ix->search_enqueue(reinterpret_cast<const float *>(queries), nq, nprobe, topk, reinterpret_cast<uint32_t *>(idx_out),
                                      reinterpret_cast<float *>(dist_out), s, &view);
        return host_search(in, s, ix->q, ix->idx, &ix->out, reinterpret_cast<const float *>(queries), nq, ix->dim, topk,
                           reinterpret_cast<uint32_t *>(idx_out), reinterpret_cast<float *>(dist_out), [&] {
            return ix->search_enqueue(ix->q.template as<float>(), nq, nprobe, topk, ix->idx.template as<uint32_t>(),
                                      ix->out.template as<float>(), s, &view);
        });
    });
}

// ------------------------------------------------------------------ inverted-file PQ (k_ivf.hip) ----
// IvfLists whose payload is PQ codes (m codes of code_bytes(k) each), and the codebooks.  A residual index
// (VQHIP_IVF_RESIDUAL) also keeps the coarse centroids on the device for its tables.
struct vqhip_ivfpq : IvfFiltered {
    uint32_t m = 0, k = 0, sd = 0;
    uint32_t flags = 0;     // VQHIP_IVF_RESIDUAL: codes of x - C[list]
    std::vector<float> cb;  // [m][k][sd]
    DevBuf d_cb, d_coarse;
    DevBuf lut, bounds, rtab, rmm;  // per-call workspaces

    int ready(hipStream_t s) {
        return ivf_ready(this, s, [&] {
            VQ_TRY(d_cb.alloc(cb.size() * 4));
            VQ_HIP(hipMemcpyAsync(d_cb.p, cb.data(), cb.size() * 4, hipMemcpyHostToDevice, s));
            if (flags & VQHIP_IVF_RESIDUAL) {
                VQ_TRY(d_coarse.alloc(coarse.size() * 4));
                VQ_HIP(hipMemcpyAsync(d_coarse.p, coarse.data(), coarse.size() * 4, hipMemcpyHostToDevice, s));
            }
            return VQHIP_OK;
        }, ivf_no_hook);
    }

    // queries_dev [nq][dim] f32 -> [nq][topk] results on the device, enqueued on s, in ivf_batch's batches: a query's
    // tables are one ADC table, nprobe of them in a residual index.  view: a filtered call's (NULL: every row) -- the batches
    // then run over its lists, ids and positions, wstride and the chunk keeping their unfiltered bounds
    int search_enqueue(const float *queries_dev, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                       hipStream_t s, const IvfView *view = nullptr) {
        const bool residual = (flags & VQHIP_IVF_RESIDUAL) != 0;
        const bool fv = view && view->pick;
        const uint32_t *ids = fv ? view->aids : d_ids.as<uint32_t>(), *off = fv ? view->aoff : d_off.as<uint32_t>();
        const uint32_t *pick = fv ? view->pick : nullptr;
        const uint64_t tab_b = (uint64_t)m * k * 4 * (residual ? nprobe : 1);
        IvfBatch b;
        VQ_TRY(ivf_batch(this, nq, nprobe, tab_b, &b));
        if (residual) {
            VQ_TRY(rtab.ensure(ivf_rtab_bytes(b.nb_max, nprobe, m, k)));
            VQ_TRY(rmm.ensure(ivf_rmm_bytes(b.nb_max, nprobe)));
        } else {
            VQ_TRY(lut.ensure((size_t)b.nb_max * tab_b));
        }
        VQ_TRY(bounds.ensure((size_t)b.nb_max * 2 * 4));
        VQ_TRY(state.ensure(topk_state_bytes(b.nb_max)));
        for (uint32_t q0 = 0; q0 < nq; q0 += b.nb_max) {
            const uint32_t nb = std::min(b.nb_max, nq - q0);
            const float *Q = queries_dev + (size_t)q0 * dim;
            VQ_TRY(ivf_probe_enqueue(this, Q, nb, nprobe, probe.as<uint32_t>(), s));
            if (residual) {
                VQ_TRY(launch_ivf_rsearch(d_payload.as<uint8_t>(), ids, off, d_coarse.as<float>(), nlist,
                                          d_cb.as<float>(), m, k, sd, metric, Q, probe.as<uint32_t>(), nb, nprobe, topk,
                                          ivf_rchunk((uint64_t)nb * b.per_q, k), b.wstride, rtab.as<float>(), rmm.as<float>(), W.as<float>(),
                                          pref.as<uint32_t>(), seg.as<uint32_t>(), bounds.as<float>(), state.p,
                                          cand.as<unsigned long long>(), idx_dev + (size_t)q0 * topk, dist_dev + (size_t)q0 * topk, s, pick));
                continue;
            }
            VQ_TRY(launch_adc_lut(Q, nb, m, k, sd, d_cb.as<float>(), metric, lut.as<float>(), bounds.as<float>(), s));
            VQ_TRY(launch_ivf_search(d_payload.as<uint8_t>(), ids, off, nlist, m, k, metric, lut.as<float>(),
                                     probe.as<uint32_t>(), nb, nprobe, topk, ivf_chunk((uint64_t)nb * b.per_q), b.wstride, W.as<float>(),
                                     pref.as<uint32_t>(), seg.as<uint32_t>(), bounds.as<float>(), state.p, cand.as<unsigned long long>(),
                                     idx_dev + (size_t)q0 * topk, dist_dev + (size_t)q0 * topk, s, pick));
        }
        return VQHIP_OK;
    }
};

extern "C" {

int vqhip_ivfpq_create(const float *coarse, uint32_t nlist, const float *codebooks, uint32_t m, uint32_t k, uint32_t sub_dim,
                       int metric, vqhip_ivfpq **out) {
    return vqhip_ivfpq_create_ex(coarse, nlist, codebooks, m, k, sub_dim, metric, 0u, out);
}

int vqhip_ivfpq_create_ex(const float *coarse, uint32_t nlist, const float *codebooks, uint32_t m, uint32_t k, uint32_t sub_dim,
                          int metric, uint32_t flags, vqhip_ivfpq **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (flags & ~(uint32_t)VQHIP_IVF_RESIDUAL) return fail(VQHIP_ERR_INVALID_INPUT, "unknown flag bits 0x%x", flags & ~(uint32_t)VQHIP_IVF_RESIDUAL);
    VQ_TRY(ivf_check_lists(codebooks ? coarse : nullptr, nlist));
    if (m == 0 || k == 0 || sub_dim == 0) return fail(VQHIP_ERR_INVALID_INPUT, "m, k and sub_dim must be positive");
    if (k > kMaxCentroids) return fail(VQHIP_ERR_UNSUPPORTED, "k=%u > 65536: codes are at most two bytes per subspace", k);
    if ((uint64_t)m * sub_dim >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "dim = m * sub_dim must be below 2^32");
    VQ_TRY(check_metric(metric));
    if (vq_is_cos(metric)) return fail(VQHIP_ERR_UNSUPPORTED, "cosine distance is not a sum over subspaces: no ADC form");
    if (!adc_table_fits(m, k)) return fail_adc_table(m, k);
    std::unique_ptr<vqhip_ivfpq> ix(new vqhip_ivfpq());
    ivf_init(ix.get(), coarse, nlist, m * sub_dim, metric, (size_t)m * code_bytes(k));
    ix->m = m;
    ix->k = k;
    ix->sd = sub_dim;
    ix->flags = flags;
    ix->cb.assign(codebooks, codebooks + (size_t)m * k * sub_dim);
    *out = ix.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfpq_destroy(vqhip_ivfpq *ix) {
    delete ix;
    return VQHIP_OK;
}

int vqhip_ivfpq_add(vqhip_ivfpq *ix, const uint32_t *list_ids, const void *codes, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, codes, n, [&] {
        VQ_TRY(check_codes(reinterpret_cast<const uint8_t *>(codes), n * ix->m, ix->k));
        return ivf_append(ix, codes, n);
    });
    VQ_API_END
}

int vqhip_ivfpq_info(const vqhip_ivfpq *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, uint32_t *m, uint32_t *k, int *metric) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<vqhip_ivfpq *>(ix)->sync.mu);  // (n changes under add)
    if (n) *n = ix->n;
    if (nlist) *nlist = ix->nlist;
    if (dim) *dim = ix->dim;
    if (m) *m = ix->m;
    if (k) *k = ix->k;
    if (metric) *metric = ix->metric;
    return VQHIP_OK;
}

int vqhip_ivfpq_flags(const vqhip_ivfpq *ix, uint32_t *flags) {
    if (!ix || !flags) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *flags = ix->flags;  // (fixed at create)
    return VQHIP_OK;
}

int vqhip_ivfpq_list_sizes(vqhip_ivfpq *ix, uint64_t *sizes) {
    VQ_API_BEGIN
    return ivf_list_sizes(ix, sizes);
    VQ_API_END
}

int vqhip_ivfpq_remove(vqhip_ivfpq *ix, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return ivf_remove(ix, remove_words, removed);
    VQ_API_END
}

int vqhip_ivfpq_uploads(const vqhip_ivfpq *ix, uint64_t *uploads) {
    return ivf_uploads(ix, uploads);
}

int vqhip_ivfpq_probe(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    VQ_API_BEGIN
    return ivf_probe(ix, queries, nq, nprobe, lists_out);
    VQ_API_END
}

int vqhip_ivfpq_search(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out,
                       float *dist_out) {
    VQ_API_BEGIN
    return ivf_search(ix, queries, nq, nprobe, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfpq_search_device(vqhip_ivfpq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk, void *dev_idx,
                              void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_device(ix, dev_queries, nq, nprobe, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfpq_search_masked(vqhip_ivfpq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, const uint32_t *allowed,
                              uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, queries, true, nq, nprobe, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfpq_search_masked_device(vqhip_ivfpq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                     const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, dev_queries, false, nq, nprobe, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

}  // extern "C"

// ------------------------------------------------------------------ inverted files over W (k_ivfflat.hip, k_ivfsq.hip, k_ivfbin.hip) ----
// What vqhip_ivfflat, vqhip_ivfsq and vqhip_ivfbin share behind IvfLists: a batch's distance passes leave every D(q, i)
// of the probed lists in W, and the selection stage or the range stage runs behind them (IvfBatchView, kernels.hpp).
// T supplies only what is its own:
//   prepare(queries_dev, nq, nb_max, s)   once per call: the query norms under the cosines, or room for the packed queries
//   distances(p, v, Q, q0, s)             one batch's distance passes behind its plan p (Q: the batch's queries, f32)
//   radii_up(radii, nq, s)                the radii of a range call into this->radii as f32 distances
// A filtered call's view of the allowed rows (IvfFiltered::filtered(); DESIGN.md sections 23 and 24) is built once per call.
template <class T>
struct IvfOverW : IvfFiltered {
    DevBuf inv, lists;              // per-call workspaces: the inverted probe table, the lists' state
    DevBuf radii, range_ws, stage;  // range search: the radii, the stage's counts and offsets, its staging areas

    // The batch loop: queries_dev [nq][dim] f32 in ivf_batch's batches -- the probe, the plan, the index's distances, then
    // stage(p, v, q0) behind them.  topk: the selection's; 0: the range stage follows (its workspace is sized here for
    // the largest batch, and the plan's check is given 1).  Enqueued on s.  view: a filtered call's (NULL: every row); the
    // batches then run over its lists and ids, wstride and max_list keeping their unfiltered bounds.
    template <class Stage>
    int batches(const float *queries_dev, uint32_t nq, uint32_t nprobe, uint32_t topk, const IvfView *view, hipStream_t s,
                Stage &&stage_fn) {
        T *ix = static_cast<T *>(this);
        IvfBatch b;
        VQ_TRY(ivf_batch(this, nq, nprobe, 0, &b));
        VQ_TRY(inv.ensure((size_t)b.nb_max * nprobe * 4));
        VQ_TRY(lists.ensure(ivfflat_lists_bytes(nlist)));
        VQ_TRY(state.ensure(knn_state_bytes(b.nb_max)));
        if (topk == 0) VQ_TRY(range_ws.ensure(ivff_range_ws_bytes(b.wstride, b.nb_max)));
        VQ_TRY(ix->prepare(queries_dev, nq, b.nb_max, s));
        const bool fv = view && view->pick;
        for (uint32_t q0 = 0; q0 < nq; q0 += b.nb_max) {
            const uint32_t nb = std::min(b.nb_max, nq - q0);
            const float *Q = queries_dev + (size_t)q0 * dim;
            VQ_TRY(ivf_probe_enqueue(this, Q, nb, nprobe, probe.as<uint32_t>(), s));  // (the f32 queries, whatever the rows are)
            const IvfBatchView v{fv ? view->aids : d_ids.as<uint32_t>(), n, fv ? view->aoff : d_off.as<uint32_t>(), nlist, max_list,
                                 probe.as<uint32_t>(), nb, nprobe, ivf_chunk((uint64_t)nb * b.per_q), b.wstride,
                                 W.as<float>(), pref.as<uint32_t>(), seg.as<uint32_t>(), inv.as<uint32_t>(), lists.as<uint32_t>(), state.p,
                                 fv ? view->pick : nullptr};
            IvffPlan p;
            VQ_TRY(launch_ivff_plan(v, topk ? topk : 1, &p, s));
            VQ_TRY(ix->distances(p, v, Q, q0, s));
            VQ_TRY(stage_fn(p, v, q0));
        }
        return VQHIP_OK;
    }

    // queries_dev [nq][dim] f32 -> [nq][topk] results on the device, enqueued on s
    int search_enqueue(const float *queries_dev, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_dev, float *dist_dev,
                       hipStream_t s, const IvfView *view = nullptr) {
        return batches(queries_dev, nq, nprobe, topk, view, s, [&](const IvffPlan &p, const IvfBatchView &v, uint32_t q0) {
            return launch_ivff_select(p, v, topk, cand.as<unsigned long long>(), idx_dev + (size_t)q0 * topk, dist_dev + (size_t)q0 * topk, s);
        });
    }

    // queries_dev [nq][dim] f32 and the radii (this->radii, [nq]) -> *out, complete on return
    int range_enqueue(const float *queries_dev, uint32_t nq, uint32_t nprobe, uint64_t max_results, RangeOut *out, hipStream_t s,
                      const IvfView *view = nullptr) {
        VQ_TRY(launch_range_begin(out, nq, max_results, s));
        if (n == 0) {  // no rows: every query's range is empty
            VQ_HIP(hipMemsetAsync(out->lims.p, 0, ((size_t)nq + 1) * 8, s));
            VQ_HIP(hipStreamSynchronize(s));
            return VQHIP_OK;
        }
        VQ_TRY(batches(queries_dev, nq, nprobe, 0, view, s, [&](const IvffPlan &, const IvfBatchView &v, uint32_t q0) {
            return launch_ivff_range(v, q0, radii.as<float>() + q0, range_ws.p, &stage, max_results, out, s);
        }));
        VQ_HIP(hipStreamSynchronize(s));
        return VQHIP_OK;
    }
};

// ------------------------------------------------------------------ inverted-file flat and scalar (k_ivfflat.hip, k_ivfsq.hip, k_ivfsq4.hip) ----
// The three indexes of exact distances: the payload is the rows themselves (f32 or f16 elements), their SQ codes (dim
// bytes) or their 4-bit SQ codes (ceil(dim / 8) words), with the rows' norms under the cosines.  They differ in the norms
// kernel and the distance launcher.
template <class T>
struct IvfExact : IvfOverW<T> {
    DevBuf d_rnorm;
    DevBuf qnorm;  // per-call workspace

    DevBuf *norm_buf() { return vq_is_cos(this->metric) ? &d_rnorm : nullptr; }  // (a removal moves the norms with the rows)
    int radii_up(const float *r, uint32_t nq, hipStream_t s) {
        VQ_TRY(this->radii.ensure((size_t)nq * 4));
        VQ_HIP(hipMemcpyAsync(this->radii.p, r, (size_t)nq * 4, hipMemcpyHostToDevice, s));
        return VQHIP_OK;
    }
    int prepare(const float *queries_dev, uint32_t nq, uint32_t, hipStream_t s) {
        if (!vq_is_cos(this->metric)) return VQHIP_OK;
        VQ_TRY(qnorm.ensure((size_t)nq * 4));
        return launch_knn_norms(queries_dev, 0, nq, this->dim, qnorm.as<float>(), s);
    }
    // the norms of the batch at query q0 (NULL off the cosines)
    const float *qnorms(uint32_t q0) const { return vq_is_cos(this->metric) ? qnorm.as<float>() + q0 : nullptr; }
};

struct vqhip_ivfflat : IvfExact<vqhip_ivfflat> {
    int dtype = 0;

    int ready(hipStream_t s) {
        return ivf_ready(this, s, ivf_no_hook, [&] {
            if (!vq_is_cos(metric)) return VQHIP_OK;
            VQ_TRY(d_rnorm.alloc((size_t)n * 4));
            return launch_knn_norms(d_payload.p, dtype, n, dim, d_rnorm.as<float>(), s);
        });
    }
    int distances(const IvffPlan &p, const IvfBatchView &v, const float *Q, uint32_t q0, hipStream_t s) {
        return launch_ivfflat_distances(p, v, metric, d_payload.p, dtype, dim, d_rnorm.as<float>(), Q, qnorms(q0), s);
    }
};

struct vqhip_ivfsq : IvfExact<vqhip_ivfsq> {
    uint32_t levels = 0;
    float mn = 0, mx = 0, step = 0;
    SqbqEncodeOp op;  // add_rows: the encode of this quantizer

    int ready(hipStream_t s) {
        return ivf_ready(this, s, ivf_no_hook, [&] {
            if (!vq_is_cos(metric)) return VQHIP_OK;
            VQ_TRY(d_rnorm.alloc((size_t)n * 4));
            return launch_sq_norms(d_payload.as<uint8_t>(), n, dim, mn, step, d_rnorm.as<float>(), s);
        });
    }
    int distances(const IvffPlan &p, const IvfBatchView &v, const float *Q, uint32_t q0, hipStream_t s) {
        return launch_ivfsq_distances(p, v, metric, d_payload.as<uint8_t>(), dim, mn, step, d_rnorm.as<float>(), Q, qnorms(q0), s);
    }
};

// The scalar index at four bits a dimension (k_ivfsq4.hip): the payload is the packed words of
// vqhip_sq4index's layout, W = sq4_words(dim) a row, pad nibbles zero, in add order on the host.
struct vqhip_ivfsq4 : IvfExact<vqhip_ivfsq4> {
    uint32_t W = 0, levels = 0;
    float mn = 0, mx = 0, step = 0;
    SqbqEncodeOp op;  // add_rows: the encode of this quantizer

    int ready(hipStream_t s) {
        return ivf_ready(this, s, ivf_no_hook, [&] {
            if (!vq_is_cos(metric)) return VQHIP_OK;
            VQ_TRY(d_rnorm.alloc((size_t)n * 4));
            return launch_sq4_norms(d_payload.as<uint32_t>(), n, dim, mn, step, d_rnorm.as<float>(), s);
        });
    }
    int distances(const IvffPlan &p, const IvfBatchView &v, const float *Q, uint32_t q0, hipStream_t s) {
        return launch_ivfsq4_distances(p, v, metric, d_payload.as<uint32_t>(), dim, mn, step, d_rnorm.as<float>(), Q, qnorms(q0), s);
    }
};

// ------------------------------------------------------------------ inverted-file binary (k_ivfbin.hip) ----
// The payload is packed BQ words (bin_words(dim) words a row, pad bits zero).  Two metrics: `metric` of the reported
// distance (the table S), `probe_metric` of the flat index over the centroids.
struct vqhip_ivfbin : IvfOverW<vqhip_ivfbin> {
    uint32_t nw = 0, low = 0, high = 1;  // nw: words a row
    float thr = 0;
    DevBuf table;                 // S [dim + 1]
    DevBuf qw;                    // per-call workspace: the batch's packed queries
    std::vector<float> h_radii;   // the host side of radii (the source of an asynchronous copy)

    // The Hamming radii of a range call as the f32 radii of the range stage: r_q = the distance the index reports for
    // H = min(h_q, dim).  The reported table is strictly increasing, so D <= r_q iff H <= h_q.
    int radii_up(const uint32_t *h, uint32_t nq, hipStream_t s) {
        std::vector<float> S(dim + 1);
        binary_table(dim, low, high, metric, S.data());
        h_radii.resize(nq);
        for (uint32_t q = 0; q < nq; ++q) {
            const float v = S[std::min(h[q], dim)];
            h_radii[q] = metric == VQHIP_EUCLIDEAN ? sqrtf(v) : v;
        }
        VQ_TRY(radii.ensure((size_t)nq * 4));
        VQ_HIP(hipMemcpyAsync(radii.p, h_radii.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
        return VQHIP_OK;
    }

    int ready(hipStream_t s) {
        return ivf_ready(this, s, [&] {
            std::vector<float> S(dim + 1);
            binary_table(dim, low, high, metric, S.data());
            VQ_TRY(table.alloc(S.size() * 4));
            VQ_HIP(hipMemcpyAsync(table.p, S.data(), S.size() * 4, hipMemcpyHostToDevice, s));
            VQ_HIP(hipStreamSynchronize(s));  // (S is this call's)
            return VQHIP_OK;
        }, ivf_no_hook);
    }
    int prepare(const float *, uint32_t, uint32_t nb_max, hipStream_t) { return qw.ensure((size_t)nb_max * nw * 4); }
    int distances(const IvffPlan &p, const IvfBatchView &v, const float *Q, uint32_t, hipStream_t s) {
        VQ_TRY(launch_bq_pack(Q, VQHIP_BINARY_F32, v.nb, dim, thr, high, qw.as<uint32_t>(), s));
        return launch_ivfbin_distances(p, v, metric, d_payload.as<uint32_t>(), dim, table.as<float>(), qw.as<uint32_t>(), s);
    }
};

// One range call on an inverted-file flat, scalar or binary index: nprobe as search checks it, then the device state as
// search builds it; the radii (radii_up: f32 distances, or the binary index's u32 Hamming radii as the distances its table
// reports for them) go up and range_enqueue leaves the result complete.
template <class T, class R>
static int ivf_range(T *ix, const void *queries, bool host, uint32_t nq, uint32_t nprobe, const R *radii, uint64_t max_results,
                     vqhip_range **out) {
    return range_enter(ix, queries, host, nq, radii, max_results, out, [&] { return ivf_check_probe(ix, nprobe); },
                       [&](const float *qdev, RangeOut *r, hipStream_t s) -> int {
        VQ_TRY(ix->ready(s));
        VQ_TRY(ix->radii_up(radii, nq, s));
        return ix->range_enqueue(qdev, nq, nprobe, max_results, r, s);
    });
}
// ivf_range under the row mask `allowed` of a filtered call (R: f32 radii, or the binary index's u32 Hamming radii): the
// mask's pointer is checked behind range_args and, like them, before the handle; the view is built behind ready(s)
// (ix->filtered).
template <class T, class R>
static int ivf_range_masked(T *ix, const void *queries, bool host, uint32_t nq, uint32_t nprobe, const R *radii,
                            uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_TRY(range_args(queries, radii, nq, max_results, out));
    if (!allowed) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (!host) VQ_TRY(check_mask_aligned(allowed));
    return range_enter(ix, queries, host, nq, radii, max_results, out, [&] { return ivf_check_probe(ix, nprobe); },
                       [&](const float *qdev, RangeOut *r, hipStream_t s) -> int {
        VQ_TRY(ix->ready(s));
        IvfView view;
        if (ix->n) VQ_TRY(ix->filtered(allowed, host, s, &view));  // (no rows: range_enqueue's empty result)
        VQ_TRY(ix->radii_up(radii, nq, s));
        return ix->range_enqueue(qdev, nq, nprobe, max_results, r, s, &view);
    });
}

extern "C" {

int vqhip_ivfflat_create(const float *coarse, uint32_t nlist, uint32_t dim, int dtype, int metric, vqhip_ivfflat **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    VQ_TRY(ivf_check_lists(coarse, nlist));
    if (dim == 0) return fail(VQHIP_ERR_INVALID_INPUT, "dim must be at least 1");
    if (dtype != 0 && dtype != 1) return fail(VQHIP_ERR_INVALID_INPUT, "dtype must be 0 (f32) or 1 (f16), not %d", dtype);
    VQ_TRY(check_metric(metric));
    std::unique_ptr<vqhip_ivfflat> ix(new vqhip_ivfflat());
    ivf_init(ix.get(), coarse, nlist, dim, metric, (size_t)dim * (dtype == 1 ? 2 : 4));
    ix->dtype = dtype;
    *out = ix.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfflat_destroy(vqhip_ivfflat *ix) {
    delete ix;
    return VQHIP_OK;
}

int vqhip_ivfflat_add(vqhip_ivfflat *ix, const uint32_t *list_ids, const void *rows, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, rows, n, [&] { return ivf_append(ix, rows, n); });
    VQ_API_END
}

int vqhip_ivfflat_info(const vqhip_ivfflat *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *dtype, int *metric) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<vqhip_ivfflat *>(ix)->sync.mu);  // (n changes under add)
    if (n) *n = ix->n;
    if (nlist) *nlist = ix->nlist;
    if (dim) *dim = ix->dim;
    if (dtype) *dtype = ix->dtype;
    if (metric) *metric = ix->metric;
    return VQHIP_OK;
}

int vqhip_ivfflat_list_sizes(vqhip_ivfflat *ix, uint64_t *sizes) {
    VQ_API_BEGIN
    return ivf_list_sizes(ix, sizes);
    VQ_API_END
}

int vqhip_ivfflat_remove(vqhip_ivfflat *ix, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return ivf_remove(ix, remove_words, removed);
    VQ_API_END
}

int vqhip_ivfflat_uploads(const vqhip_ivfflat *ix, uint64_t *uploads) {
    return ivf_uploads(ix, uploads);
}

int vqhip_ivfflat_probe(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    VQ_API_BEGIN
    return ivf_probe(ix, queries, nq, nprobe, lists_out);
    VQ_API_END
}

int vqhip_ivfflat_search(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out,
                         float *dist_out) {
    VQ_API_BEGIN
    return ivf_search(ix, queries, nq, nprobe, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfflat_search_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_device(ix, dev_queries, nq, nprobe, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfflat_range_search(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                               uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, queries, true, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfflat_range_search_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                      uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, dev_queries, false, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfflat_search_masked(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, queries, true, nq, nprobe, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfflat_search_masked_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                       const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, dev_queries, false, nq, nprobe, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfflat_range_search_masked(vqhip_ivfflat *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                      uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, queries, true, nq, nprobe, radii, max_results, allowed, out);
    VQ_API_END
}

int vqhip_ivfflat_range_search_masked_device(vqhip_ivfflat *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                             const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                             vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, dev_queries, false, nq, nprobe, radii, max_results, dev_allowed, out);
    VQ_API_END
}

int vqhip_ivfsq_create(float min, float max, uint32_t levels, const float *coarse, uint32_t nlist, uint32_t dim, int metric,
                       vqhip_ivfsq **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    float step = 0;
    VQ_TRY(sq_check(min, max, levels, &step));
    VQ_TRY(ivf_check_lists(coarse, nlist));
    if (dim == 0) return fail(VQHIP_ERR_INVALID_INPUT, "dim must be at least 1");
    VQ_TRY(check_metric(metric));
    std::unique_ptr<vqhip_ivfsq> ix(new vqhip_ivfsq());
    VQ_TRY(sq_encode_op(min, max, levels, &ix->op));
    ivf_init(ix.get(), coarse, nlist, dim, metric, dim);
    ix->levels = levels;
    ix->mn = min, ix->mx = max, ix->step = step;
    *out = ix.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfsq_destroy(vqhip_ivfsq *ix) {
    delete ix;
    return VQHIP_OK;
}

int vqhip_ivfsq_add_codes(vqhip_ivfsq *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, codes, n, [&] { return ivf_append(ix, codes, n); });
    VQ_API_END
}

int vqhip_ivfsq_add_rows(vqhip_ivfsq *ix, const uint32_t *list_ids, const float *rows, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, rows, n, [&] {
        VQ_TRY(require_gfx950());
        VQ_TRY(ix->on_device());
        const size_t have = ix->payload.size();
        ix->payload.resize(have + (size_t)n * ix->dim);
        const int rc = sqbq_encode_host(ix->op, rows, n * ix->dim, ix->payload.data() + have);  // vqhip_sq_encode's path
        if (rc != VQHIP_OK) ix->payload.resize(have);  // (nothing is stored)
        return rc;
    });
    VQ_API_END
}

int vqhip_ivfsq_info(const vqhip_ivfsq *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, float *min, float *max,
                     uint32_t *levels) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<vqhip_ivfsq *>(ix)->sync.mu);  // (n changes under add)
    if (n) *n = ix->n;
    if (nlist) *nlist = ix->nlist;
    if (dim) *dim = ix->dim;
    if (metric) *metric = ix->metric;
    if (min) *min = ix->mn;
    if (max) *max = ix->mx;
    if (levels) *levels = ix->levels;
    return VQHIP_OK;
}

int vqhip_ivfsq_list_sizes(vqhip_ivfsq *ix, uint64_t *sizes) {
    VQ_API_BEGIN
    return ivf_list_sizes(ix, sizes);
    VQ_API_END
}

int vqhip_ivfsq_codes(vqhip_ivfsq *ix, uint8_t *codes_out) {
    VQ_API_BEGIN
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    if (ix->n == 0) return VQHIP_OK;
    if (!codes_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    memcpy(codes_out, ix->payload.data(), ix->payload.size());
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfsq_remove(vqhip_ivfsq *ix, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return ivf_remove(ix, remove_words, removed);
    VQ_API_END
}

int vqhip_ivfsq_uploads(const vqhip_ivfsq *ix, uint64_t *uploads) {
    return ivf_uploads(ix, uploads);
}

int vqhip_ivfsq_probe(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    VQ_API_BEGIN
    return ivf_probe(ix, queries, nq, nprobe, lists_out);
    VQ_API_END
}

int vqhip_ivfsq_search(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out,
                       float *dist_out) {
    VQ_API_BEGIN
    return ivf_search(ix, queries, nq, nprobe, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfsq_search_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk, void *dev_idx,
                              void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_device(ix, dev_queries, nq, nprobe, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfsq_range_search(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                             uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, queries, true, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfsq_range_search_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                    uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, dev_queries, false, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfsq_search_masked(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                              const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, queries, true, nq, nprobe, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfsq_search_masked_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                     const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, dev_queries, false, nq, nprobe, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfsq_range_search_masked(vqhip_ivfsq *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                    uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, queries, true, nq, nprobe, radii, max_results, allowed, out);
    VQ_API_END
}

int vqhip_ivfsq_range_search_masked_device(vqhip_ivfsq *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                           const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                           vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, dev_queries, false, nq, nprobe, radii, max_results, dev_allowed, out);
    VQ_API_END
}

int vqhip_ivfsq4_create(float min, float max, uint32_t levels, const float *coarse, uint32_t nlist, uint32_t dim, int metric,
                        vqhip_ivfsq4 **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    float step = 0;
    VQ_TRY(sq_check(min, max, levels, &step));
    if (levels > 16) return fail(VQHIP_ERR_INVALID_INPUT, "levels %u: a 4-bit index holds at most 16", levels);  // (vqhip_sq4index's)
    VQ_TRY(ivf_check_lists(coarse, nlist));
    if (dim == 0) return fail(VQHIP_ERR_INVALID_INPUT, "dim must be at least 1");
    VQ_TRY(check_metric(metric));
    std::unique_ptr<vqhip_ivfsq4> ix(new vqhip_ivfsq4());
    VQ_TRY(sq_encode_op(min, max, levels, &ix->op));
    ix->W = sq4_words(dim);
    ivf_init(ix.get(), coarse, nlist, dim, metric, (size_t)ix->W * 4);
    ix->levels = levels;
    ix->mn = min, ix->mx = max, ix->step = step;
    *out = ix.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfsq4_destroy(vqhip_ivfsq4 *ix) {
    delete ix;
    return VQHIP_OK;
}

int vqhip_ivfsq4_add_codes(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, codes, n, [&] {
        const uint32_t d = ix->dim, W = ix->W;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t t = 0; t < d; ++t)
                if (codes[i * d + t] > 15)
                    return fail(VQHIP_ERR_INVALID_INPUT, "added row %llu holds code %u: a 4-bit code is at most 15", (unsigned long long)i,
                                (unsigned)codes[i * d + t]);
        const size_t have = ix->payload.size();
        ix->payload.resize(have + (size_t)n * ix->row_b, 0);
        uint32_t *w = reinterpret_cast<uint32_t *>(ix->payload.data() + have);  // (row_b is a multiple of 4, the vector's base aligned)
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t t = 0; t < d; ++t) w[i * W + t / 8] |= (uint32_t)codes[i * d + t] << (4 * (t % 8));
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_ivfsq4_add_packed(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const uint32_t *words, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, words, n, [&] {
        if (ix->dim % 8) {
            const uint32_t keep = (1u << (4 * (ix->dim % 8))) - 1u;
            for (uint64_t i = 0; i < n; ++i)
                if (words[i * ix->W + ix->W - 1] & ~keep)
                    return fail(VQHIP_ERR_INVALID_INPUT, "added row %llu has a pad nibble set", (unsigned long long)i);
        }
        return ivf_append(ix, words, n);
    });
    VQ_API_END
}

int vqhip_ivfsq4_add_rows(vqhip_ivfsq4 *ix, const uint32_t *list_ids, const float *rows, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, rows, n, [&] {
        VQ_TRY(require_gfx950());
        VQ_TRY(ix->on_device());
        hipStream_t s;
        VQ_TRY(current_stream(&s));
        const uint32_t d = ix->dim;
        const size_t have = ix->payload.size(), row_b = ix->row_b;
        ix->payload.resize(have + (size_t)n * row_b);
        auto pack = [&]() -> int {  // vqhip_sq4index's path for f32 rows: encode a piece, pack it, and the words come down
            const uint64_t per = std::max<uint64_t>(1, kStageBytes / ((size_t)d * 4));  // (staged_rows' piece for rows of 4 d bytes)
            const uint64_t piece_n = std::min<uint64_t>(per, n);
            DevBuf codes, words, bad;
            VQ_TRY(codes.alloc((size_t)piece_n * d));
            VQ_TRY(words.alloc((size_t)piece_n * row_b));
            VQ_TRY(bad.alloc(4));
            VQ_HIP(hipMemsetAsync(bad.p, 0, 4, s));  // (an encoded code is below levels <= 16: never set)
            return staged_rows(rows, n, (size_t)d * 4, s, [&](const void *piece, uint64_t r0, uint64_t rn) -> int {
                VQ_TRY(launch_sqbq_encode(ix->op, static_cast<const float *>(piece), rn * d, codes.as<uint8_t>(), s));
                VQ_TRY(launch_sq4_pack(codes.as<uint8_t>(), rn, d, words.as<uint32_t>(), bad.as<uint32_t>(), s));
                VQ_HIP(hipMemcpyAsync(ix->payload.data() + have + (size_t)r0 * row_b, words.p, (size_t)rn * row_b, hipMemcpyDeviceToHost, s));
                return VQHIP_OK;  // (staged_rows waits for the piece)
            });
        };
        const int rc = pack();
        if (rc != VQHIP_OK) ix->payload.resize(have);  // (nothing is stored)
        return rc;
    });
    VQ_API_END
}

int vqhip_ivfsq4_info(const vqhip_ivfsq4 *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, float *min, float *max,
                      uint32_t *levels) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<vqhip_ivfsq4 *>(ix)->sync.mu);  // (n changes under add)
    if (n) *n = ix->n;
    if (nlist) *nlist = ix->nlist;
    if (dim) *dim = ix->dim;
    if (metric) *metric = ix->metric;
    if (min) *min = ix->mn;
    if (max) *max = ix->mx;
    if (levels) *levels = ix->levels;
    return VQHIP_OK;
}

int vqhip_ivfsq4_list_sizes(vqhip_ivfsq4 *ix, uint64_t *sizes) {
    VQ_API_BEGIN
    return ivf_list_sizes(ix, sizes);
    VQ_API_END
}

int vqhip_ivfsq4_codes(vqhip_ivfsq4 *ix, uint8_t *codes_out) {
    VQ_API_BEGIN
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    if (ix->n == 0) return VQHIP_OK;
    if (!codes_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    const uint32_t *w = reinterpret_cast<const uint32_t *>(ix->payload.data());
    for (uint64_t i = 0; i < ix->n; ++i)
        for (uint32_t t = 0; t < ix->dim; ++t) codes_out[i * ix->dim + t] = (uint8_t)((w[i * ix->W + t / 8] >> (4 * (t % 8))) & 15u);
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfsq4_packed(vqhip_ivfsq4 *ix, uint32_t *words_out) {
    VQ_API_BEGIN
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    if (ix->n == 0) return VQHIP_OK;
    if (!words_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    memcpy(words_out, ix->payload.data(), ix->payload.size());
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfsq4_remove(vqhip_ivfsq4 *ix, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return ivf_remove(ix, remove_words, removed);
    VQ_API_END
}

int vqhip_ivfsq4_uploads(const vqhip_ivfsq4 *ix, uint64_t *uploads) {
    return ivf_uploads(ix, uploads);
}

int vqhip_ivfsq4_probe(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    VQ_API_BEGIN
    return ivf_probe(ix, queries, nq, nprobe, lists_out);
    VQ_API_END
}

int vqhip_ivfsq4_search(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out,
                        float *dist_out) {
    VQ_API_BEGIN
    return ivf_search(ix, queries, nq, nprobe, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfsq4_search_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk, void *dev_idx,
                               void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_device(ix, dev_queries, nq, nprobe, topk, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfsq4_range_search(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                              uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, queries, true, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfsq4_range_search_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                     uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, dev_queries, false, nq, nprobe, radii, max_results, out);
    VQ_API_END
}

int vqhip_ivfsq4_search_masked(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, queries, true, nq, nprobe, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfsq4_search_masked_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, dev_queries, false, nq, nprobe, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfsq4_range_search_masked(vqhip_ivfsq4 *ix, const float *queries, uint32_t nq, uint32_t nprobe, const float *radii,
                                     uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, queries, true, nq, nprobe, radii, max_results, allowed, out);
    VQ_API_END
}

int vqhip_ivfsq4_range_search_masked_device(vqhip_ivfsq4 *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                            const float *radii, uint64_t max_results, const uint32_t *dev_allowed,
                                            vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, dev_queries, false, nq, nprobe, radii, max_results, dev_allowed, out);
    VQ_API_END
}

int vqhip_ivfbin_create(float threshold, uint32_t low, uint32_t high, const float *coarse, uint32_t nlist, uint32_t dim, int metric,
                        int coarse_metric, vqhip_ivfbin **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    VQ_TRY(bq_check(threshold, low, high));
    VQ_TRY(ivf_check_lists(coarse, nlist));
    if (dim == 0 || dim > VQHIP_BINARY_MAX_DIM) return fail(VQHIP_ERR_INVALID_INPUT, "d %u must be in [1, 8192]", dim);
    if (vq_is_cos(metric)) return fail(VQHIP_ERR_UNSUPPORTED, "cosine is not a function of the Hamming distance alone");
    if (metric != VQHIP_SQUARED_EUCLIDEAN && metric != VQHIP_EUCLIDEAN && metric != VQHIP_MANHATTAN)
        return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    VQ_TRY(check_metric(coarse_metric));
    std::unique_ptr<vqhip_ivfbin> ix(new vqhip_ivfbin());
    ivf_init(ix.get(), coarse, nlist, dim, metric, (size_t)bin_words(dim) * 4);
    ix->probe_metric = coarse_metric;
    ix->nw = bin_words(dim);
    ix->thr = threshold, ix->low = low, ix->high = high;
    *out = ix.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfbin_destroy(vqhip_ivfbin *ix) {
    delete ix;
    return VQHIP_OK;
}

int vqhip_ivfbin_add_packed(vqhip_ivfbin *ix, const uint32_t *list_ids, const uint32_t *words, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, words, n, [&] {
        if (ix->dim % 32) {
            const uint32_t mask = (1u << (ix->dim % 32)) - 1u;
            for (uint64_t i = 0; i < n; ++i)
                if (words[i * ix->nw + ix->nw - 1] & ~mask)
                    return fail(VQHIP_ERR_INVALID_INPUT, "row %llu has a pad bit set", (unsigned long long)i);
        }
        return ivf_append(ix, words, n);
    });
    VQ_API_END
}

int vqhip_ivfbin_add_codes(vqhip_ivfbin *ix, const uint32_t *list_ids, const uint8_t *codes, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, codes, n, [&] {
        const size_t have = ix->payload.size();
        ix->payload.resize(have + (size_t)n * ix->row_b, 0);
        uint32_t *w = reinterpret_cast<uint32_t *>(ix->payload.data() + have);  // (row_b is a multiple of 4, the vector's base aligned)
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t t = 0; t < ix->dim; ++t)
                if (codes[i * ix->dim + t] >= ix->high) w[i * ix->nw + t / 32] |= 1u << (t % 32);
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_ivfbin_add_rows(vqhip_ivfbin *ix, const uint32_t *list_ids, const float *rows, uint64_t n) {
    VQ_API_BEGIN
    return ivf_add(ix, list_ids, rows, n, [&] {
        VQ_TRY(require_gfx950());
        VQ_TRY(ix->on_device());
        hipStream_t s;
        VQ_TRY(current_stream(&s));
        const size_t have = ix->payload.size();
        ix->payload.resize(have + (size_t)n * ix->row_b);
        auto pack = [&]() -> int {  // vqhip_bq_pack's path with this quantizer's threshold
            const uint64_t per = std::max<uint64_t>(1, (256ull << 20) / ((uint64_t)ix->dim * 4));
            const uint64_t rows_b = std::min<uint64_t>(per, n);
            DevBuf dx, dw;
            VQ_TRY(dx.alloc((size_t)rows_b * ix->dim * 4));
            VQ_TRY(dw.alloc((size_t)rows_b * ix->row_b));
            for (uint64_t r0 = 0; r0 < n; r0 += per) {
                const uint64_t rn = std::min<uint64_t>(per, n - r0);
                VQ_HIP(hipMemcpyAsync(dx.p, rows + r0 * ix->dim, (size_t)rn * ix->dim * 4, hipMemcpyHostToDevice, s));
                VQ_TRY(launch_bq_pack(dx.p, VQHIP_BINARY_F32, rn, ix->dim, ix->thr, ix->high, dw.as<uint32_t>(), s));
                VQ_HIP(hipMemcpyAsync(ix->payload.data() + have + (size_t)r0 * ix->row_b, dw.p, (size_t)rn * ix->row_b,
                                      hipMemcpyDeviceToHost, s));
                VQ_HIP(hipStreamSynchronize(s));
            }
            return VQHIP_OK;
        };
        const int rc = pack();
        if (rc != VQHIP_OK) ix->payload.resize(have);  // (nothing is stored)
        return rc;
    });
    VQ_API_END
}

int vqhip_ivfbin_info(const vqhip_ivfbin *ix, uint64_t *n, uint32_t *nlist, uint32_t *dim, int *metric, int *coarse_metric,
                      float *threshold, uint32_t *low, uint32_t *high) {
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(const_cast<vqhip_ivfbin *>(ix)->sync.mu);  // (n changes under add)
    if (n) *n = ix->n;
    if (nlist) *nlist = ix->nlist;
    if (dim) *dim = ix->dim;
    if (metric) *metric = ix->metric;
    if (coarse_metric) *coarse_metric = ix->probe_metric;
    if (threshold) *threshold = ix->thr;
    if (low) *low = ix->low;
    if (high) *high = ix->high;
    return VQHIP_OK;
}

int vqhip_ivfbin_list_sizes(vqhip_ivfbin *ix, uint64_t *sizes) {
    VQ_API_BEGIN
    return ivf_list_sizes(ix, sizes);
    VQ_API_END
}

int vqhip_ivfbin_packed(vqhip_ivfbin *ix, uint32_t *words_out) {
    VQ_API_BEGIN
    if (!ix) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(ix->sync);
    if (ix->n == 0) return VQHIP_OK;
    if (!words_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    memcpy(words_out, ix->payload.data(), ix->payload.size());
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_ivfbin_remove(vqhip_ivfbin *ix, const uint32_t *remove_words, uint64_t *removed) {
    VQ_API_BEGIN
    return ivf_remove(ix, remove_words, removed);
    VQ_API_END
}

int vqhip_ivfbin_uploads(const vqhip_ivfbin *ix, uint64_t *uploads) {
    return ivf_uploads(ix, uploads);
}

int vqhip_ivfbin_probe(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t *lists_out) {
    VQ_API_BEGIN
    return ivf_probe(ix, queries, nq, nprobe, lists_out);
    VQ_API_END
}

int vqhip_ivfbin_search(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk, uint32_t *idx_out,
                        float *dist_out) {
    VQ_API_BEGIN
    return ivf_search(ix, queries, nq, nprobe, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfbin_search_masked(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                               const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, queries, true, nq, nprobe, topk, allowed, idx_out, dist_out);
    VQ_API_END
}

int vqhip_ivfbin_search_masked_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk,
                                      const uint32_t *dev_allowed, void *dev_idx, void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_masked(ix, dev_queries, false, nq, nprobe, topk, dev_allowed, dev_idx, dev_dist);
    VQ_API_END
}

int vqhip_ivfbin_range_search_masked(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, const uint32_t *hradii,
                                     uint64_t max_results, const uint32_t *allowed, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, queries, true, nq, nprobe, hradii, max_results, allowed, out);
    VQ_API_END
}

int vqhip_ivfbin_range_search_masked_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe,
                                            const uint32_t *hradii, uint64_t max_results, const uint32_t *dev_allowed,
                                            vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range_masked(ix, dev_queries, false, nq, nprobe, hradii, max_results, dev_allowed, out);
    VQ_API_END
}

int vqhip_ivfbin_range_search(vqhip_ivfbin *ix, const float *queries, uint32_t nq, uint32_t nprobe, const uint32_t *hradii,
                              uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, queries, true, nq, nprobe, hradii, max_results, out);
    VQ_API_END
}

int vqhip_ivfbin_range_search_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, const uint32_t *hradii,
                                     uint64_t max_results, vqhip_range **out) {
    VQ_API_BEGIN
    return ivf_range(ix, dev_queries, false, nq, nprobe, hradii, max_results, out);
    VQ_API_END
}

int vqhip_ivfbin_search_device(vqhip_ivfbin *ix, const void *dev_queries, uint32_t nq, uint32_t nprobe, uint32_t topk, void *dev_idx,
                               void *dev_dist) {
    VQ_API_BEGIN
    return ivf_search_device(ix, dev_queries, nq, nprobe, topk, dev_idx, dev_dist);
    VQ_API_END
}

}  // extern "C"
