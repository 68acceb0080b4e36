// api.hip -- extern "C" entry points of libvqhip (see include/vqhip.h for the contract and
// the reference file:line each entry replaces).  Host-side orchestration only; the kernels
// are in k_*.hip.  No CPU compute fallback exists anywhere in this file.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "adc_plan.hpp"
#include "compact.hpp"
#include "ivf_remove.hpp"
#include "kernels.hpp"

namespace vqhip {

// ---------------------------------------------------------------- thread-local state ----
ThreadState &tls() {
    static thread_local ThreadState st;
    return st;
}

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    tls().last_error = buf;
    return code;
}

// per-device facts, published once per device: std::call_once (threads of different handles may make their first call
// at the same time)
static int g_num_cus[64];
static int g_dev_ok[64];  // 0 unknown (probe failed), 1 gfx950, -1 other
static char g_dev_arch[64][64];
static std::once_flag g_dev_once[64];

int require_gfx950() {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(VQHIP_ERR_NO_DEVICE, "no HIP device available (%s); libvqhip has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    int dev = 0;
    VQ_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(VQHIP_ERR_NO_DEVICE, "device index %d out of range", dev);
    std::call_once(g_dev_once[dev], [dev]() {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return;  // g_dev_ok stays 0: reported below
        g_num_cus[dev] = prop.multiProcessorCount;
        strncpy(g_dev_arch[dev], prop.gcnArchName, sizeof(g_dev_arch[dev]) - 1);
        g_dev_ok[dev] = (strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? 1 : -1;
    });
    if (g_dev_ok[dev] == 0) return fail(VQHIP_ERR_NO_DEVICE, "could not read the properties of HIP device %d", dev);
    if (g_dev_ok[dev] < 0)
        return fail(VQHIP_ERR_NO_DEVICE, "current HIP device is %s, not gfx950; libvqhip targets MI355X only", g_dev_arch[dev]);
    return VQHIP_OK;
}

int num_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    return g_num_cus[dev] > 0 ? g_num_cus[dev] : 256;
}

int current_stream(hipStream_t *out) {
    ThreadState &st = tls();
    if (st.user_stream_set) {
        *out = st.user_stream;
        return VQHIP_OK;
    }
    int dev = 0;
    VQ_HIP(hipGetDevice(&dev));
    if (!st.own_stream || st.own_stream_device != dev) {
        // one lazily created non-blocking stream per thread and device
        hipStream_t s;
        VQ_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        st.own_stream = s;
        st.own_stream_device = dev;
    }
    *out = st.own_stream;
    return VQHIP_OK;
}

// ------------------------------------------------------------------ codebook state ----
struct CodebookState {
    uint32_t m = 0, k = 0, sd = 0, nt = 0, ks = 0;
    bool mfma_ok = false, bf16_ok = false;
    bool prepared = false;  // false = the centroids changed: every image is stale
    bool prepared_base = false, prepared_x32 = false;
    int metric = VQHIP_SQUARED_EUCLIDEAN;  // what the prepared images are for (cosine differs)
    DevBuf cb, prepA, prepCn, meta, cnsqrt, prepA32, prepA32_3, cbc, cen, cn32;
    bool x32_ok = false;
    uint32_t x32_groups = 0;  // > 1: centroid groups (sub_dim 32 / 48), partial verdicts merged per row

    // encode_only: the handle never trains (a PQ encoder) -- eligible shapes also carry the two-slice image of the
    // three-product screen; a k-means handle re-prepares its images every iteration and has no use for it
    int init(uint32_t m_, uint32_t k_, uint32_t sd_, bool encode_only = false) {
        m = m_;
        k = k_;
        sd = sd_;
        // the update / gather / prepare kernels index a codebook's m*k*(sub_dim+1) elements with 32 bits
        if ((uint64_t)m * k * ((uint64_t)sd + 1) >= (1ull << 32))
            return fail(VQHIP_ERR_UNSUPPORTED, "m*k*(sub_dim+1) = %llu exceeds 2^32-1 codebook elements",
                        (unsigned long long)((uint64_t)m * k * ((uint64_t)sd + 1)));
        mfma_ok = screen_supported(sd, k);
        VQ_TRY(cb.alloc((size_t)m * k * sd * 4));
        VQ_TRY(cnsqrt.alloc((size_t)m * k * 4));
        VQ_TRY(meta.alloc((size_t)m * 4 * 4));
        nt = ks = 0;
        if (mfma_ok) {
            screen_tiling(sd, k, &nt, &ks);
            VQ_TRY(prepA.alloc((size_t)m * nt * ks * 64 * 4));
            VQ_TRY(prepCn.alloc((size_t)m * nt * 16 * 4));
        }
        // bf16 engine (X32 kernels; their own tilings, e.g. sub_dim 24): only on a device whose bf16 MFMA
        // matches the accumulation model the margin is derived from (k_selftest.hip)
        x32_ok = screen_bf16_x32_supported(sd, k);
        if (x32_ok) {
            int trusted = 0;
            VQ_TRY(bf16_mfma_selftest(nullptr, nullptr, &trusted));
            if (!trusted) x32_ok = false;
        }
        bf16_ok = x32_ok;
        x32_groups = 0;
        if (x32_ok) {
            uint32_t per = 0;
            screen_bf16_x32_tiling(sd, k, &per, &x32_groups);
            const size_t tiles = (size_t)per * x32_groups;  // image padded to whole centroid groups
            VQ_TRY(prepA32.alloc((size_t)m * tiles * screen_bf16_x32_mfmas(sd) * 4 * 64 * 4));
            if (encode_only && screen_bf16_three_products_supported(sd, k)) VQ_TRY(prepA32_3.alloc((size_t)m * tiles * 3 * 4 * 64 * 4));
            const uint32_t sdp = x32_padded_sd(sd);  // >= sd: the screen kernel's sub_dim (zero padding)
            VQ_TRY(cbc.alloc((size_t)m * k * sdp * 4));
            VQ_TRY(cen.alloc((size_t)m * (sdp + 4) * 4));
            VQ_TRY(cn32.alloc((size_t)m * tiles * 32 * 4));
        }
        prepared = false;
        return VQHIP_OK;
    }
    CodebookView view() const {
        CodebookView v;
        v.m = m;
        v.k = k;
        v.sd = sd;
        v.cb = cb.as<float>();
        v.nt = nt;
        v.ks = ks;
        v.prepA = mfma_ok ? prepA.as<float>() : nullptr;
        v.prepCn = mfma_ok ? prepCn.as<float>() : nullptr;
        v.meta = meta.as<float>();
        v.cnsqrt = cnsqrt.as<float>();
        v.prepA32 = x32_ok ? prepA32.as<uint32_t>() : nullptr;
        v.prepA32_3 = (x32_ok && prepA32_3.p && metric != VQHIP_COSINE) ? prepA32_3.as<uint32_t>() : nullptr;
        v.cen = x32_ok ? cen.as<float>() : nullptr;
        v.cn32 = x32_ok ? cn32.as<float>() : nullptr;
        return v;
    }
    // need_base = false: only the X32 images (squared-L2 on the single-pass bf16 screen reads nothing else: the
    // fp32 engine's image, the centroid norms and `meta` are for the other engines, cosine and the grouped merge)
    int prepare(hipStream_t stream, bool need_base = true) {
        CodebookView v = view();
        if (!prepared) prepared_base = prepared_x32 = false;
        if (need_base && !prepared_base) {
            VQ_TRY(launch_prepare_codebook(v, mfma_ok ? prepA.as<float>() : nullptr,
                                           mfma_ok ? prepCn.as<float>() : nullptr, meta.as<float>(),
                                           cnsqrt.as<float>(), stream));
            prepared_base = true;
        }
        if (x32_ok && !prepared_x32) {
            VQ_TRY(launch_prepare_bf16_x32(v, prepA32.as<uint32_t>(), metric == VQHIP_COSINE ? 1 : 0, cbc.as<float>(),
                                           cen.as<float>(), cn32.as<float>(), stream, const_cast<uint32_t *>(v.prepA32_3)));
            prepared_x32 = true;
        }
        prepared = true;
        return VQHIP_OK;
    }
};

// --------------------------------------------------------------- assign workspace ----
struct AssignWorkspace {
    DevBuf wl_rows, wl_count, sub_list, sub_pos, wl_seg, part, codes_t;
    static constexpr uint32_t kSegCap = 4096;  // wave-private work-list segments per subspace
    uint32_t *seg_host = nullptr;               // pinned [m][kSegCap][2]
    uint32_t last_n_seg = 0;
    bool last_segmented = false;  // the last screened pass filled list segments (wl_seg), not the per-subspace counters
    uint64_t wl_stride = 0;
    uint32_t wl_m = 0;
    std::vector<uint32_t> sub_host;
    uint32_t *stats_host = nullptr;  // pinned [m]
    uint32_t stats_m = 0;
    bool stats_pending = false;
    int last_engine = 0;
    int last_products = 0;  // bf16 products per dimension of the last screen kernel (6 or 3), 0 without a bf16 screen
    ~AssignWorkspace() {
        if (stats_host) (void)hipHostFree(stats_host);
        if (seg_host) (void)hipHostFree(seg_host);
    }
    int ensure(uint32_t m, uint64_t n, bool need_wl) {
        if (!sub_list.p || sub_list.bytes < (size_t)m * 4) VQ_TRY(sub_list.alloc((size_t)m * 4));
        if (!sub_pos.p || sub_pos.bytes < (size_t)m * 4) VQ_TRY(sub_pos.alloc((size_t)m * 4));
        if (!wl_count.p || wl_m < m) {
            VQ_TRY(wl_count.alloc((size_t)m * 4));
            if (stats_host) (void)hipHostFree(stats_host);
            stats_host = nullptr;
            VQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&stats_host), (size_t)m * 4));
            memset(stats_host, 0, (size_t)m * 4);
            stats_m = m;
            VQ_TRY(wl_seg.alloc((size_t)m * kSegCap * 8));
            if (seg_host) (void)hipHostFree(seg_host);
            seg_host = nullptr;
            VQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&seg_host), (size_t)m * kSegCap * 8));
        }
        if (need_wl && (wl_stride < n || wl_m < m)) {
            VQ_TRY(wl_rows.alloc((size_t)m * (size_t)n * 4));
            wl_stride = n;
        }
        if (wl_m < m) wl_m = m;
        return VQHIP_OK;
    }
    int set_sub_list(const std::vector<uint32_t> &subs, uint32_t m, hipStream_t stream) {
        if (subs != sub_host) {
            // the previous list may still be read by queued kernels: order on the stream
            std::vector<int32_t> pos(m, -1);  // subspace -> position in the list (the fused update's slab index)
            for (size_t i = 0; i < subs.size(); ++i)
                if (subs[i] < m) pos[subs[i]] = (int32_t)i;
            VQ_HIP(hipMemcpyAsync(sub_list.p, subs.data(), subs.size() * 4, hipMemcpyHostToDevice, stream));
            VQ_HIP(hipMemcpyAsync(sub_pos.p, pos.data(), (size_t)m * 4, hipMemcpyHostToDevice, stream));
            VQ_HIP(hipStreamSynchronize(stream));
            sub_host = subs;
        }
        return VQHIP_OK;
    }
};

// Optional per-call HIP-event timing of the two assignment stages, recorded on the stream
// the kernels are launched on (bench.py derives the roofline figure from it).
struct ProfileState {
    bool on = false;
    std::vector<hipEvent_t> ev;  // triples: start, after screen (or exact), after re-check
    std::vector<int> engines;
};
static thread_local ProfileState g_prof;

static int pick_engine(int requested, const CodebookState &cs, int metric, int *engine) {
    const bool l2_metric = (metric == VQHIP_SQUARED_EUCLIDEAN || metric == VQHIP_EUCLIDEAN);
    // cosine has a screen too (s = -x.c/|c| on the X32 bf16 engine); Manhattan has no contraction form
    const bool cos_ok = (metric == VQHIP_COSINE) && cs.x32_ok && cs.metric == VQHIP_COSINE;
    if (requested == VQHIP_ENGINE_EXACT) {
        *engine = VQHIP_ENGINE_EXACT;
    } else if (requested == VQHIP_ENGINE_MFMA) {
        if (!cs.mfma_ok || !l2_metric)
            return fail(VQHIP_ERR_UNSUPPORTED, "fp32 MFMA engine unavailable for sub_dim=%u k=%u metric=%d",
                        cs.sd, cs.k, metric);
        *engine = VQHIP_ENGINE_MFMA;
    } else if (requested == VQHIP_ENGINE_MFMA_BF16) {
        if (!((cs.bf16_ok && l2_metric) || cos_ok))
            return fail(VQHIP_ERR_UNSUPPORTED, "bf16 MFMA engine unavailable for sub_dim=%u k=%u metric=%d",
                        cs.sd, cs.k, metric);
        *engine = VQHIP_ENGINE_MFMA_BF16;
    } else {
        *engine = cos_ok                     ? VQHIP_ENGINE_MFMA_BF16
                  : !l2_metric               ? VQHIP_ENGINE_EXACT
                  : cs.bf16_ok               ? VQHIP_ENGINE_MFMA_BF16
                  : cs.mfma_ok               ? VQHIP_ENGINE_MFMA
                                             : VQHIP_ENGINE_EXACT;
    }
    return VQHIP_OK;
}

// Fused update of a training step: the screen adds the rows it proves into partial slabs, the rows it
// re-checks are added by a list-driven pass behind the re-check.  in: buffers + capacity in slabs; out: used / chunks.
struct FusedAcc {
    float *sums = nullptr;
    uint32_t *counts = nullptr;
    uint32_t slab_cap = 0;   // slabs of [k][sd] available (one per (chunk, active subspace))
    uint32_t n_patch = 16;   // list-driven chunks behind the screen's
    bool used = false;       // out: the launch sequence took the fused path
    uint32_t chunks = 0;     // out: chunks to reduce (screen + patch)
    const uint8_t *gate_active = nullptr;  // vqhip_kmeans_run: device-side gates handed to the screen
    const uint32_t *gate_halt = nullptr;
};

// assignment of every row of X [n][d] for the listed subspaces -> codes [n][m]
static int run_assign(CodebookState &cs, AssignWorkspace &ws, const float *X, uint64_t n, uint32_t d,
                      int metric, const std::vector<uint32_t> &subs, uint8_t *codes, int engine_req,
                      hipStream_t stream, FusedAcc *fused = nullptr) {
    if (n == 0 || subs.empty()) return VQHIP_OK;
    if (n >= (1ull << 32)) return fail(VQHIP_ERR_UNSUPPORTED, "more than 2^32-1 rows per device");
    if ((reinterpret_cast<uintptr_t>(X) & 15) != 0)
        return fail(VQHIP_ERR_INVALID_INPUT, "device row buffer must be 16-byte aligned");
    int engine = 0;
    VQ_TRY(pick_engine(engine_req, cs, metric, &engine));
    // k > 256 on the grouped X32 screen keeps a 16-byte partial verdict per (row, subspace, group): past 4 GiB
    // of them the exact scan is used instead (unless the caller asked for the screen by name)
    if (engine == VQHIP_ENGINE_MFMA_BF16 && engine_req == VQHIP_ENGINE_AUTO && cs.k > 256 &&
        (size_t)cs.m * cs.x32_groups * n * 16 > ((size_t)4 << 30))
        engine = VQHIP_ENGINE_EXACT;
    // small work (C1's encode: 10k rows x 4 subspaces x 16 centroids x 16 dimensions): the exact scan is one launch of a
    // few microseconds, the screen is two (+ its codebook images) -- launch latency is all there is at that size
    if (engine_req == VQHIP_ENGINE_AUTO && engine != VQHIP_ENGINE_EXACT && !(fused && fused->sums) &&
        (double)n * cs.m * cs.k * cs.sd <= 32.0e6)
        engine = VQHIP_ENGINE_EXACT;
    const bool x32_only = engine == VQHIP_ENGINE_MFMA_BF16 && cs.x32_groups == 1 && x32_padded_sd(cs.sd) <= 64 &&
                          (metric == VQHIP_SQUARED_EUCLIDEAN || metric == VQHIP_EUCLIDEAN) && cs.metric != VQHIP_COSINE;
    VQ_TRY(cs.prepare(stream, !x32_only));
    const bool screened = (engine == VQHIP_ENGINE_MFMA || engine == VQHIP_ENGINE_MFMA_BF16);
    VQ_TRY(ws.ensure(cs.m, n, screened));
    VQ_TRY(ws.set_sub_list(subs, cs.m, stream));
    AssignArgs a;
    a.X = X;
    a.n = n;
    a.d = d;
    a.metric = metric;
    a.encode = (fused == nullptr);
    a.sub_list = ws.sub_list.as<uint32_t>();
    a.n_sub = (uint32_t)subs.size();
    a.codes = codes;
    a.wl_rows = ws.wl_rows.as<uint32_t>();
    a.wl_count = ws.wl_count.as<uint32_t>();
    a.wl_stride = ws.wl_stride;
    a.wl_seg = ws.wl_seg.as<uint32_t>();
    a.wl_seg_cap = AssignWorkspace::kSegCap;
    a.n_seg = 0;
    if (engine == VQHIP_ENGINE_MFMA_BF16 && (cs.x32_groups > 1 || x32_padded_sd(cs.sd) > 64)) {  // (the wide kernel goes through the partial verdicts even with one group)
        VQ_TRY(ws.part.ensure((size_t)cs.m * cs.x32_groups * n * 16));
        a.part = ws.part.p;
    }
    // many subspaces: the single-pass bf16 screen writes its codes subspace-major into a scratch and a transposition
    // forms [n][m] (k_screen_bf16.hip): at m = 96 the byte stores m apart were 1.46 GB of write traffic for 96 MB of codes
    const bool ct_shape = engine == VQHIP_ENGINE_MFMA_BF16 && cs.x32_groups == 1 && x32_padded_sd(cs.sd) <= 64 && cs.k <= 256 &&
                          cs.m % 4 == 0 && (size_t)256 * codes_transpose_pitch(cs.m) + cs.m <= 60 * 1024 && (reinterpret_cast<uintptr_t>(codes) & 3) == 0;
    if (ct_shape && cs.m >= 16) {
        const uint64_t pitch = (n + 255) / 256 * 256;
        VQ_TRY(ws.codes_t.ensure((size_t)cs.m * pitch));
        a.codes_t = ws.codes_t.as<uint8_t>();
        a.codes_t_pitch = pitch;
    }
    if (fused) fused->used = false;
    if (fused && fused->sums && engine == VQHIP_ENGINE_MFMA_BF16 && metric != VQHIP_COSINE && cs.x32_groups == 1 &&
        screen_bf16_fused_update_supported(cs.sd, cs.k) && fused->slab_cap / a.n_sub > fused->n_patch) {
        a.acc_sums = fused->sums;
        a.acc_counts = fused->counts;
        a.acc_chunk_cap = fused->slab_cap / a.n_sub - fused->n_patch;
        a.gate_active = fused->gate_active;
        a.gate_halt = fused->gate_halt;
    }
    CodebookView v = cs.view();
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (g_prof.on) {
        VQ_HIP(hipEventCreate(&e0));
        VQ_HIP(hipEventCreate(&e1));
        VQ_HIP(hipEventCreate(&e2));
        g_prof.ev.push_back(e0);
        g_prof.ev.push_back(e1);
        g_prof.ev.push_back(e2);
        g_prof.engines.push_back(engine);
    }
    if (screened) {
        // the single-pass bf16 screen fills wave-private list SEGMENTS (wl_seg); only the other screens append to the
        // per-subspace counters, which must start at zero
        const bool segmented = engine == VQHIP_ENGINE_MFMA_BF16 && cs.x32_groups == 1 && x32_padded_sd(cs.sd) <= 64;
        if (!segmented) VQ_HIP(hipMemsetAsync(ws.wl_count.p, 0, (size_t)cs.m * 4, stream));
        if (e0) VQ_HIP(hipEventRecord(e0, stream));
        if (engine == VQHIP_ENGINE_MFMA_BF16) VQ_TRY(launch_assign_screen_bf16(v, a, stream));
        else VQ_TRY(launch_assign_screen(v, a, stream));
        if (e1) VQ_HIP(hipEventRecord(e1, stream));
        VQ_TRY(launch_assign_exact(v, a, true, stream));
        if (a.acc_sums) {  // the re-checked rows, now that their codes are final
            VQ_TRY(launch_accumulate_listed(cs.m, cs.k, cs.sd, X, d, codes, a.sub_list, a.n_sub, a.wl_rows, a.wl_stride, a.wl_seg,
                                            a.n_seg, a.acc_chunks, fused->n_patch, a.acc_sums, a.acc_counts, stream));
            fused->used = true;
            fused->chunks = a.acc_chunks + fused->n_patch;
        }
        if (e2) VQ_HIP(hipEventRecord(e2, stream));
        // the re-check counts stay on the device: vqhip_last_assign_stats fetches them when somebody asks (a copy queued
        // behind every pass was one of five stream operations of a 10k-row encode)
        ws.last_n_seg = a.n_seg;
        ws.last_segmented = segmented;
        ws.stats_pending = true;
    } else {
        if (e0) VQ_HIP(hipEventRecord(e0, stream));
        VQ_TRY(launch_assign_exact(v, a, false, stream));
        if (e1) VQ_HIP(hipEventRecord(e1, stream));
        if (e2) VQ_HIP(hipEventRecord(e2, stream));
        ws.stats_pending = false;
    }
    ws.last_engine = engine;
    ws.last_products = (engine == VQHIP_ENGINE_MFMA_BF16) ? (int)a.products : 0;
    ThreadState &st = tls();
    st.last_engine = engine;
    st.last_products = ws.last_products;
    st.last_rechecked = 0;
    return VQHIP_OK;
}

// ----------------------------------------------------------- handles under threads ----
// The reference's quantizers are plain data (src/pq.rs:39-45, src/tsvq.rs:186-191): `Send + Sync`, and
// `quantize(&self)` may run on many threads at once.  Here a handle owns device workspaces and work is queued on the
// CALLING thread's stream, so two things are needed for the same guarantee:
//   * one recursive mutex per handle around every entry point that touches the handle's state (entry points call each
//     other: vqhip_pq_encode -> _device, vqhip_kmeans_run -> _step -> _set_active);
//   * stream order across threads: a call that returns with work still queued leaves a tail (its stream); the next
//     call on ANOTHER stream first waits for that tail through an event.  The event is recorded when the other
//     stream shows up if the tail is one of the library's own per-thread streams (never destroyed); for a caller's
//     stream (vqhip_set_stream) it is recorded when the call leaves, because the caller may destroy that stream later.
struct HandleSync {
    std::recursive_mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t tail = nullptr;  // stream holding queued work of this handle (nullptr: the last call synchronised)
    bool tail_lazy = false;      // the event for `tail` has not been recorded yet (library-owned stream)
    int depth = 0;
    ~HandleSync() {
        if (ev) (void)hipEventDestroy(ev);
    }
    int event() {
        if (!ev) VQ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return VQHIP_OK;
    }
    // order stream s behind whatever this handle still has queued elsewhere
    int order(hipStream_t s) {
        if (tail && tail != s) {
            VQ_TRY(event());
            if (tail_lazy) VQ_HIP(hipEventRecord(ev, tail));
            VQ_HIP(hipStreamWaitEvent(s, ev, 0));
            tail = nullptr;
        }
        return VQHIP_OK;
    }
    void leave(hipStream_t s, bool synced) {
        if (synced || !s) {
            if (synced) tail = nullptr;
            return;
        }
        tail = s;
        tail_lazy = true;
        if (tls().user_stream_set && tls().user_stream == s) {
            if (event() == VQHIP_OK && hipEventRecord(ev, s) == hipSuccess) tail_lazy = false;
        }
    }
};

// RAII for one entry point: lock, order the calling thread's stream behind the handle's tail, and on the way out
// note whether the call left work queued (the default) or synchronised its stream (`synced()`).
class Entry {
   public:
    explicit Entry(HandleSync &h) : h_(&h) {
        h_->mu.lock();
        ++h_->depth;
    }
    ~Entry() { release(); }
    Entry(const Entry &) = delete;
    Entry &operator=(const Entry &) = delete;
    int stream(hipStream_t *out) {
        VQ_TRY(current_stream(&s_));
        VQ_TRY(h_->order(s_));
        *out = s_;
        return VQHIP_OK;
    }
    void synced() { synced_ = true; }
    // give the handle back before the call ends (the rest of the call touches nothing the handle owns mutably)
    void release() {
        if (!h_) return;
        if (--h_->depth == 0) h_->leave(s_, synced_);
        h_->mu.unlock();
        h_ = nullptr;
    }

   private:
    HandleSync *h_;
    hipStream_t s_ = nullptr;
    bool synced_ = false;
};

// vqhip_last_assign_stats names "the most recent pass of this thread" by workspace; the workspace may belong to a
// handle another thread destroys, so the thread-local note is an id looked up in a registry of live workspaces.
struct WsEntry {
    AssignWorkspace *ws;
    HandleSync *sync;
    int pins = 0;  // vqhip_last_assign_stats queries in flight: the handle's destructor waits for them
};
static std::mutex g_ws_mu;
static std::condition_variable g_ws_cv;
static std::map<uint64_t, WsEntry> g_ws_live;
static std::atomic<uint64_t> g_ws_next{1};
static thread_local uint64_t g_last_ws = 0;  // registry id, 0 = none

static uint64_t ws_register(AssignWorkspace *ws, HandleSync *sync) {
    const uint64_t id = g_ws_next.fetch_add(1);
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws_live[id] = WsEntry{ws, sync, 0};
    return id;
}
static void ws_unregister(uint64_t id) {
    std::unique_lock<std::mutex> lk(g_ws_mu);
    auto it = g_ws_live.find(id);
    if (it == g_ws_live.end()) return;
    g_ws_cv.wait(lk, [&] { return it->second.pins == 0; });  // only THIS handle's destructor waits for a query on it
    g_ws_live.erase(it);
}
// a live workspace pinned for one query: the registry lock is held only to look it up and to let it go, so a query that
// blocks behind a long call on its handle stalls no other handle's constructor / destructor
struct WsPin {
    uint64_t id = 0;
    AssignWorkspace *ws = nullptr;
    HandleSync *sync = nullptr;
    explicit WsPin(uint64_t want) {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        auto it = g_ws_live.find(want);
        if (it == g_ws_live.end()) return;
        ++it->second.pins;
        id = want;
        ws = it->second.ws;
        sync = it->second.sync;
    }
    ~WsPin() {
        if (!id) return;
        std::lock_guard<std::mutex> lk(g_ws_mu);
        auto it = g_ws_live.find(id);
        if (it != g_ws_live.end() && --it->second.pins == 0) g_ws_cv.notify_all();
    }
    WsPin(const WsPin &) = delete;
    WsPin &operator=(const WsPin &) = delete;
};


}  // namespace vqhip

using namespace vqhip;

// ------------------------------------------------------------------------ handles ----
struct vqhip_dataset {
    DevBuf own;
    const float *X = nullptr;
    uint64_t n = 0;
    uint32_t d = 0;
    mutable TsvqPolicyCache tsvq_policy;  // (library-owned rows only: a borrowed buffer may change between builds)
};

struct vqhip_kmeans {
    HandleSync sync;
    uint64_t ws_id = 0;
    const vqhip_dataset *ds = nullptr;
    CodebookState cs;
    AssignWorkspace ws;
    UpdatePlan plan;
    DevBuf codes, partial_sums, partial_counts, slab, counts, changed, active_dev, rows_tmp, xs_ws, gather_ws;
    DevBuf agree;      // two words the ranks of a sharded run all-reduce before anything is queued
    DevBuf sm_psum, sm_pcnt, sm_tick;  // k_lloyd_small.hip: partials per 64-row range, the two flag sets of a device-driven run
    DevBuf run_state;  // vqhip_kmeans_run: [0] halt flag, [1 .. m] iterations executed per subspace, [m+1], [m+2] k_finalize's own
    std::vector<uint8_t> active;
    bool all_active = true;
    int engine = VQHIP_ENGINE_AUTO;
    int exact_update = 0;
    uint32_t fused_slabs = 0;     // > 0: partial buffers sized for the fused update (screen + list-driven slabs)
    bool sums_by_chains = false;  // sub_dim beyond the LDS update kernels: cluster sums always through launch_exact_sums
    bool chain_update = false;    // no wave-owned accumulate for this shape / row alignment: the unfused update's sums through launch_exact_sums
    bool accumulated = false;
    uint32_t *counts_host = nullptr;   // pinned [m*k]
    uint32_t *changed_host = nullptr;  // pinned [m]
    // pinned, vqhip_kmeans_run's read-back: {paused, iterations [m]} | small-problem flag sets [6 m] | active set [m bytes].
    // (Read into vectors on the stack, every one of those copies was a staged pageable copy with a wait of its own: 85 us per
    // call, whatever the number of iterations -- a third of a ten-iteration run at 10k rows.)
    uint32_t *run_host = nullptr;
    // launch-bound regime (small n): one Lloyd step = ~14 stream operations, replayed as a hipGraph
    hipGraphExec_t graph_exec = nullptr;
    hipStream_t graph_stream = nullptr;
    uint64_t graph_key = 0, warm_key = 0;
    bool graph_failed = false;
    void drop_graph() {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        graph_exec = nullptr;
    }
    vqhip_kmeans() { ws_id = ws_register(&ws, &sync); }
    ~vqhip_kmeans() {
        ws_unregister(ws_id);
        drop_graph();
        if (counts_host) (void)hipHostFree(counts_host);
        if (changed_host) (void)hipHostFree(changed_host);
        if (run_host) (void)hipHostFree(run_host);
    }
};

struct vqhip_comm {
    std::recursive_mutex mu;  // an ncclComm_t takes one enqueueing thread at a time
    Comm *c = nullptr;
};

// Pinned, device-mapped staging for the per-vector latency path (k_small.hip)
struct PinnedStage {
    void *host = nullptr, *dev = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return VQHIP_OK;
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
        bytes = 0;
        const size_t cap = need < 65536 ? 65536 : need;
        VQ_HIP(hipHostMalloc(&host, cap, hipHostMallocMapped));
        VQ_HIP(hipHostGetDevicePointer(&dev, host, 0));
        bytes = cap;
        return VQHIP_OK;
    }
    ~PinnedStage() {
        if (host) (void)hipHostFree(host);
    }
};
constexpr uint64_t kSmallRows = 8;  // calls with at most this many host rows take the one-kernel path

// ------------------------------------------------- host <-> device streaming for large batches ----
// What this pool's boxes deliver (profiles/ubench/pcie_duplex.hip, tools/host_xfer.py): a copy between device memory
// and host pages that have been touched runs at 55-57 GB/s each way whether the pages are pinned or not, both ways at
// once if TWO host threads issue them (a pageable copy occupies its thread); staging through pinned buffers with host
// memcpys (29 GB/s per thread) only loses (measured: 4 lanes of pinned staging 6.1e7 vectors/s against 7.1e7 for the
// plain copies in turn, rows in / f16 out at 1M x 128).  So a large host batch whose results are a sizeable share of
// its input goes through LANES: a few host threads (three), each with its own stream and device buffers, take every
// n-th chunk end to end -- H2D straight from the caller's rows, the kernels (the handle orders the lanes' launches on the
// device: HandleSync), D2H straight into the caller's buffers -- so one lane's results travel while the other lane's rows do.
struct XferLane {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf dev_in, dev_out, dev_out2;
    int ensure() {
        if (!stream) VQ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return VQHIP_OK;
    }
};
// host threads per large transfer: two suffice when they stay out of phase (9.7 ms at 1M x 128 rows in / f16 out), but
// now and then a call fell back to 14 ms; three took 10.2-10.5 ms every time
constexpr int kXferLanes = 3;
constexpr size_t kXferChunkBytes = (size_t)32 << 20;  // bytes of input per chunk
constexpr size_t kXferMinBytes = (size_t)96 << 20;  // smaller batches keep the one-stream path (two host threads to start)
// lanes pay when the results are at least a quarter of the rows in bytes (f16 reconstructions); codes alone are 1-6 %
static bool xfer_lanes_pay(size_t in_b, size_t out_b) { return in_b >= kXferMinBytes && 4 * out_b >= in_b; }
struct XferPool {  // leaked on purpose, like StagePool
    std::mutex mu;
    std::vector<XferLane *> idle;
};
static XferPool &xfer_pool() {
    static XferPool *p = new XferPool();
    return *p;
}
// fn(lane index, lane, lanes) on that many host threads (each bound to the caller's device); the first failure's status
// and text come back on the calling thread
static std::atomic<uint64_t> g_xfer_lane_calls{0};
template <class Fn>
static int run_lanes(Fn fn) {
    int dev = 0;
    VQ_HIP(hipGetDevice(&dev));
    g_xfer_lane_calls.fetch_add(1);
    const int n_lanes = kXferLanes;
    XferLane *lanes[kXferLanes] = {};
    {
        XferPool &p = xfer_pool();
        std::lock_guard<std::mutex> lk(p.mu);
        int got = 0;
        for (size_t i = 0; i < p.idle.size() && got < n_lanes;)
            if (p.idle[i]->device == dev) {
                lanes[got++] = p.idle[i];
                p.idle.erase(p.idle.begin() + (long)i);
            } else {
                ++i;
            }
        for (; got < n_lanes; ++got) {
            lanes[got] = new XferLane();
            lanes[got]->device = dev;
        }
    }
    int rcs[kXferLanes];
    std::string errs[kXferLanes];
    std::thread th[kXferLanes];
    for (int t = 0; t < n_lanes; ++t)
        th[t] = std::thread([&, t] {
            rcs[t] = VQHIP_OK;
            if (hipSetDevice(dev) != hipSuccess) {
                rcs[t] = VQHIP_ERR_RUNTIME;
                errs[t] = "hipSetDevice failed on a transfer lane";
                return;
            }
            rcs[t] = lanes[t]->ensure();
            if (rcs[t] == VQHIP_OK) {
                ThreadState &st = tls();
                st.user_stream = lanes[t]->stream, st.user_stream_set = true;  // this thread's launches go to the lane's stream
                rcs[t] = fn(t, *lanes[t], n_lanes);
            }
            if (rcs[t] != VQHIP_OK) errs[t] = tls().last_error;
        });
    for (int t = 0; t < n_lanes; ++t) th[t].join();
    {
        XferPool &p = xfer_pool();
        std::lock_guard<std::mutex> lk(p.mu);
        for (int t = 0; t < n_lanes; ++t) p.idle.push_back(lanes[t]);
    }
    for (int t = 0; t < n_lanes; ++t)
        if (rcs[t] != VQHIP_OK) return fail(rcs[t], "%s", errs[t].c_str());
    return VQHIP_OK;
}

// The per-vector path stages through a buffer that belongs to the CALL, not to the handle: `quantize(&self)` from many
// threads on one quantizer then overlaps on the device (each thread its own stream and staging) instead of queueing on
// the handle's lock.  Buffers are pooled per device and never returned to the runtime (64 KB each, as many as there
// were concurrent calls); the pool itself is leaked on purpose -- static destructors run after the HIP runtime's.
struct StagePool {
    std::mutex mu;
    std::vector<std::pair<int, PinnedStage *>> idle;
};
static StagePool &stage_pool() {
    static StagePool *p = new StagePool();
    return *p;
}
class StageLease {
   public:
    StageLease() = default;
    StageLease(const StageLease &) = delete;
    StageLease &operator=(const StageLease &) = delete;
    ~StageLease() {
        if (!st_) return;
        std::lock_guard<std::mutex> lk(stage_pool().mu);
        stage_pool().idle.emplace_back(dev_, st_);
    }
    int acquire(size_t need) {
        VQ_HIP(hipGetDevice(&dev_));
        {
            StagePool &p = stage_pool();
            std::lock_guard<std::mutex> lk(p.mu);
            for (size_t i = 0; i < p.idle.size(); ++i)
                if (p.idle[i].first == dev_) {
                    st_ = p.idle[i].second;
                    p.idle.erase(p.idle.begin() + (long)i);
                    break;
                }
        }
        if (!st_) st_ = new PinnedStage();
        return st_->ensure(need);
    }
    char *host() const { return static_cast<char *>(st_->host); }
    char *dev() const { return static_cast<char *>(st_->dev); }

   private:
    PinnedStage *st_ = nullptr;
    int dev_ = 0;
};

// wait for a ~10-40 us kernel by polling: hipStreamSynchronize parks the thread after a short spin and
// then costs ~100 us to wake up (measured 134 us per TSVQ quantize call against a 14 us kernel)
static int spin_wait(hipStream_t s) {
    for (int i = 0; i < 200000; ++i) {
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return VQHIP_OK;
        if (e != hipErrorNotReady) return fail(VQHIP_ERR_RUNTIME, "stream query failed: %s", hipGetErrorString(e));
    }
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
}

// One rule carries a caller's host rows through a device-form launch and back, for every host form with tiers (PQ and
// TSVQ encode, the SQ / BQ maps):
//   * per-vector: a call the caller judges tiny stages through a call-owned pinned, device-mapped buffer (input, then the
//     outputs at 16-byte-aligned offsets), makes one launch that reads and writes host memory, and polls;
//   * transfer lanes: a batch of kXferMinBytes and more whose results are at least a quarter of its input
//     (xfer_lanes_pay) goes through run_lanes in chunks of kXferChunkBytes of input;
//   * one stream: anything else, in passes of at most 1 GiB of input through the buffers the caller names.
// A handle's call passes its Entry: the handle is given back before the per-vector launch and before the lanes (which
// take it per chunk through the device form), and the one-stream passes leave the stream synchronised.
// Both launches are `launch(dev_in, rows, dev_out0, dev_out1, stream)`; dev_out1 is null when out1 is.
enum class XferTier { kVector, kLanes, kStream };
struct HostBatch {
    const void *in;
    size_t in_b;     // bytes per row (SQ / BQ: per element); out0_b and out1_b likewise
    void *out0;      // null: still written on the device (the launch needs it), not copied back
    size_t out0_b;
    void *out1;      // null: not produced
    size_t out1_b;
    uint64_t rows;
    uint64_t grain;  // chunks hold a multiple of this many rows
    size_t out0_off() const { return ((size_t)rows * in_b + 15) & ~(size_t)15; }
    size_t out1_off() const { return out0_off() + (((size_t)rows * out0_b + 15) & ~(size_t)15); }
    size_t stage_bytes() const { return out1 ? out1_off() + (size_t)rows * out1_b : out0_off() + (size_t)rows * out0_b; }
};
constexpr size_t kElementwiseSmallBytes = 65536;  // SQ / BQ: per-vector while the staging fits this

template <class VecLaunch, class ChunkLaunch>
static int host_batch(const HostBatch &b, Entry *entry, bool per_vector, VecLaunch vec_launch, ChunkLaunch chunk_launch,
                      DevBuf &buf_in, DevBuf &buf_out0, DevBuf &buf_out1, XferTier *tier = nullptr) {
    const uint64_t n = b.rows, g = b.grain;
    const char *in = static_cast<const char *>(b.in);
    char *out0 = static_cast<char *>(b.out0), *out1 = static_cast<char *>(b.out1);
    hipStream_t s;
    if (per_vector) {
        if (tier) *tier = XferTier::kVector;
        if (entry) entry->release();
        VQ_TRY(current_stream(&s));
        StageLease stage;
        VQ_TRY(stage.acquire(b.stage_bytes()));
        char *hb = stage.host(), *db = stage.dev();
        memcpy(hb, in, (size_t)n * b.in_b);
        VQ_TRY(vec_launch(db, n, db + b.out0_off(), out1 ? db + b.out1_off() : nullptr, s));
        VQ_TRY(spin_wait(s));
        if (out0) memcpy(out0, hb + b.out0_off(), (size_t)n * b.out0_b);
        if (out1) memcpy(out1, hb + b.out1_off(), (size_t)n * b.out1_b);
        return VQHIP_OK;
    }
    if (xfer_lanes_pay((size_t)n * b.in_b, (out0 ? (size_t)n * b.out0_b : 0) + (out1 ? (size_t)n * b.out1_b : 0))) {
        if (entry) {
            VQ_TRY(entry->stream(&s));  // (what the handle still has queued stays its tail: the lanes order behind it)
            entry->release();
        }
        if (tier) *tier = XferTier::kLanes;
        const uint64_t per = std::max<uint64_t>(g, kXferChunkBytes / b.in_b / g * g), chunks = (n + per - 1) / per;
        std::mutex h2d_turn;  // one lane's rows on the bus at a time: the lanes stay out of phase (both copying in, then both out, overlaps nothing: 13.3 against 10.6 ms)
        return run_lanes([&](int t, XferLane &ln, int n_lanes) -> int {
            VQ_TRY(ln.dev_in.ensure((size_t)per * b.in_b));
            VQ_TRY(ln.dev_out.ensure((size_t)per * b.out0_b));
            if (out1) VQ_TRY(ln.dev_out2.ensure((size_t)per * b.out1_b));
            for (uint64_t c = (uint64_t)t; c < chunks; c += (uint64_t)n_lanes) {
                const uint64_t r0 = c * per, nr = std::min(per, n - r0);
                {
                    std::lock_guard<std::mutex> turn(h2d_turn);
                    VQ_HIP(hipMemcpyAsync(ln.dev_in.p, in + r0 * b.in_b, (size_t)nr * b.in_b, hipMemcpyHostToDevice, ln.stream));
                    VQ_HIP(hipStreamSynchronize(ln.stream));
                }
                VQ_TRY(chunk_launch(ln.dev_in.p, nr, ln.dev_out.p, out1 ? ln.dev_out2.p : nullptr, ln.stream));
                if (out0) VQ_HIP(hipMemcpyAsync(out0 + r0 * b.out0_b, ln.dev_out.p, (size_t)nr * b.out0_b, hipMemcpyDeviceToHost, ln.stream));
                if (out1) VQ_HIP(hipMemcpyAsync(out1 + r0 * b.out1_b, ln.dev_out2.p, (size_t)nr * b.out1_b, hipMemcpyDeviceToHost, ln.stream));
                VQ_HIP(hipStreamSynchronize(ln.stream));
            }
            return VQHIP_OK;
        });
    }
    if (tier) *tier = XferTier::kStream;
    if (entry) VQ_TRY(entry->stream(&s));
    else VQ_TRY(current_stream(&s));
    const uint64_t chunk = std::min<uint64_t>(n, std::max<uint64_t>(g, (1ull << 30) / b.in_b / g * g));
    VQ_TRY(buf_in.ensure((size_t)chunk * b.in_b));
    VQ_TRY(buf_out0.ensure((size_t)chunk * b.out0_b));
    if (out1) VQ_TRY(buf_out1.ensure((size_t)chunk * b.out1_b));
    for (uint64_t r0 = 0; r0 < n; r0 += chunk) {
        const uint64_t nr = std::min(chunk, n - r0);
        VQ_HIP(hipMemcpyAsync(buf_in.p, in + r0 * b.in_b, (size_t)nr * b.in_b, hipMemcpyHostToDevice, s));
        VQ_TRY(chunk_launch(buf_in.p, nr, buf_out0.p, out1 ? buf_out1.p : nullptr, s));
        if (out0) VQ_HIP(hipMemcpyAsync(out0 + r0 * b.out0_b, buf_out0.p, (size_t)nr * b.out0_b, hipMemcpyDeviceToHost, s));
        if (out1) VQ_HIP(hipMemcpyAsync(out1 + r0 * b.out1_b, buf_out1.p, (size_t)nr * b.out1_b, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
    }
    if (entry) entry->synced();
    return VQHIP_OK;
}

// host codes (one or two bytes each, the caller's pointer at any alignment) inside [0, k)
static int check_codes(const uint8_t *codes, uint64_t count, uint32_t k) {
    const bool wide = code_bytes(k) == 2;
    for (uint64_t i = 0; i < count; ++i) {
        uint32_t c = codes[i];
        if (wide) {
            uint16_t w;
            memcpy(&w, codes + 2 * i, 2);
            c = w;
        }
        if (c >= k) return fail(VQHIP_ERR_INVALID_INPUT, "code %u at element %llu is outside [0, %u)", c, (unsigned long long)i, k);
    }
    return VQHIP_OK;
}

struct vqhip_pq_encoder {
    HandleSync sync;
    uint64_t ws_id = 0;
    vqhip_pq_encoder() { ws_id = ws_register(&ws, &sync); }
    ~vqhip_pq_encoder() { ws_unregister(ws_id); }
    CodebookState cs;
    AssignWorkspace ws;
    int metric = VQHIP_EUCLIDEAN;
    int engine = VQHIP_ENGINE_AUTO;
    DevBuf xbuf, codes, f16buf, f32buf, adc_q, adc_lut, adc_dist, adc_idx, adc_out, adc_codes, adc_state, adc_cand, adc_redo, adc_resident;
    DevBuf adc_mask;               // a filtered ADC call's row mask on the device
    uint64_t adc_resident_n = 0;   // rows of the code store vqhip_pq_adc_set_codes uploaded
    uint32_t adc_last_redone = 0;  // queries of the last ADC call that went through the full pass
    std::vector<uint32_t> all_subs;
    // the per-vector path's images (codebooks, cosine norms) are complete on the DEVICE -- set only after a host wait behind
    // their prepare kernels; `cs.prepared` alone says they were ENQUEUED, possibly on another thread's stream
    bool small_ready = false;
};

struct vqhip_tsvq {
    HandleSync sync;
    uint32_t n_nodes = 0, d = 0;
    int metric = VQHIP_EUCLIDEAN;
    DevBuf centroids, cnorm, left, right, xbuf, leafbuf, f16buf, table16;
    // screened descent (k_tsvq_screen.hip); use_screen = false -> exact walk only
    bool use_screen = false, last_screened = false;
    TsvqScreen scr;
    DevBuf scr_w, scr_info, scr_mu, scr_wl, scr_count, scr_slot_node, scr_node_slot;
};

// Per-node data of the screened descent, from the host copy of the tree (f64, rounded once).
static int tsvq_prepare_screen(vqhip_tsvq *t, const float *centroids, const int32_t *left, const int32_t *right,
                               hipStream_t s) {
    const uint32_t n_nodes = t->n_nodes, d = t->d;
    uint32_t n_int = 0;
    for (uint32_t i = 0; i < n_nodes; ++i) n_int += (left[i] >= 0 && right[i] >= 0) ? 1u : 0u;
    const char *off = getenv("VQHIP_TSVQ_EXACT");
    if ((off && off[0] == '1') || n_int == 0 || !tsvq_screen_supported(1, n_nodes, d, t->metric)) return VQHIP_OK;
    // A tree too large for one CU's LDS: the two-child nodes are given slots in breadth-first order, the first
    // n_lds of them (the levels nearest the root) live in LDS, the kernel reads the others' w / record from L2.
    uint32_t n_lds = n_int;
    while (n_lds > 1 && !tsvq_screen_supported(n_lds, n_nodes, d, t->metric)) --n_lds;
    const uint32_t dp = tsvq_screen_width(d);  // >= d: width of the kernel's w / mu rows (zeros behind d)
    const bool cosine = t->metric == VQHIP_COSINE, manhattan = t->metric == VQHIP_MANHATTAN;
    const uint32_t nv = (cosine || manhattan) ? 2u : 1u;  // vectors per slot
    std::vector<float> cn32;               // cosine: the reference's f32 centroid norms, as the device computed them
    if (cosine) {
        cn32.resize(n_nodes);
        VQ_HIP(hipMemcpyAsync(cn32.data(), t->cnorm.p, (size_t)n_nodes * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
    }
    std::vector<float> w((size_t)n_int * nv * dp, 0.0f);
    std::vector<int32_t> info((size_t)n_int * 4), slot_node(n_int), slot_of(n_nodes, -1);
    const float *mu = centroids;  // root
    double r2max = 0.0;
    bool finite = true;
    std::vector<double> a2(n_nodes);
    for (uint32_t i = 0; i < n_nodes; ++i) {
        double acc = 0.0;
        for (uint32_t q = 0; q < d; ++q) {
            const double a = (double)centroids[(size_t)i * d + q] - (double)mu[q];
            acc += a * a;
        }
        a2[i] = acc;
        if (!(acc <= 1e300)) finite = false;
        if (acc > r2max) r2max = acc;
    }
    uint32_t slot = 0;
    {
        std::vector<int32_t> queue;  // breadth-first: the levels nearest the root get the LDS slots
        queue.reserve(n_nodes);
        queue.push_back(0);
        for (size_t qi = 0; qi < queue.size(); ++qi) {
            const int32_t i = queue[qi];
            if (left[i] >= 0 && right[i] >= 0) {
                slot_of[i] = (int32_t)slot;
                slot_node[slot++] = i;
            }
            if (left[i] >= 0) queue.push_back(left[i]);
            if (right[i] >= 0) queue.push_back(right[i]);
        }
    }
    // where a walk entering node i first has to decide (slot >= 0) or ends (leaf: -1-node); one-child
    // nodes just pass the row on (tsvq.rs:124-129)
    auto resolve = [&](int32_t i) {
        for (;;) {
            const int32_t l = left[i], r = right[i];
            if (l >= 0 && r >= 0) return slot_of[i];
            if (l < 0 && r < 0) return -1 - i;
            i = (l >= 0) ? l : r;
        }
    };
    for (uint32_t sl = 0; sl < n_int; ++sl) {
        const int32_t i = slot_node[sl], l = left[i], r = right[i];
        int32_t *rec = info.data() + (size_t)sl * 4;
        if (manhattan) {
            // the children's centroids as they are; both L1 sums are within a relative gamma of the same exact sum of
            // the reference's own terms: m = 2.01 (d + D/32 + 6) u (+1 % for the threshold's own arithmetic)
            for (uint32_t side = 0; side < 2; ++side)
                memcpy(&w[((size_t)sl * 2 + side) * dp], centroids + (size_t)(side == 0 ? l : r) * d, (size_t)d * 4);
            const float mf = (float)(2.01 * ((double)d + (double)dp / 32.0 + 6.0) * 5.9604644775390625e-08 * 1.01);
            rec[0] = resolve(l);
            rec[1] = resolve(r);
            memcpy(&rec[2], &mf, 4);
            rec[3] = 0;
            continue;
        }
        if (cosine) {
            // per child: c / nb with nb the REFERENCE's f32 norm of the centroid (cnorm, as the exact walk uses it; f64
            // quotient rounded once), so the screen and the reference divide by the same number.  The slot's margin
            // M = 2.0002 e_p + a_l + a_r + u  (DESIGN.md 4.4 "cosine descent"): e_p = (D/32 + 6.1) u for the screen's
            // summation tree, a = (2.02 + 1.0003 |w o c| / nb) u for the reference's sequential dot product, w_i the
            // number of roundings term i goes through.  A child whose norm the EPSILON rule or an overflowing squared
            // norm could touch, or that is not finite, makes the slot exact-only (NaN margin).
            bool usable = true;
            double a_sum = 0.0;
            for (uint32_t side = 0; side < 2; ++side) {
                const int32_t ch = side == 0 ? l : r;
                const float *c = centroids + (size_t)ch * d;
                const double nb = (double)cn32[ch];
                double c2 = 0.0, wc2 = 0.0;
                for (uint32_t q = 0; q < d; ++q) {
                    const double wq = (q == 0) ? (double)d : (double)(d - q + 1);  // additions behind term q, plus its product
                    c2 += (double)c[q] * (double)c[q];
                    wc2 += wq * wq * (double)c[q] * (double)c[q];
                }
                const double cn = std::sqrt(c2);
                if (!(cn >= 1e-9 && cn <= 1e18) || !(nb >= 1e-9 && nb <= 1e18)) {
                    usable = false;
                    continue;
                }
                for (uint32_t q = 0; q < d; ++q) w[((size_t)sl * 2 + side) * dp + q] = (float)((double)c[q] / nb);
                a_sum += 2.02 + 1.0003 * std::sqrt(wc2) / nb;
            }
            const double e_p = (double)dp / 32.0 + 6.1;
            const double margin = (2.0002 * e_p + a_sum + 1.0) * 5.9604644775390625e-08 * 1.01;  // 1 %: the threshold's own f32 arithmetic
            const float mf = usable ? (float)margin : std::numeric_limits<float>::quiet_NaN();
            rec[0] = resolve(l);
            rec[1] = resolve(r);
            memcpy(&rec[2], &mf, 4);
            rec[3] = 0;
            continue;
        }
        double w2 = 0.0;
        for (uint32_t q = 0; q < d; ++q) {
            const float wv = centroids[(size_t)l * d + q] - centroids[(size_t)r * d + q];
            w[(size_t)sl * dp + q] = wv;
            w2 += (double)wv * (double)wv;
        }
        const float b = (float)(a2[l] - a2[r]);
        const float wn = (float)(std::sqrt(w2) * 1.000001);
        if (!(w2 <= 1e300)) finite = false;
        rec[0] = resolve(l);
        rec[1] = resolve(r);
        memcpy(&rec[2], &b, 4);
        memcpy(&rec[3], &wn, 4);
    }
    const int32_t start = resolve(0);
    if (start < 0) return VQHIP_OK;  // the root leads to one leaf without any decision: exact walk
    t->scr.start_slot = start;
    VQ_TRY(t->scr_slot_node.alloc((size_t)n_int * 4));
    VQ_HIP(hipMemcpyAsync(t->scr_slot_node.p, slot_node.data(), (size_t)n_int * 4, hipMemcpyHostToDevice, s));
    t->scr.slot_node = t->scr_slot_node.as<int32_t>();
    VQ_TRY(t->scr_node_slot.alloc((size_t)n_nodes * 4));
    VQ_HIP(hipMemcpyAsync(t->scr_node_slot.p, slot_of.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s));
    t->scr.node_slot = t->scr_node_slot.as<int32_t>();
    VQ_TRY(t->scr_w.alloc(w.size() * 4));
    VQ_TRY(t->scr_info.alloc(info.size() * 4));
    VQ_TRY(t->scr_mu.alloc((size_t)dp * 4));
    VQ_HIP(hipMemsetAsync(t->scr_mu.p, 0, (size_t)dp * 4, s));
    VQ_TRY(t->scr_count.alloc(8));  // two counters used in turn (TsvqScreen::turn)
    VQ_HIP(hipMemsetAsync(t->scr_count.p, 0, 8, s));
    VQ_HIP(hipMemcpyAsync(t->scr_w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipMemcpyAsync(t->scr_info.p, info.data(), info.size() * 4, hipMemcpyHostToDevice, s));
    if (!cosine && !manhattan) VQ_HIP(hipMemcpyAsync(t->scr_mu.p, mu, (size_t)d * 4, hipMemcpyHostToDevice, s));  // else y = x
    VQ_HIP(hipStreamSynchronize(s));  // w / info are stack-owned
    t->scr.w = t->scr_w.as<float>();
    t->scr.info = t->scr_info.as<int4>();
    t->scr.mu = t->scr_mu.as<float>();
    t->scr.wl_count = t->scr_count.as<uint32_t>();
    t->scr.n_int = n_lds;  // slots resident in LDS; w / info / slot_node hold all of the tree's slots
    t->scr.n_slots = n_int;
    t->scr.n_nodes = n_nodes;
    // a non-finite tree sends every row to the exact continuation (T = NaN never passes)
    t->scr.R = finite ? (float)(std::sqrt(r2max) * 1.000001) : std::numeric_limits<float>::quiet_NaN();
    // T = u * base * (coef_a * base + coef_b * |w|), base >= |x - mu| + R
    t->scr.coef_a = 1.1f * (2.0f * d + 20.0f);
    t->scr.coef_b = 1.1f * (2.0f * d + 16.0f);
    if (cosine || manhattan) {
        // DESIGN.md 4.4 "cosine descent" / "Manhattan descent": the margin travels in the slot's record
        t->scr.R = 0.0f;
        t->scr.coef_a = 0.0f;
        t->scr.coef_b = 0.0f;
    }
    t->use_screen = true;
    return VQHIP_OK;
}

#define VQ_API_BEGIN try {
#define VQ_API_END                                                                  \
    }                                                                               \
    catch (const std::bad_alloc &) { return fail(VQHIP_ERR_FAILURE, "host allocation failed"); } \
    catch (...) { return fail(VQHIP_ERR_FAILURE, "unexpected C++ exception"); }

extern "C" {

// ------------------------------------------------------------------ library/device ----
const char *vqhip_backend(void) { return "libvqhip 0.1 (HIP, gfx950 / MI355X: bf16-split MFMA screen + exact VALU re-check)"; }

const char *vqhip_last_error(void) { return tls().last_error.c_str(); }

int vqhip_device_count(void) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    int good = 0;
    for (int i = 0; i < ndev; ++i) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            ++good;
    }
    return good;
}

int vqhip_set_device(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(VQHIP_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(VQHIP_ERR_INVALID_INPUT, "device %d out of range [0,%d)", device, ndev);
    VQ_HIP(hipSetDevice(device));
    return require_gfx950();
}

int vqhip_get_device(int *device) {
    if (!device) return fail(VQHIP_ERR_NULL_PTR, "device is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VQHIP_ERR_NO_DEVICE, "no HIP device available");
    VQ_HIP(hipGetDevice(device));
    return VQHIP_OK;
}

int vqhip_set_stream(void *hip_stream) {
    ThreadState &st = tls();
    st.user_stream = reinterpret_cast<hipStream_t>(hip_stream);
    st.user_stream_set = (hip_stream != nullptr);
    return VQHIP_OK;
}

int vqhip_selftest(float *bf16_32x32x16_ratio, float *bf16_16x16x32_ratio, int *bf16_engine_trusted) {
    VQ_API_BEGIN
    VQ_TRY(require_gfx950());
    return bf16_mfma_selftest(bf16_32x32x16_ratio, bf16_16x16x32_ratio, bf16_engine_trusted);
    VQ_API_END
}

int vqhip_mfma_bf16_probe(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d) {
    VQ_API_BEGIN
    if (trials && (!a || !b || !c || !d)) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    return mfma_bf16_probe(a, b, c, trials, d);
    VQ_API_END
}

int vqhip_mfma_bf16_model(const uint16_t *a, const uint16_t *b, const float *c, uint64_t trials, float *d) {
    VQ_API_BEGIN
    if (trials && (!a || !b || !c || !d)) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    mfma_bf16_model_host(a, b, c, trials, d);  // pure integer model of one instruction: needs no device
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_mfma_bf16_model_check(uint64_t trials, uint64_t seed, uint64_t *mismatches, uint64_t *first_bad_trial) {
    VQ_API_BEGIN
    VQ_TRY(require_gfx950());
    return mfma_bf16_model_check(trials, seed, mismatches, first_bad_trial, nullptr, 0);
    VQ_API_END
}

int vqhip_mfma_bf16_model_failures(uint64_t trials, uint64_t seed, uint64_t *trial_ids, uint32_t cap, uint64_t *n_failures) {
    VQ_API_BEGIN
    if (!trial_ids || !n_failures) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    return mfma_bf16_model_check(trials, seed, n_failures, nullptr, trial_ids, cap);
    VQ_API_END
}

int vqhip_mfma_bf16_model_case(uint64_t seed, uint64_t trial, uint16_t *a, uint16_t *b, float *c) {
    if (!a || !b || !c) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    mfma_bf16_model_case(seed, trial, a, b, c);
    return VQHIP_OK;
}

int vqhip_synchronize(void) {
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
}

int vqhip_last_assign_stats(uint64_t *rechecked, int *engine) {
    VQ_API_BEGIN
    ThreadState &st = tls();
    if (engine) *engine = st.last_engine;
    if (rechecked) {
        *rechecked = 0;
        if (!g_last_ws) return VQHIP_OK;
        // the workspace is pinned for the query: its handle's destructor unregisters first and waits for the pin
        WsPin pin(g_last_ws);
        if (!pin.ws) return VQHIP_OK;  // the handle is gone
        AssignWorkspace *ws = pin.ws;
        Entry in(*pin.sync);
        if (ws->stats_pending) {
            // the copy is ordered behind the pass whatever stream that ran on (Entry::stream waits for the handle's
            // tail); a handle that several threads use reports its most recent pass, whoever queued it
            hipStream_t s;
            VQ_TRY(in.stream(&s));
            uint64_t tot = 0;
            if (ws->last_segmented) {
                if (ws->last_n_seg > 0) {
                    VQ_HIP(hipMemcpyAsync(ws->seg_host, ws->wl_seg.p, (size_t)ws->stats_m * ws->last_n_seg * 8, hipMemcpyDeviceToHost, s));
                    VQ_HIP(hipStreamSynchronize(s));
                    for (size_t i = 0; i < (size_t)ws->stats_m * ws->last_n_seg; ++i) tot += ws->seg_host[2 * i + 1];
                }
            } else {
                VQ_HIP(hipMemcpyAsync(ws->stats_host, ws->wl_count.p, (size_t)ws->stats_m * 4, hipMemcpyDeviceToHost, s));
                VQ_HIP(hipStreamSynchronize(s));
                for (uint32_t i = 0; i < ws->stats_m; ++i) tot += ws->stats_host[i];
            }
            in.synced();
            *rechecked = tot;
        }
    }
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_last_screen_products(int *products) {
    if (!products) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    const ThreadState &st = tls();
    *products = (st.last_engine == VQHIP_ENGINE_MFMA_BF16) ? st.last_products : 0;
    return VQHIP_OK;
}

int vqhip_xfer_lane_calls(uint64_t *calls) {
    if (!calls) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *calls = g_xfer_lane_calls.load();
    return VQHIP_OK;
}

int vqhip_set_profiling(int on) {
    g_prof.on = on != 0;
    return VQHIP_OK;
}

int vqhip_profile_collect(uint32_t *n_calls, double *primary_ms, double *recheck_ms) {
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    VQ_HIP(hipStreamSynchronize(s));
    double a = 0.0, b = 0.0;
    const size_t calls = g_prof.ev.size() / 3;
    for (size_t i = 0; i < calls; ++i) {
        float t01 = 0.f, t12 = 0.f;
        VQ_HIP(hipEventElapsedTime(&t01, g_prof.ev[3 * i], g_prof.ev[3 * i + 1]));
        VQ_HIP(hipEventElapsedTime(&t12, g_prof.ev[3 * i + 1], g_prof.ev[3 * i + 2]));
        a += t01;
        b += t12;
    }
    for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
    g_prof.ev.clear();
    g_prof.engines.clear();
    if (n_calls) *n_calls = (uint32_t)calls;
    if (primary_ms) *primary_ms = a;
    if (recheck_ms) *recheck_ms = b;
    return VQHIP_OK;
}

int vqhip_memcpy_device(void *dst, const void *src, uint64_t bytes) {
    if (bytes == 0) return VQHIP_OK;
    if (!dst || !src) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    VQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    return VQHIP_OK;
}

// ------------------------------------------------------------------------ datasets ----
int vqhip_dataset_from_host(const float *rows, uint64_t n, uint32_t d, vqhip_dataset **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (n == 0 || d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "empty dataset (n=%llu, d=%u)", (unsigned long long)n, d);
    if (!rows) return fail(VQHIP_ERR_NULL_PTR, "rows is NULL");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    vqhip_dataset *ds = new vqhip_dataset();
    int rc = ds->own.alloc((size_t)n * d * 4);
    if (rc != VQHIP_OK) {
        delete ds;
        return rc;
    }
    // ONE copy straight from the caller's pages: 54.7 GB/s here (tools/host_xfer.py), 0.96 of what pinned memory gives;
    // staging through pinned buffers on several host threads was measured slower (45.9 GB/s: the host memcpys)
    hipError_t e = hipMemcpyAsync(ds->own.p, rows, (size_t)n * d * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        delete ds;
        return fail(VQHIP_ERR_RUNTIME, "H2D copy of the dataset failed: %s", hipGetErrorString(e));
    }
    ds->X = ds->own.as<float>();
    ds->n = n;
    ds->d = d;
    *out = ds;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_dataset_from_device(const void *dev_rows, uint64_t n, uint32_t d, vqhip_dataset **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (n == 0 || d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "empty dataset");
    if (!dev_rows) return fail(VQHIP_ERR_NULL_PTR, "dev_rows is NULL");
    if ((reinterpret_cast<uintptr_t>(dev_rows) & 15) != 0)
        return fail(VQHIP_ERR_INVALID_INPUT, "device row buffer must be 16-byte aligned");
    VQ_TRY(require_gfx950());
    vqhip_dataset *ds = new vqhip_dataset();
    ds->X = reinterpret_cast<const float *>(dev_rows);
    ds->n = n;
    ds->d = d;
    *out = ds;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_dataset_synthetic(uint64_t n, uint32_t d, uint64_t seed, uint64_t row_offset, vqhip_dataset **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (n == 0 || d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "empty dataset");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    vqhip_dataset *ds = new vqhip_dataset();
    int rc = ds->own.alloc((size_t)n * d * 4);
    if (rc == VQHIP_OK) rc = launch_synth_uniform(ds->own.as<float>(), n, d, seed, row_offset, s);
    // a data set is immutable and shared freely between threads / streams: it is complete when the handle exists
    if (rc == VQHIP_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(VQHIP_ERR_RUNTIME, "generating the synthetic rows failed");
    if (rc != VQHIP_OK) {
        delete ds;
        return rc;
    }
    ds->X = ds->own.as<float>();
    ds->n = n;
    ds->d = d;
    *out = ds;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_dataset_info(const vqhip_dataset *ds, uint64_t *n, uint32_t *d, const void **dev_rows) {
    if (!ds) return fail(VQHIP_ERR_NULL_PTR, "dataset is NULL");
    if (n) *n = ds->n;
    if (d) *d = ds->d;
    if (dev_rows) *dev_rows = ds->X;
    return VQHIP_OK;
}

int vqhip_dataset_read(const vqhip_dataset *ds, uint64_t row0, uint64_t nrows, float *out) {
    if (!ds || !out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (row0 > ds->n || nrows > ds->n - row0) return fail(VQHIP_ERR_INVALID_INPUT, "row range out of bounds");
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    VQ_HIP(hipMemcpyAsync(out, ds->X + row0 * ds->d, (size_t)nrows * ds->d * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
}

int vqhip_dataset_destroy(vqhip_dataset *ds) {
    delete ds;
    return VQHIP_OK;
}

int vqhip_synth_uniform_host(float *out, uint64_t n, uint32_t d, uint64_t seed, uint64_t row_offset) {
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    synth_uniform_host(out, n, d, seed, row_offset);
    return VQHIP_OK;
}

// ------------------------------------------------------------------------- k-means ----
int vqhip_kmeans_create(const vqhip_dataset *ds, uint32_t m, uint32_t k, vqhip_kmeans **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!ds) return fail(VQHIP_ERR_NULL_PTR, "dataset is NULL");
    if (m == 0 || ds->d < m || ds->d % m != 0)
        return fail(VQHIP_ERR_INVALID_INPUT, "dimension (%u) must be divisible by m (%u)", ds->d, m);
    if (k == 0) return fail(VQHIP_ERR_INVALID_INPUT, "k must be greater than 0");
    if (k > kMaxCentroids) return fail(VQHIP_ERR_UNSUPPORTED, "k=%u > 65536: codes are at most two bytes per subspace", k);
    VQ_TRY(require_gfx950());
    const uint32_t sd = ds->d / m;
    std::unique_ptr<vqhip_kmeans> km(new vqhip_kmeans());
    km->ds = ds;
    VQ_TRY(km->cs.init(m, k, sd));
    // sub_dim > 1024 (lbg_quantize on long whole vectors): no LDS accumulator layout; the bucket-and-chain sums of
    // the reference-order update serve any length
    km->sums_by_chains = sd > 1024;
    if (!km->sums_by_chains) VQ_TRY(plan_update(m, k, sd, ds->n, &km->plan));
    VQ_TRY(km->codes.alloc((size_t)ds->n * m * code_bytes(k)));
    if (!km->sums_by_chains) {
        size_t sums_b = km->plan.partial_floats * km->plan.n_row_chunks * 4, cnt_b = km->plan.partial_counts * km->plan.n_row_chunks * 4;
        if (km->cs.x32_ok && screen_bf16_fused_update_supported(sd, k)) {
            // fused update: one slab per (screen wave chunk or patch chunk, active subspace); <= 8 waves per CU
            km->fused_slabs = (uint32_t)num_cus() * 8 + 16 * m;
            sums_b = std::max(sums_b, (size_t)km->fused_slabs * k * sd * 4);
            cnt_b = std::max(cnt_b, (size_t)km->fused_slabs * k * 4);
        }
        VQ_TRY(km->partial_sums.alloc(sums_b));
        VQ_TRY(km->partial_counts.alloc(cnt_b));
        // the LDS-atomic accumulate adds in whatever order its atomics land: where no wave-owned kernel serves the shape,
        // the reference-order chains give the same bits every run (k beyond their limit keeps the atomic kernel)
        km->chain_update = !accumulate_owned(km->plan, ds->X, ds->d) && exact_sums_supported(k);
    }
    VQ_TRY(km->slab.alloc((size_t)m * k * (sd + 1) * 8));
    VQ_TRY(km->counts.alloc((size_t)m * k * 4));
    VQ_TRY(km->changed.alloc((size_t)m * 4));
    VQ_TRY(km->active_dev.alloc(m));
    VQ_TRY(km->rows_tmp.alloc((size_t)m * k * 8));
    VQ_TRY(km->agree.alloc(16));
    VQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&km->counts_host), (size_t)m * k * 4));
    VQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&km->changed_host), (size_t)m * 4));
    VQ_HIP(hipHostMalloc(reinterpret_cast<void **>(&km->run_host), (size_t)(m + 1 + 6 * m) * 4 + ((size_t)m + 3) / 4 * 4));
    km->active.assign(m, 1);
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    VQ_HIP(hipMemsetAsync(km->active_dev.p, 1, m, s));
    VQ_HIP(hipMemsetAsync(km->cs.cb.p, 0, km->cs.cb.bytes, s));
    VQ_HIP(hipMemsetAsync(km->slab.p, 0, km->slab.bytes, s));
    VQ_HIP(hipStreamSynchronize(s));
    *out = km.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_kmeans_destroy(vqhip_kmeans *km) {
    delete km;  // (unregisters its workspace: a later vqhip_last_assign_stats of any thread finds it gone)
    return VQHIP_OK;
}

int vqhip_kmeans_set_centroids(vqhip_kmeans *km, const float *centroids) {
    if (!km || !centroids) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_HIP(hipMemcpyAsync(km->cs.cb.p, centroids, (size_t)km->cs.m * km->cs.k * km->cs.sd * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    km->cs.prepared = false;
    return VQHIP_OK;
}

int vqhip_kmeans_init_from_rows(vqhip_kmeans *km, const uint64_t *init_rows) {
    if (!km || !init_rows) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    const size_t cnt = (size_t)km->cs.m * km->cs.k;
    for (size_t i = 0; i < cnt; ++i)
        if (init_rows[i] >= km->ds->n)
            return fail(VQHIP_ERR_INVALID_INPUT, "init row %llu out of range", (unsigned long long)init_rows[i]);
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_HIP(hipMemcpyAsync(km->rows_tmp.p, init_rows, cnt * 8, hipMemcpyHostToDevice, s));
    VQ_TRY(launch_gather_rows(km->ds->X, km->ds->d, km->cs.m, km->cs.k, km->cs.sd, km->rows_tmp.as<uint64_t>(),
                              km->cs.cb.as<float>(), s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    km->cs.prepared = false;
    return VQHIP_OK;
}

int vqhip_kmeans_get_centroids(vqhip_kmeans *km, float *centroids) {
    if (!km || !centroids) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_HIP(hipMemcpyAsync(centroids, km->cs.cb.p, (size_t)km->cs.m * km->cs.k * km->cs.sd * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
}

int vqhip_kmeans_set_active(vqhip_kmeans *km, const uint8_t *active) {
    if (!km || !active) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    bool all = true;
    for (uint32_t s = 0; s < km->cs.m; ++s) {
        km->active[s] = active[s] ? 1 : 0;
        all = all && km->active[s];
    }
    km->all_active = all;
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_HIP(hipMemcpyAsync(km->active_dev.p, km->active.data(), km->cs.m, hipMemcpyHostToDevice, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
}

int vqhip_kmeans_get_active(const vqhip_kmeans *km, uint8_t *active) {
    if (!km || !active) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lk(const_cast<vqhip_kmeans *>(km)->sync.mu);
    for (uint32_t s = 0; s < km->cs.m; ++s) active[s] = km->active[s] ? 1 : 0;
    return VQHIP_OK;
}

int vqhip_kmeans_set_engine(vqhip_kmeans *km, int engine) {
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (engine < VQHIP_ENGINE_AUTO || engine > VQHIP_ENGINE_MFMA_BF16) return fail(VQHIP_ERR_INVALID_INPUT, "unknown engine %d", engine);
    std::lock_guard<std::recursive_mutex> lk(km->sync.mu);
    km->engine = engine;
    return VQHIP_OK;
}

uint32_t vqhip_code_bytes(uint32_t k) { return code_bytes(k); }

int vqhip_kmeans_set_exact_update(vqhip_kmeans *km, int exact_update) {
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lk(km->sync.mu);
    km->exact_update = exact_update ? 1 : 0;
    return VQHIP_OK;
}

// A small problem's iteration is TWO launches (k_lloyd_small.hip) wherever the whole loop body runs on this device: the
// single-GPU vqhip_kmeans_step / vqhip_kmeans_run; the split accumulate / all-reduce / finalize forms run the same
// kernels up to the f64 slab and k_finalize behind it, with the same bits.  Against the general path (VQHIP_SMALL_LLOYD=0)
// codes, counts and flags are equal bit for bit; the means differ in the last bits (other row ranges behind the f64
// combination), both inside the tolerance DESIGN.md 2 states.
static bool kmeans_small_eligible(const vqhip_kmeans *km) {
    static const char *env = getenv("VQHIP_SMALL_LLOYD");  // =0: never (A/B)
    if (env && env[0] == '0') return false;
    return km->engine == VQHIP_ENGINE_AUTO && !km->exact_update && !km->sums_by_chains && !g_prof.on &&
           lloyd_small_supported(km->ds->n, km->cs.m, km->cs.k, km->cs.sd);
}
static int kmeans_small_workspace(vqhip_kmeans *km, hipStream_t s) {
    const uint32_t m = km->cs.m, k = km->cs.k, sd = km->cs.sd;
    if (!km->sm_tick.p) {
        size_t cnt_b = 0, tick_b = 0;
        const size_t sum_b = lloyd_small_workspace(km->ds->n, m, k, sd, &cnt_b, &tick_b);
        VQ_TRY(km->sm_psum.alloc(sum_b));
        VQ_TRY(km->sm_pcnt.alloc(cnt_b));
        VQ_TRY(km->sm_tick.alloc(tick_b));
        VQ_HIP(hipMemsetAsync(km->sm_tick.p, 0, tick_b, s));
    }
    return VQHIP_OK;
}
static void kmeans_small_note(vqhip_kmeans *km) {  // host-side state behind a small-path launch
    km->ws.stats_pending = false;
    km->ws.last_engine = VQHIP_ENGINE_EXACT;
    ThreadState &st = tls();
    st.last_engine = VQHIP_ENGINE_EXACT;
    st.last_rechecked = 0;
    g_last_ws = km->ws_id;
}
// run: iteration `it` of a device-driven run (its flags behind sm_tick, the iterations executed in run_state[1 .. m])
static int kmeans_small_enqueue(vqhip_kmeans *km, hipStream_t s, bool run, uint32_t it = 0) {
    const uint32_t m = km->cs.m, k = km->cs.k, sd = km->cs.sd;
    VQ_TRY(kmeans_small_workspace(km, s));
    const uint8_t *act = run ? km->active_dev.as<uint8_t>() : (km->all_active ? nullptr : km->active_dev.as<uint8_t>());
    VQ_TRY(launch_lloyd_small(km->ds->X, km->ds->n, km->ds->d, m, k, sd, km->cs.cb.as<float>(), km->codes.as<uint8_t>(),
                              km->sm_psum.as<float>(), km->sm_pcnt.as<uint32_t>(), km->counts.as<uint32_t>(), km->changed.as<uint32_t>(),
                              act, run ? km->sm_tick.as<uint32_t>() : nullptr, run ? km->run_state.as<uint32_t>() + 1 : nullptr, it, s));
    km->cs.prepared = false;
    km->accumulated = false;
    kmeans_small_note(km);
    return VQHIP_OK;
}

// queue assign + update of one Lloyd iteration on `s` (no host synchronisation: capturable); gated: inside a
// device-driven run (vqhip_kmeans_run) every kernel that changes state checks the run's device flags
static int kmeans_accumulate_enqueue(vqhip_kmeans *km, hipStream_t s, bool gated = false, bool fuse_finalize = false) {
    std::vector<uint32_t> subs;
    for (uint32_t i = 0; i < km->cs.m; ++i)
        if (km->active[i]) subs.push_back(i);
    const vqhip_dataset *ds = km->ds;
    g_last_ws = km->ws_id;
    if (kmeans_small_eligible(km)) {  // small problem: assignment + this rank's f64 slab in one launch (k_lloyd_small.hip)
        VQ_TRY(kmeans_small_workspace(km, s));
        const uint8_t *act = gated ? km->active_dev.as<uint8_t>() : (km->all_active ? nullptr : km->active_dev.as<uint8_t>());
        VQ_TRY(launch_lloyd_small_slab(ds->X, ds->n, ds->d, km->cs.m, km->cs.k, km->cs.sd, km->cs.cb.as<float>(), km->codes.as<uint8_t>(),
                                       km->sm_psum.as<float>(), km->sm_pcnt.as<uint32_t>(), act,
                                       gated ? km->run_state.as<uint32_t>() : nullptr, km->changed.as<uint32_t>(), km->slab.as<double>(), s));
        kmeans_small_note(km);
        km->accumulated = true;
        return VQHIP_OK;
    }
    // assignment: always squared L2 (src/core/vector.rs:352-363); with the update fused in where the shape allows
    FusedAcc fused;
    if (km->fused_slabs && !km->exact_update && !km->sums_by_chains) {
        fused.sums = km->partial_sums.as<float>();
        fused.counts = km->partial_counts.as<uint32_t>();
        fused.slab_cap = km->fused_slabs;
        if (gated) {
            fused.gate_active = km->active_dev.as<uint8_t>();
            fused.gate_halt = km->run_state.as<uint32_t>();
        }
    }
    VQ_TRY(run_assign(km->cs, km->ws, ds->X, ds->n, ds->d, VQHIP_SQUARED_EUCLIDEAN, subs,
                      km->codes.as<uint8_t>(), km->engine, s, &fused));
    if (gated && !fused.used) return fail(VQHIP_ERR_FAILURE, "device-driven run without the fused update");
    const uint8_t *act = km->all_active ? nullptr : km->active_dev.as<uint8_t>();
    if (fused.used && gated && fuse_finalize) {
        // one rank, device-driven: sums and means in one launch, the iteration's decisions behind it (k_reduce_finalize_run)
        uint32_t *rs = km->run_state.as<uint32_t>();  // [0] halt, [1..m] iterations, [m+1] unused, [m+2] empty-cluster flag, [m+3..] `changed` scratch [m]
        const uint32_t m = km->cs.m;
        VQ_TRY(launch_reduce_finalize_run(m, km->cs.k, km->cs.sd, km->partial_sums.as<float>(), km->partial_counts.as<uint32_t>(),
                                          fused.chunks, (uint32_t)subs.size(), km->ws.sub_pos.as<int32_t>(), km->slab.as<double>(),
                                          km->active_dev.as<uint8_t>(), km->cs.cb.as<float>(), km->counts.as<uint32_t>(),
                                          km->changed.as<uint32_t>(), rs, rs + 1, rs + 1 + m, rs + 3 + m, s));
    } else if (fused.used) {
        VQ_TRY(launch_reduce_partials_pos(km->cs.m, km->cs.k, km->cs.sd, km->partial_sums.as<float>(),
                                          km->partial_counts.as<uint32_t>(), fused.chunks, (uint32_t)subs.size(),
                                          km->ws.sub_pos.as<int32_t>(), km->slab.as<double>(), s, fused.gate_active,
                                          fused.gate_halt, gated ? km->changed.as<uint32_t>() : nullptr));
    } else if (km->exact_update || km->sums_by_chains || km->chain_update) {
        size_t need = exact_sums_workspace_bytes(km->cs.m, km->cs.k, ds->n);
        VQ_TRY(km->xs_ws.ensure(need));
        VQ_TRY(launch_exact_sums(km->cs.m, km->cs.k, km->cs.sd, ds->X, ds->n, ds->d, km->codes.as<uint8_t>(), act,
                                 km->xs_ws.p, km->xs_ws.bytes, km->slab.as<double>(), s));
    } else {
        VQ_TRY(launch_accumulate(km->plan, ds->X, ds->n, ds->d, km->codes.as<uint8_t>(), act,
                                 km->partial_sums.as<float>(), km->partial_counts.as<uint32_t>(), s));
        VQ_TRY(launch_reduce_partials(km->plan, km->partial_sums.as<float>(), km->partial_counts.as<uint32_t>(), act,
                                      km->slab.as<double>(), s));
    }
    km->accumulated = true;
    return VQHIP_OK;
}

int vqhip_kmeans_accumulate(vqhip_kmeans *km) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    return kmeans_accumulate_enqueue(km, s);
    VQ_API_END
}

int vqhip_kmeans_partials(vqhip_kmeans *km, void **dev_slab, uint64_t *n_doubles) {
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lk(km->sync.mu);
    if (dev_slab) *dev_slab = km->slab.p;
    if (n_doubles) *n_doubles = (uint64_t)km->cs.m * km->cs.k * (km->cs.sd + 1);
    return VQHIP_OK;
}

// queue mean / convergence test + the read-back of counts and flags (capturable); gated (device-driven run): the same
// kernel also ends the iteration (retire converged subspaces, count it, halt on an empty cluster)
static int kmeans_finalize_enqueue(vqhip_kmeans *km, hipStream_t s, bool gated = false, bool read_back = true, bool done_already = false) {
    const uint32_t m = km->cs.m, k = km->cs.k;
    if (done_already) {
        // (k_reduce_finalize_run has formed the means behind the sums)
    } else if (gated) {
        uint32_t *rs = km->run_state.as<uint32_t>();  // [0] halt, [1..m] iterations, [m+1] finished-workgroup counter, [m+2] empty-cluster flag of the iteration
        VQ_TRY(launch_finalize_run(m, k, km->cs.sd, km->slab.as<double>(), km->active_dev.as<uint8_t>(), km->cs.cb.as<float>(),
                                   km->counts.as<uint32_t>(), km->changed.as<uint32_t>(), rs, rs + 1, rs + 1 + m, s));
    } else {
        const uint8_t *act = km->all_active ? nullptr : km->active_dev.as<uint8_t>();
        VQ_TRY(launch_finalize(m, k, km->cs.sd, km->slab.as<double>(), act, km->cs.cb.as<float>(),
                               km->counts.as<uint32_t>(), km->changed.as<uint32_t>(), km->exact_update, s));
    }
    km->cs.prepared = false;
    km->accumulated = false;
    if (read_back) {
        VQ_HIP(hipMemcpyAsync(km->counts_host, km->counts.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipMemcpyAsync(km->changed_host, km->changed.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    }
    return VQHIP_OK;
}
static void kmeans_finalize_collect(vqhip_kmeans *km, uint32_t *counts, uint8_t *changed) {
    const uint32_t m = km->cs.m, k = km->cs.k;
    if (counts) memcpy(counts, km->counts_host, (size_t)m * k * 4);
    if (changed)
        for (uint32_t i = 0; i < m; ++i) changed[i] = (km->active[i] && km->changed_host[i]) ? 1 : 0;
}

int vqhip_kmeans_finalize(vqhip_kmeans *km, uint32_t *counts, uint8_t *changed) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    if (!km->accumulated) return fail(VQHIP_ERR_INVALID_INPUT, "finalize without a preceding accumulate");
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_TRY(kmeans_finalize_enqueue(km, s));
    VQ_TRY(spin_wait(s));  // a parked thread wakes ~100 us late; an iteration is 0.1-10 ms
    in.synced();
    kmeans_finalize_collect(km, counts, changed);
    return VQHIP_OK;
    VQ_API_END
}

// Small data sets are launch-bound (C1, 10k x 64: ~60 us of kernels behind ~14 stream operations),
// so the whole step is captured once per (active set, engine) and replayed as a hipGraph; the first
// step with a given key runs eagerly (allocations, code objects, sub-list upload), the second is
// captured, later ones are replays.  VQHIP_GRAPH=0 disables, =1 forces it for any size.
static bool kmeans_graph_eligible(const vqhip_kmeans *km) {
    static const char *env = getenv("VQHIP_GRAPH");
    if (env && env[0] == '0') return false;
    if (km->graph_failed || km->exact_update || km->sums_by_chains || km->chain_update || g_prof.on) return false;
    if (env && env[0] == '1') return true;
    return (uint64_t)km->ds->n * km->cs.m <= (4ull << 20);
}

int vqhip_kmeans_step(vqhip_kmeans *km, uint32_t *counts, uint8_t *changed) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    if (kmeans_small_eligible(km)) {
        const uint32_t m = km->cs.m, k = km->cs.k;
        VQ_TRY(kmeans_small_enqueue(km, s, false));
        VQ_HIP(hipMemcpyAsync(km->counts_host, km->counts.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipMemcpyAsync(km->changed_host, km->changed.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        VQ_TRY(spin_wait(s));
        in.synced();
        kmeans_finalize_collect(km, counts, changed);
        return VQHIP_OK;
    }
    if (!kmeans_graph_eligible(km)) {
        VQ_TRY(kmeans_accumulate_enqueue(km, s));
        VQ_TRY(kmeans_finalize_enqueue(km, s));
        VQ_TRY(spin_wait(s));
        in.synced();
        kmeans_finalize_collect(km, counts, changed);
        return VQHIP_OK;
    }
    uint64_t key = 1469598103934665603ull;  // FNV-1a over what shapes the launch sequence
    auto mix = [&](uint64_t v) { key = (key ^ v) * 1099511628211ull; };
    for (uint32_t i = 0; i < km->cs.m; ++i) mix(km->active[i]);
    mix((uint64_t)km->engine + 17);
    mix(reinterpret_cast<uintptr_t>(s));
    if (km->graph_exec && km->graph_key == key) {
        VQ_HIP(hipGraphLaunch(km->graph_exec, s));
        VQ_TRY(spin_wait(s));
    } else if (km->warm_key == key) {
        km->drop_graph();
        km->cs.prepared = false;  // the codebook images must be part of the captured sequence
        hipGraph_t graph = nullptr;
        VQ_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        int rc = kmeans_accumulate_enqueue(km, s);
        if (rc == VQHIP_OK) rc = kmeans_finalize_enqueue(km, s);
        const hipError_t e = hipStreamEndCapture(s, &graph);
        if (rc == VQHIP_OK && e == hipSuccess && graph &&
            hipGraphInstantiate(&km->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            (void)hipGraphDestroy(graph);
            km->graph_key = key;
            VQ_HIP(hipGraphLaunch(km->graph_exec, s));
            VQ_TRY(spin_wait(s));
        } else {  // capture is an optimisation only: fall back to the plain sequence for this handle
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            km->graph_exec = nullptr;
            km->graph_failed = true;
            km->cs.prepared = false;
            VQ_TRY(kmeans_accumulate_enqueue(km, s));
            VQ_TRY(kmeans_finalize_enqueue(km, s));
            VQ_TRY(spin_wait(s));
        }
    } else {
        VQ_TRY(kmeans_accumulate_enqueue(km, s));
        VQ_TRY(kmeans_finalize_enqueue(km, s));
        VQ_TRY(spin_wait(s));
        km->warm_key = key;
    }
    in.synced();  // every branch above ended in spin_wait
    // host-side state the enqueue functions leave behind (a replay does not run them)
    km->cs.prepared = false;
    km->accumulated = false;
    km->ws.stats_pending = (km->ws.last_engine == VQHIP_ENGINE_MFMA || km->ws.last_engine == VQHIP_ENGINE_MFMA_BF16);
    g_last_ws = km->ws_id;
    tls().last_engine = km->ws.last_engine;
    tls().last_products = km->ws.last_products;
    kmeans_finalize_collect(km, counts, changed);
    return VQHIP_OK;
    VQ_API_END
}

// ---- failure containment of the sharded entry points -------------------------------------------------------------------
// A rank that leaves a collective call early (allocation / launch failure on its device only) must not leave its peers
// waiting: every sharded entry point goes out through sharded_exit, which poisons an in-process group (comm.hip:
// comm_abort; the peers' barriers return VQHIP_ERR_RUNTIME at once, and their waits are bounded anyway).  Argument errors
// every rank sees alike (NULL, INVALID_INPUT, UNSUPPORTED) do not poison.
static int sharded_exit(vqhip_comm *comm, int rc) {
    if ((rc == VQHIP_ERR_RUNTIME || rc == VQHIP_ERR_FAILURE || rc == VQHIP_ERR_NO_DEVICE) && comm && comm->c) {
        const char *silent = getenv("VQHIP_TEST_FAIL_SILENT");  // tests: a rank that dies without telling (peers time out)
        if (!(silent && silent[0] == '1')) comm_abort(comm->c, tls().last_error.c_str());
    }
    return rc;
}

// Fault injection for tests/test_gpu_multi.py (compiled in, off unless BOTH variables are set; read per call):
// rank VQHIP_TEST_FAIL_RANK of a sharded run fails in front of iteration VQHIP_TEST_FAIL_ITER with VQHIP_ERR_RUNTIME, as a
// launch failure on that rank's device would.
static int fault_injected(Comm *comm, uint32_t it) {
    const char *fr = getenv("VQHIP_TEST_FAIL_RANK"), *fi = getenv("VQHIP_TEST_FAIL_ITER");
    if (!fr || !fi || !fr[0] || !fi[0]) return VQHIP_OK;
    int world = 1, rank = 0;
    comm_info(comm, &world, &rank);
    if (rank != atoi(fr) || it != (uint32_t)atoi(fi)) return VQHIP_OK;
    return fail(VQHIP_ERR_RUNTIME, "fault injection: rank %d of %d fails in front of iteration %u (VQHIP_TEST_FAIL_RANK / _ITER)", rank, world, it);
}

// Up to max_iters Lloyd iterations (src/core/vector.rs:415-458) with the loop's decisions taken on the device: the
// iterations are queued back to back; a converged subspace stops being processed, an empty cluster in an active
// subspace pauses the run after that iteration (every later queued kernel becomes a no-op) so that the caller can
// draw the reseed rows.  Shapes without the fused update take the same decisions on the host, one step at a time.
static int kmeans_run_impl(vqhip_kmeans *km, Comm *comm, uint32_t max_iters, uint32_t *iters_done, uint32_t *counts,
                           uint8_t *changed, int *paused) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    int world = 1;
    comm_info(comm, &world, nullptr);
    Entry in(km->sync);
    // (arguments every rank passes alike -- the host program's contract -- may end the call before the agreement below;
    // anything that depends on THIS rank's device, environment or memory may not: a rank that left early would leave
    // its peers blocked in the collective)
    if (world > 1 && km->exact_update)
        return fail(VQHIP_ERR_UNSUPPORTED, "exact_update sums rows in one sequential chain: single GPU only");
    const uint32_t m = km->cs.m, k = km->cs.k;
    if (iters_done) memset(iters_done, 0, (size_t)m * 4);
    if (paused) *paused = 0;
    bool any_active = false;
    for (uint32_t i = 0; i < m; ++i) any_active = any_active || km->active[i];
    if (max_iters == 0 || !any_active) {
        if (changed) memset(changed, 0, m);
        return VQHIP_OK;
    }
    hipStream_t s = nullptr;
    int engine = 0;
    int local_rc = require_gfx950();
    if (local_rc == VQHIP_OK) local_rc = in.stream(&s);
    if (local_rc == VQHIP_OK) local_rc = pick_engine(km->engine, km->cs, VQHIP_SQUARED_EUCLIDEAN, &engine);
    uint32_t n_active = 0;
    for (uint32_t i = 0; i < m; ++i) n_active += km->active[i] ? 1u : 0u;
    // the device-driven loop needs the fused update: exactly run_assign's predicate (engine, one centroid group, a slab
    // per (chunk, active subspace) beyond the list-driven ones), evaluated BEFORE anything is queued -- otherwise the
    // host-driven loop below serves the shape
    bool device_loop = local_rc == VQHIP_OK && km->fused_slabs && !km->exact_update && !km->sums_by_chains &&
                       engine == VQHIP_ENGINE_MFMA_BF16 && km->cs.x32_groups == 1 && screen_bf16_fused_update_supported(km->cs.sd, k) &&
                       km->fused_slabs / n_active > FusedAcc().n_patch && km->ds->n != 0 && km->ds->n < (1ull << 32) &&
                       !g_prof.on;
    if (local_rc == VQHIP_OK && kmeans_small_eligible(km)) device_loop = true;
    if (world > 1) {
        // every rank must queue the same number of all-reduces: the decision depends on per-rank state (profiling
        // hooks, the local row count), so the ranks agree on it -- device loop only if ALL of them can -- and
        // in the same collective on whether every rank got this far: {ranks that are ready, ranks that can loop on
        // the device}.  `agree` was allocated with the handle, so a rank short of memory still takes part.
        const std::string my_error = local_rc == VQHIP_OK ? std::string() : tls().last_error;
        if (!s) VQ_TRY(current_stream(&s));  // (no stream at all: nothing can be queued, the peers time out in RCCL)
        const uint32_t mine[2] = {local_rc == VQHIP_OK ? 1u : 0u, device_loop ? 1u : 0u};
        uint32_t all[2] = {0, 0};
        VQ_HIP(hipMemcpyAsync(km->agree.p, mine, 8, hipMemcpyHostToDevice, s));
        VQ_TRY(comm_allreduce_u32(comm, km->agree.as<uint32_t>(), 2, s));
        VQ_HIP(hipMemcpyAsync(all, km->agree.p, 8, hipMemcpyDeviceToHost, s));
        VQ_HIP(hipStreamSynchronize(s));
        if (local_rc != VQHIP_OK) return fail(local_rc, "%s", my_error.c_str());
        if (all[0] != (uint32_t)world)
            return fail(VQHIP_ERR_FAILURE, "%u of %d ranks could not start the run (their own error text says why)",
                        (uint32_t)world - all[0], world);
        device_loop = all[1] == (uint32_t)world;
    }
    VQ_TRY(local_rc);
    // small problems: one launch per iteration on a single GPU (small_loop); row-sharded, the slab form of the same kernel
    // + all-reduce + k_finalize<true>, still without the host
    const bool small_ok = local_rc == VQHIP_OK && kmeans_small_eligible(km);
    const bool small_loop = world == 1 && small_ok;
    if (!device_loop) {
        std::vector<uint32_t> cnt((size_t)m * k);
        std::vector<uint8_t> chg(m);
        for (uint32_t it = 0; it < max_iters; ++it) {
            bool any = false;
            for (uint32_t i = 0; i < m; ++i) any = any || km->active[i];
            if (!any) break;
            VQ_TRY(fault_injected(comm, it));
            if (world > 1) {
                VQ_TRY(kmeans_accumulate_enqueue(km, s));
                VQ_TRY(comm_allreduce_f64(comm, km->slab.as<double>(), (size_t)m * k * (km->cs.sd + 1), s));
                VQ_TRY(kmeans_finalize_enqueue(km, s));
                VQ_TRY(spin_wait(s));
                kmeans_finalize_collect(km, cnt.data(), chg.data());
            } else {
                VQ_TRY(vqhip_kmeans_step(km, cnt.data(), chg.data()));
            }
            bool empty = false;
            for (uint32_t i = 0; i < m; ++i) {
                if (!km->active[i]) continue;
                if (iters_done) iters_done[i] += 1;
                for (uint32_t j = 0; j < k; ++j) empty = empty || cnt[(size_t)i * k + j] == 0;
            }
            if (counts) memcpy(counts, cnt.data(), cnt.size() * 4);
            if (changed) memcpy(changed, chg.data(), m);
            if (empty) {
                if (paused) *paused = 1;
                break;
            }
            std::vector<uint8_t> act(km->active.begin(), km->active.end());
            bool flip = false;
            for (uint32_t i = 0; i < m; ++i)
                if (act[i] && !chg[i]) {
                    act[i] = 0;
                    flip = true;
                }
            if (flip) VQ_TRY(vqhip_kmeans_set_active(km, act.data()));
        }
        in.synced();  // every step ended in a wait
        return VQHIP_OK;
    }
    VQ_TRY(km->run_state.ensure((size_t)(2 * m + 3) * 4));
    VQ_HIP(hipMemsetAsync(km->run_state.p, 0, (size_t)(2 * m + 3) * 4, s));
    // one rank: nothing is exchanged between the sums and the means, so both are one launch
    const bool fuse_finalize = world == 1 && !small_loop;
    if (small_loop) {  // the small form keeps the loop's decisions in two flag sets (k_lloyd_small.hip)
        VQ_TRY(kmeans_small_workspace(km, s));
        VQ_HIP(hipMemsetAsync(km->sm_tick.p, 0, (size_t)6 * m * 4, s));
    }
    for (uint32_t it = 0; it < max_iters; ++it) {
        if (small_loop) {  // two launches per iteration, the loop's decisions read from the previous iteration's flags
            VQ_TRY(kmeans_small_enqueue(km, s, true, it));
            continue;
        }
        VQ_TRY(fault_injected(comm, it));
        VQ_TRY(kmeans_accumulate_enqueue(km, s, true, fuse_finalize));
        // row-sharded: the one exchange of the iteration (a paused run re-sums a slab nobody reads: all ranks pause alike)
        if (!fuse_finalize) VQ_TRY(comm_allreduce_f64(comm, km->slab.as<double>(), (size_t)m * k * (km->cs.sd + 1), s));
        VQ_TRY(kmeans_finalize_enqueue(km, s, true, false, fuse_finalize));  // + the iteration's decisions (k_finalize<true> + k_run_decide)
    }
    // everything the host reads goes to pinned memory, queued back to back, ONE wait
    uint32_t *const st = km->run_host, *const sm_flags = st + (m + 1);
    uint8_t *const act = reinterpret_cast<uint8_t *>(sm_flags + (size_t)6 * m);
    VQ_HIP(hipMemcpyAsync(km->counts_host, km->counts.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipMemcpyAsync(km->changed_host, km->changed.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipMemcpyAsync(st, km->run_state.p, (size_t)(m + 1) * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipMemcpyAsync(act, km->active_dev.p, m, hipMemcpyDeviceToHost, s));
    if (small_loop) VQ_HIP(hipMemcpyAsync(sm_flags, km->sm_tick.p, (size_t)6 * m * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    if (small_loop) {  // the loop's decisions from the flags the last executed iteration left (the kernels never write the set itself)
        bool pause = false;
        std::vector<uint8_t> start(act, act + m);  // active_dev still holds the set the run started from
        lloyd_small_run_result(m, start.data(), sm_flags, st + 1, &pause, act, km->changed_host);
        st[0] = pause ? 1u : 0u;
        // the set as the run left it goes back behind everything queued so far; pinned source, nothing else writes it before
        // the next run's own read-back has been waited for: no wait here (the handle's stream tail stays set)
        VQ_HIP(hipMemcpyAsync(km->active_dev.p, act, m, hipMemcpyHostToDevice, s));
    } else {
        in.synced();
    }
    kmeans_finalize_collect(km, counts, changed);  // flags of the last executed iteration, for the subspaces active in it
    if (iters_done) memcpy(iters_done, st + 1, (size_t)m * 4);
    if (paused) *paused = st[0] ? 1 : 0;
    bool all = true;
    for (uint32_t i = 0; i < m; ++i) {
        km->active[i] = act[i] ? 1 : 0;  // converged subspaces retired on the device (none on a pause: the caller decides)
        all = all && km->active[i];
    }
    km->all_active = all;
    km->ws.stats_pending = !small_loop;
    g_last_ws = km->ws_id;
    tls().last_engine = km->ws.last_engine;
    tls().last_products = km->ws.last_products;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_kmeans_run(vqhip_kmeans *km, uint32_t max_iters, uint32_t *iters_done, uint32_t *counts, uint8_t *changed,
                     int *paused) {
    return kmeans_run_impl(km, nullptr, max_iters, iters_done, counts, changed, paused);
}

int vqhip_kmeans_run_sharded(vqhip_kmeans *km, vqhip_comm *comm, uint32_t max_iters, uint32_t *iters_done, uint32_t *counts,
                             uint8_t *changed, int *paused) {
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    std::lock_guard<std::recursive_mutex> lk_km(km->sync.mu);  // lock order: k-means handle, then communicator
    std::unique_lock<std::recursive_mutex> lk_comm;
    if (comm) lk_comm = std::unique_lock<std::recursive_mutex>(comm->mu);
    return sharded_exit(comm, kmeans_run_impl(km, comm ? comm->c : nullptr, max_iters, iters_done, counts, changed, paused));
}

int vqhip_kmeans_patch_centroid(vqhip_kmeans *km, uint32_t s, uint32_t j, const float *sub_row) {
    if (!km || !sub_row) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (s >= km->cs.m || j >= km->cs.k) return fail(VQHIP_ERR_INVALID_INPUT, "centroid (%u,%u) out of range", s, j);
    Entry in(km->sync);
    hipStream_t st;
    VQ_TRY(in.stream(&st));
    float *dst = km->cs.cb.as<float>() + ((size_t)s * km->cs.k + j) * km->cs.sd;
    VQ_HIP(hipMemcpyAsync(dst, sub_row, (size_t)km->cs.sd * 4, hipMemcpyHostToDevice, st));
    VQ_HIP(hipStreamSynchronize(st));
    in.synced();
    km->cs.prepared = false;
    return VQHIP_OK;
}

int vqhip_kmeans_patch_from_row(vqhip_kmeans *km, uint32_t s, uint32_t j, uint64_t row) {
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (s >= km->cs.m || j >= km->cs.k) return fail(VQHIP_ERR_INVALID_INPUT, "centroid (%u,%u) out of range", s, j);
    if (row >= km->ds->n) return fail(VQHIP_ERR_INVALID_INPUT, "row %llu out of range", (unsigned long long)row);
    Entry in(km->sync);
    hipStream_t st;
    VQ_TRY(in.stream(&st));
    float *dst = km->cs.cb.as<float>() + ((size_t)s * km->cs.k + j) * km->cs.sd;
    const float *src = km->ds->X + row * km->ds->d + (size_t)s * km->cs.sd;
    VQ_HIP(hipMemcpyAsync(dst, src, (size_t)km->cs.sd * 4, hipMemcpyDeviceToDevice, st));
    km->cs.prepared = false;
    return VQHIP_OK;
}

int vqhip_kmeans_get_assignments(vqhip_kmeans *km, uint8_t *codes) {
    if (!km || !codes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_HIP(hipMemcpyAsync(codes, km->codes.p, (size_t)km->ds->n * km->cs.m * code_bytes(km->cs.k), hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
}

// ------------------------------------------------- row-sharded training (RCCL below the ABI) ----
int vqhip_comm_unique_id(uint8_t *id) {
    VQ_API_BEGIN
    if (!id) return fail(VQHIP_ERR_NULL_PTR, "id is NULL");
    return comm_unique_id(id);
    VQ_API_END
}

int vqhip_comm_create(const uint8_t *id, int world, int rank, vqhip_comm **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (world > 1 && !id) return fail(VQHIP_ERR_NULL_PTR, "a communicator of %d ranks needs the unique id", world);
    if (id) VQ_TRY(require_gfx950());  // ncclCommInitRank binds the calling thread's current device
    std::unique_ptr<vqhip_comm> h(new vqhip_comm());
    VQ_TRY(comm_create(id, world, rank, &h->c));
    *out = h.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_comm_adopt(void *nccl_comm, vqhip_comm **out) {
    VQ_API_BEGIN
    if (!out || !nccl_comm) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *out = nullptr;
    std::unique_ptr<vqhip_comm> h(new vqhip_comm());
    VQ_TRY(comm_adopt(nccl_comm, &h->c));
    *out = h.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_comm_info(const vqhip_comm *comm, int *world, int *rank) {
    comm_info(comm ? comm->c : nullptr, world, rank);
    return VQHIP_OK;
}

int vqhip_comm_destroy(vqhip_comm *comm) {
    if (comm) {
        (void)comm_destroy(comm->c);
        delete comm;
    }
    return VQHIP_OK;
}

struct vqhip_comm_group {
    LocalGroup *g = nullptr;
};

int vqhip_comm_group_create(int world, vqhip_comm_group **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    std::unique_ptr<vqhip_comm_group> h(new vqhip_comm_group());
    VQ_TRY(local_group_create(world, &h->g));
    *out = h.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_comm_create_local(vqhip_comm_group *group, int rank, vqhip_comm **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!group) return fail(VQHIP_ERR_NULL_PTR, "group is NULL");
    VQ_TRY(require_gfx950());
    std::unique_ptr<vqhip_comm> h(new vqhip_comm());
    VQ_TRY(comm_create_local(group->g, rank, &h->c));
    *out = h.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_comm_group_destroy(vqhip_comm_group *group) {
    if (group) {
        local_group_destroy(group->g);
        delete group;
    }
    return VQHIP_OK;
}

// from ANY thread, no lock taken (the thread that owns the communicator may be blocked inside a collective with it)
int vqhip_comm_abort(vqhip_comm *comm) {
    if (!comm || !comm->c) return VQHIP_OK;
    comm_abort(comm->c, "aborted by the caller (vqhip_comm_abort)");
    comm_abort_rccl(comm->c);
    return VQHIP_OK;
}

int vqhip_comm_kind(const vqhip_comm *comm, int *kind) {
    if (!kind) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    *kind = comm_kind(comm ? comm->c : nullptr);
    return VQHIP_OK;
}

static int kmeans_allreduce_impl(vqhip_kmeans *km, vqhip_comm *comm) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(km->sync);
    std::unique_lock<std::recursive_mutex> lk_comm;
    if (comm) lk_comm = std::unique_lock<std::recursive_mutex>(comm->mu);
    if (!km->accumulated) return fail(VQHIP_ERR_INVALID_INPUT, "allreduce without a preceding accumulate");
    int world = 1;
    comm_info(comm ? comm->c : nullptr, &world, nullptr);
    if (world > 1 && km->exact_update)
        return fail(VQHIP_ERR_UNSUPPORTED, "exact_update sums rows in one sequential chain: single GPU only");
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    return comm_allreduce_f64(comm ? comm->c : nullptr, km->slab.as<double>(),
                              (size_t)km->cs.m * km->cs.k * (km->cs.sd + 1), s);
    VQ_API_END
}

int vqhip_kmeans_allreduce(vqhip_kmeans *km, vqhip_comm *comm) { return sharded_exit(comm, kmeans_allreduce_impl(km, comm)); }

static int kmeans_step_sharded_impl(vqhip_kmeans *km, vqhip_comm *comm, uint32_t *counts, uint8_t *changed) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    std::unique_lock<std::recursive_mutex> lk_comm;
    if (comm) lk_comm = std::unique_lock<std::recursive_mutex>(comm->mu);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_TRY(kmeans_accumulate_enqueue(km, s));
    VQ_TRY(kmeans_allreduce_impl(km, comm));
    VQ_TRY(kmeans_finalize_enqueue(km, s));
    VQ_TRY(spin_wait(s));
    in.synced();
    kmeans_finalize_collect(km, counts, changed);
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_kmeans_step_sharded(vqhip_kmeans *km, vqhip_comm *comm, uint32_t *counts, uint8_t *changed) { return sharded_exit(comm, kmeans_step_sharded_impl(km, comm, counts, changed)); }

// bits of the owned rows among `global_rows` [m][k] into xs_ws (device u32 [m][k][sd]); zeros elsewhere
static int gather_owned_enqueue(vqhip_kmeans *km, const uint64_t *global_rows, uint64_t row_offset, hipStream_t s) {
    const size_t cnt = (size_t)km->cs.m * km->cs.k;
    VQ_TRY(km->gather_ws.ensure(cnt * km->cs.sd * 4));
    VQ_HIP(hipMemcpyAsync(km->rows_tmp.p, global_rows, cnt * 8, hipMemcpyHostToDevice, s));
    return launch_gather_rows_owned(km->ds->X, km->ds->d, km->cs.m, km->cs.k, km->cs.sd, km->rows_tmp.as<uint64_t>(),
                                    row_offset, km->ds->n, km->gather_ws.as<uint32_t>(), s);
}

int vqhip_kmeans_gather_owned_rows(vqhip_kmeans *km, const uint64_t *global_rows, uint64_t row_offset, uint32_t *bits_out) {
    VQ_API_BEGIN
    if (!km || !global_rows || !bits_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    VQ_TRY(gather_owned_enqueue(km, global_rows, row_offset, s));
    VQ_HIP(hipMemcpyAsync(bits_out, km->gather_ws.p, (size_t)km->cs.m * km->cs.k * km->cs.sd * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
    VQ_API_END
}

static int kmeans_init_from_global_rows_impl(vqhip_kmeans *km, vqhip_comm *comm, const uint64_t *global_rows, uint64_t row_offset) {
    VQ_API_BEGIN
    if (!km || !global_rows) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    std::unique_lock<std::recursive_mutex> lk_comm;
    if (comm) lk_comm = std::unique_lock<std::recursive_mutex>(comm->mu);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const size_t words = (size_t)km->cs.m * km->cs.k * km->cs.sd;
    VQ_TRY(gather_owned_enqueue(km, global_rows, row_offset, s));
    VQ_TRY(comm_allreduce_u32(comm ? comm->c : nullptr, km->gather_ws.as<uint32_t>(), words, s));
    VQ_HIP(hipMemcpyAsync(km->cs.cb.p, km->gather_ws.p, words * 4, hipMemcpyDeviceToDevice, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    km->cs.prepared = false;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_kmeans_init_from_global_rows(vqhip_kmeans *km, vqhip_comm *comm, const uint64_t *global_rows, uint64_t row_offset) { return sharded_exit(comm, kmeans_init_from_global_rows_impl(km, comm, global_rows, row_offset)); }

static int kmeans_patch_from_global_row_impl(vqhip_kmeans *km, vqhip_comm *comm, uint32_t sub, uint32_t j, uint64_t global_row, uint64_t row_offset) {
    VQ_API_BEGIN
    if (!km) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (sub >= km->cs.m || j >= km->cs.k) return fail(VQHIP_ERR_INVALID_INPUT, "centroid (%u,%u) out of range", sub, j);
    VQ_TRY(require_gfx950());
    Entry in(km->sync);
    std::unique_lock<std::recursive_mutex> lk_comm;
    if (comm) lk_comm = std::unique_lock<std::recursive_mutex>(comm->mu);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const uint32_t sd = km->cs.sd;
    VQ_TRY(km->gather_ws.ensure((size_t)km->cs.m * km->cs.k * sd * 4));
    VQ_HIP(hipMemcpyAsync(km->rows_tmp.p, &global_row, 8, hipMemcpyHostToDevice, s));
    // one (subspace, cluster) pair: the kernel's subspace 0 is column block `sub` of the rows
    VQ_TRY(launch_gather_rows_owned(km->ds->X + (size_t)sub * sd, km->ds->d, 1, 1, sd, km->rows_tmp.as<uint64_t>(),
                                    row_offset, km->ds->n, km->gather_ws.as<uint32_t>(), s));
    VQ_TRY(comm_allreduce_u32(comm ? comm->c : nullptr, km->gather_ws.as<uint32_t>(), sd, s));
    VQ_HIP(hipMemcpyAsync(km->cs.cb.as<float>() + ((size_t)sub * km->cs.k + j) * sd, km->gather_ws.p, (size_t)sd * 4,
                          hipMemcpyDeviceToDevice, s));
    VQ_HIP(hipStreamSynchronize(s));  // &global_row is a stack address
    in.synced();
    km->cs.prepared = false;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_kmeans_patch_from_global_row(vqhip_kmeans *km, vqhip_comm *comm, uint32_t sub, uint32_t j, uint64_t global_row, uint64_t row_offset) { return sharded_exit(comm, kmeans_patch_from_global_row_impl(km, comm, sub, j, global_row, row_offset)); }

// ----------------------------------------------------------------------- PQ encode ----
int vqhip_pq_encoder_create(const float *codebooks, uint32_t m, uint32_t k, uint32_t sub_dim, int metric,
                            vqhip_pq_encoder **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!codebooks) return fail(VQHIP_ERR_NULL_PTR, "codebooks is NULL");
    if (m == 0 || k == 0 || sub_dim == 0) return fail(VQHIP_ERR_INVALID_INPUT, "m, k and sub_dim must be positive");
    if (k > kMaxCentroids) return fail(VQHIP_ERR_UNSUPPORTED, "k=%u > 65536: codes are at most two bytes per subspace", k);
    if (metric < VQHIP_SQUARED_EUCLIDEAN || metric > VQHIP_COSINE_UNCLAMPED) return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_pq_encoder> enc(new vqhip_pq_encoder());
    enc->metric = metric;
    VQ_TRY(enc->cs.init(m, k, sub_dim, true));
    enc->cs.metric = (metric == VQHIP_COSINE) ? VQHIP_COSINE : VQHIP_SQUARED_EUCLIDEAN;
    VQ_HIP(hipMemcpyAsync(enc->cs.cb.p, codebooks, (size_t)m * k * sub_dim * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < m; ++i) enc->all_subs.push_back(i);
    *out = enc.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_encoder_destroy(vqhip_pq_encoder *enc) {
    delete enc;
    return VQHIP_OK;
}

int vqhip_pq_encoder_set_engine(vqhip_pq_encoder *enc, int engine) {
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (engine < VQHIP_ENGINE_AUTO || engine > VQHIP_ENGINE_MFMA_BF16) return fail(VQHIP_ERR_INVALID_INPUT, "unknown engine %d", engine);
    std::lock_guard<std::recursive_mutex> lk(enc->sync.mu);
    enc->engine = engine;
    return VQHIP_OK;
}

int vqhip_pq_encode_device(vqhip_pq_encoder *enc, const void *dev_rows, uint64_t n, void *dev_codes, void *dev_f16_out) {
    VQ_API_BEGIN
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "encoder is NULL");
    if (n == 0) return VQHIP_OK;
    if (!dev_rows) return fail(VQHIP_ERR_NULL_PTR, "dev_rows is NULL");
    VQ_TRY(require_gfx950());
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    uint8_t *codes = reinterpret_cast<uint8_t *>(dev_codes);
    if (!codes) {  // f16-only output still needs the codes internally
        VQ_TRY(enc->codes.ensure((size_t)n * enc->cs.m * code_bytes(enc->cs.k)));
        codes = enc->codes.as<uint8_t>();
    }
    g_last_ws = enc->ws_id;
    VQ_TRY(run_assign(enc->cs, enc->ws, reinterpret_cast<const float *>(dev_rows), n, enc->cs.m * enc->cs.sd,
                      enc->metric, enc->all_subs, codes, enc->engine, s));
    if (dev_f16_out) VQ_TRY(launch_gather_f16(enc->cs.view(), codes, n, reinterpret_cast<uint16_t *>(dev_f16_out), s));
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_encode(vqhip_pq_encoder *enc, const float *rows, uint64_t n, uint8_t *codes, uint16_t *f16_out) {
    VQ_API_BEGIN
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "encoder is NULL");
    if (n == 0) return VQHIP_OK;
    if (!rows) return fail(VQHIP_ERR_NULL_PTR, "rows is NULL");
    VQ_TRY(require_gfx950());
    Entry in(enc->sync);
    const uint32_t m = enc->cs.m, k = enc->cs.k, sd = enc->cs.sd, d = m * sd;
    const size_t cw = code_bytes(k);  // bytes per code: 1 (k <= 256) or 2
    // per-vector calls (Quantizer::quantize): one kernel over mapped pinned memory, exact arithmetic.  The kernel reads
    // only what an encoder never changes after its first use (codebooks, centroid norms), and the staging belongs to the
    // call: the handle is given back before the launch, so calls from many threads on one encoder (`quantize(&self)` on
    // a Sync type, src/pq.rs:39-45) run side by side on their threads' streams, with no order behind the handle's queued
    // batch work once the images are known to be complete.
    const bool small = n <= kSmallRows;
    if (small) {
        if (!enc->small_ready) {
            // once per encoder: s is ordered behind the handle's tail here (in.stream), so the wait also covers a prepare
            // another thread's asynchronous batch call enqueued on ITS stream; other threads' streams read the images
            // without any order from now on
            hipStream_t s;
            VQ_TRY(in.stream(&s));
            if (!(enc->cs.prepared && enc->cs.prepared_base)) VQ_TRY(enc->cs.prepare(s));  // centroid norms (cosine)
            VQ_HIP(hipStreamSynchronize(s));
            in.synced();
            enc->small_ready = true;
        }
        enc->ws.stats_pending = false;
        enc->ws.last_engine = VQHIP_ENGINE_EXACT;
    }
    const int metric = enc->metric;
    const float *cb = enc->cs.cb.as<float>(), *cnsqrt = enc->cs.cnsqrt.as<float>();
    auto small_launch = [&](const void *di, uint64_t nr, void *dc, void *df, hipStream_t s) {
        return launch_pq_encode_small(static_cast<const float *>(di), (uint32_t)nr, d, m, k, sd, metric, cb, cnsqrt,
                                      static_cast<uint8_t *>(dc), static_cast<uint16_t *>(df), s);
    };
    // (the device form takes the handle itself; on a lane that is the lane's thread, on the lane's stream)
    auto chunk_launch = [enc](const void *di, uint64_t nr, void *dc, void *df, hipStream_t) {
        return vqhip_pq_encode_device(enc, di, nr, dc, df);
    };
    XferTier tier = XferTier::kStream;
    const int rc = host_batch(HostBatch{rows, (size_t)d * 4, codes, m * cw, f16_out, (size_t)d * 2, n, 1}, &in, small,
                              small_launch, chunk_launch, enc->xbuf, enc->codes, enc->f16buf, &tier);
    if (tier == XferTier::kLanes) {
        // "the most recent pass of this thread" for vqhip_last_assign_stats: the lanes' passes were this call's
        g_last_ws = enc->ws_id;
        std::lock_guard<std::recursive_mutex> lk(enc->sync.mu);
        tls().last_engine = enc->ws.last_engine;
        tls().last_products = enc->ws.last_products;
    }
    VQ_TRY(rc);
    if (tier == XferTier::kVector) {
        ThreadState &st = tls();
        st.last_engine = VQHIP_ENGINE_EXACT;
        st.last_rechecked = 0;
        g_last_ws = 0;
    }
    return VQHIP_OK;
    VQ_API_END
}

// ------------------------------------------------------------------------ ADC search ----
// dev_mask: a filtered call's row mask on the device, ceil(n / 32) words (adc_search_masked below); NULL: every row.  A
// filtered call never takes the sampled-threshold schedule -- a sample of evenly spaced rows says nothing about the
// allowed ones -- and goes through the full pass with the masked scan and the masked source.
static int adc_search(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, const float *queries, uint32_t nq, uint32_t topk,
                      uint32_t *idx_out, float *dist_out, const uint32_t *dev_mask) {
    VQ_API_BEGIN
    if (!enc || !dev_codes || !queries || !idx_out || !dist_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (nq == 0) return VQHIP_OK;
    if (n == 0 || n >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "n must be in [1, 2^32)");
    VQ_TRY(require_gfx950());
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const uint32_t m = enc->cs.m, k = enc->cs.k, sd = enc->cs.sd, dim = m * sd;
    constexpr uint32_t kAdcCallQueries = 4096;  // per set of launches: the candidate lists are 64 KB per query
    if (nq > kAdcCallQueries) {
        uint32_t redone = 0;
        for (uint32_t q0 = 0; q0 < nq; q0 += kAdcCallQueries) {
            const uint32_t cn = std::min(kAdcCallQueries, nq - q0);
            VQ_TRY(adc_search(enc, dev_codes, n, queries + (size_t)q0 * dim, cn, topk, idx_out + (size_t)q0 * topk,
                              dist_out + (size_t)q0 * topk, dev_mask));
            redone += enc->adc_last_redone;
        }
        enc->adc_last_redone = redone;
        return VQHIP_OK;
    }
    // (refused before any workspace is sized by the table: both schedules take m * k <= kAdcMaxTable, adc_plan.hpp)
    if (!vq_is_cos(enc->metric) && !adc_table_fits(m, k)) return fail_adc_table(m, k);
    VQ_TRY(enc->adc_q.ensure((size_t)nq * dim * 4));
    VQ_TRY(enc->adc_idx.ensure((size_t)nq * topk * 4));
    VQ_TRY(enc->adc_out.ensure((size_t)nq * topk * 4));
    // Small calls stage through pinned, device-mapped memory: the queries leave as one asynchronous DMA and the results
    // are WRITTEN into host memory by the last kernel -- a copy from or into pageable memory is a staged transfer inside
    // the runtime that holds the calling thread (~12 us each; an 8-query call spent more time in its four copies than in
    // its kernels)
    const size_t q_b = (size_t)nq * dim * 4, nres = (size_t)nq * topk, pack_b = (2 * nres + 2 * (size_t)nq) * 4;
    const bool fast = !dev_mask && adc_fast_eligible(m, k, n, topk), staged = fast && q_b + pack_b <= (1u << 20);
    StageLease stage;
    if (staged) {
        VQ_TRY(stage.acquire(q_b + pack_b));
        memcpy(stage.host(), queries, q_b);  // (the table kernel reads them from there: no copy engine in front of the kernels)
    } else {
        VQ_HIP(hipMemcpyAsync(enc->adc_q.p, queries, q_b, hipMemcpyHostToDevice, s));
    }
    // the full pass (every distance written, histogram cut, candidates collected) for the queries [q0, q0 + cnt)
    auto full_pass = [&](uint32_t q0, uint32_t cnt) -> int {
        const uint32_t qg = adc_query_group(n, cnt);
        VQ_TRY(enc->adc_lut.ensure((size_t)qg * m * k * 4));
        VQ_TRY(enc->adc_dist.ensure((size_t)qg * n * 4));
        VQ_TRY(enc->adc_state.ensure(adc_state_bytes(qg)));
        VQ_TRY(enc->adc_cand.ensure(topk_cand_bytes(qg)));
        return launch_adc_search(enc->cs.cb.as<float>(), m, k, sd, enc->metric, reinterpret_cast<const uint8_t *>(dev_codes), n,
                                 enc->adc_q.as<float>() + (size_t)q0 * dim, cnt, topk, enc->adc_lut.as<float>(), enc->adc_dist.as<float>(),
                                 enc->adc_state.p, enc->adc_cand.as<unsigned long long>(), enc->adc_idx.as<uint32_t>() + (size_t)q0 * topk,
                                 enc->adc_out.as<float>() + (size_t)q0 * topk, s, qg, dev_mask);
    };
    if (fast) {
        // one scan of the codes per batch of queries against a sampled threshold, only candidates written (k_adc.hip);
        // a query whose threshold let too few or too many rows pass is repeated through the full pass
        VQ_TRY(enc->adc_lut.ensure(adc_fast_lut_bytes(m, k, nq)));
        VQ_TRY(enc->adc_state.ensure(adc_fast_state_bytes(m, k, nq)));
        VQ_TRY(enc->adc_cand.ensure(adc_fast_cand_bytes(m, k, nq)));
        // results, flags and candidate counts in ONE buffer: [nq][topk] idx | [nq][topk] dist | [nq] redo | [nq] count -- one
        // copy back instead of three (each a staged transfer of its own into pageable memory, ~12 us)
        if (!staged) VQ_TRY(enc->adc_redo.ensure(pack_b));
        uint32_t *pack_dev = staged ? reinterpret_cast<uint32_t *>(stage.dev() + q_b) : enc->adc_redo.as<uint32_t>();
        VQ_TRY(launch_adc_search_fast(enc->cs.cb.as<float>(), m, k, sd, enc->metric, reinterpret_cast<const uint8_t *>(dev_codes), n,
                                      staged ? reinterpret_cast<const float *>(stage.dev()) : enc->adc_q.as<float>(), nq, topk, enc->adc_lut.as<float>(), enc->adc_state.p,
                                      enc->adc_cand.as<unsigned long long>(), pack_dev, reinterpret_cast<float *>(pack_dev + nres),
                                      pack_dev + 2 * nres, s));
        std::vector<uint32_t> pack_copy;
        const uint32_t *pack = nullptr;
        if (staged) {
            VQ_TRY(spin_wait(s));
            pack = reinterpret_cast<const uint32_t *>(stage.host() + q_b);
        } else {
            pack_copy.resize(2 * nres + 2 * (size_t)nq);
            VQ_HIP(hipMemcpyAsync(pack_copy.data(), pack_dev, pack_b, hipMemcpyDeviceToHost, s));
            VQ_HIP(hipStreamSynchronize(s));
            pack = pack_copy.data();
        }
        memcpy(idx_out, pack, nres * 4);
        memcpy(dist_out, pack + nres, nres * 4);
        const uint32_t *redo = pack + 2 * nres;
        uint32_t redone = 0;
        for (uint32_t q0 = 0; q0 < nq;) {
            if (!redo[q0]) {
                ++q0;
                continue;
            }
            uint32_t q1 = q0;
            while (q1 < nq && redo[q1]) ++q1;  // a run of flagged queries goes through together
            if (staged && !redone) VQ_HIP(hipMemcpyAsync(enc->adc_q.p, queries, q_b, hipMemcpyHostToDevice, s));  // (the full pass reads them from device memory)
            VQ_TRY(full_pass(q0, q1 - q0));
            VQ_HIP(hipMemcpyAsync(idx_out + (size_t)q0 * topk, enc->adc_idx.as<uint32_t>() + (size_t)q0 * topk, (size_t)(q1 - q0) * topk * 4, hipMemcpyDeviceToHost, s));
            VQ_HIP(hipMemcpyAsync(dist_out + (size_t)q0 * topk, enc->adc_out.as<float>() + (size_t)q0 * topk, (size_t)(q1 - q0) * topk * 4, hipMemcpyDeviceToHost, s));
            VQ_HIP(hipStreamSynchronize(s));
            redone += q1 - q0;
            q0 = q1;
        }
        enc->adc_last_redone = redone;
        in.synced();
        return VQHIP_OK;
    }
    VQ_TRY(full_pass(0, nq));
    enc->adc_last_redone = nq;
    VQ_HIP(hipMemcpyAsync(idx_out, enc->adc_idx.p, (size_t)nq * topk * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipMemcpyAsync(dist_out, enc->adc_out.p, (size_t)nq * topk * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_adc_search_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, const float *queries,
                               uint32_t nq, uint32_t topk, uint32_t *idx_out, float *dist_out) {
    return adc_search(enc, dev_codes, n, queries, nq, topk, idx_out, dist_out, nullptr);
}

}  // extern "C"

// The filtered forms: the host mask, ceil(n / 32) words, goes up once per call into the encoder's adc_mask, under the
// encoder's lock; the search behind it is adc_search over the device codes that codes_up(s, &dev_codes) names or uploads.
template <class CodesUp>
static int adc_search_masked(vqhip_pq_encoder *enc, uint64_t n, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                             uint32_t *idx_out, float *dist_out, CodesUp &&codes_up) {
    Entry in(enc->sync);
    if (nq == 0) return VQHIP_OK;
    if (n == 0 || n >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "n must be in [1, 2^32)");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const void *dev_codes = nullptr;
    VQ_TRY(codes_up(s, &dev_codes));
    const size_t mask_b = (size_t)((n + 31) / 32) * 4;
    VQ_TRY(enc->adc_mask.ensure(mask_b));
    VQ_HIP(hipMemcpyAsync(enc->adc_mask.p, allowed, mask_b, hipMemcpyHostToDevice, s));
    return adc_search(enc, dev_codes, n, queries, nq, topk, idx_out, dist_out, enc->adc_mask.as<uint32_t>());
}

extern "C" {

int vqhip_pq_adc_search_masked_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, const float *queries, uint32_t nq,
                                      uint32_t topk, const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    if (!enc || !dev_codes || !queries || !allowed || !idx_out || !dist_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    return adc_search_masked(enc, n, queries, nq, topk, allowed, idx_out, dist_out, [&](hipStream_t, const void **codes) -> int {
        *codes = dev_codes;
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_pq_adc_search_resident_masked(vqhip_pq_encoder *enc, const float *queries, uint32_t nq, uint32_t topk, const uint32_t *allowed,
                                        uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    if (!enc || !queries || !allowed || !idx_out || !dist_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(enc->sync);
    if (!enc->adc_resident_n) return fail(VQHIP_ERR_INVALID_INPUT, "no codes loaded: call vqhip_pq_adc_set_codes first");
    return adc_search_masked(enc, enc->adc_resident_n, queries, nq, topk, allowed, idx_out, dist_out,
                             [&](hipStream_t, const void **codes) -> int {
        *codes = enc->adc_resident.p;
        return VQHIP_OK;
    });
    VQ_API_END
}

int vqhip_pq_adc_search_masked(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, const float *queries, uint32_t nq, uint32_t topk,
                               const uint32_t *allowed, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    if (!enc || !codes || !queries || !allowed || !idx_out || !dist_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    return adc_search_masked(enc, n, queries, nq, topk, allowed, idx_out, dist_out, [&](hipStream_t s, const void **dev_codes) -> int {
        const size_t code_b = (size_t)n * enc->cs.m * code_bytes(enc->cs.k);
        VQ_TRY(enc->adc_codes.ensure(code_b));
        VQ_HIP(hipMemcpyAsync(enc->adc_codes.p, codes, code_b, hipMemcpyHostToDevice, s));
        *dev_codes = enc->adc_codes.p;
        return VQHIP_OK;
    });
    VQ_API_END
}

// A code store that is searched again and again (vq_amd.store.PQIndex): its codes uploaded ONCE into the encoder's own
// buffer, every later search is the device form over them (an 8 MB upload per call is 0.15 ms in front of a 0.06 ms search).
int vqhip_pq_adc_set_codes(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n) {
    VQ_API_BEGIN
    if (!enc || (!codes && n)) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "n must be below 2^32");
    VQ_TRY(require_gfx950());
    const uint32_t m = enc->cs.m, k = enc->cs.k, cw = code_bytes(k);
    VQ_TRY(check_codes(codes, n * m, k));  // the scan indexes its LDS tables by code: checked here, once, not per search
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    enc->adc_resident_n = 0;
    if (n) {
        VQ_TRY(enc->adc_resident.ensure((size_t)n * m * cw));
        VQ_HIP(hipMemcpyAsync(enc->adc_resident.p, codes, (size_t)n * m * cw, hipMemcpyHostToDevice, s));
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
    }
    enc->adc_resident_n = n;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_adc_search_resident(vqhip_pq_encoder *enc, const float *queries, uint32_t nq, uint32_t topk, uint32_t *idx_out,
                                 float *dist_out) {
    VQ_API_BEGIN
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(enc->sync);
    if (!enc->adc_resident_n) return fail(VQHIP_ERR_INVALID_INPUT, "no codes loaded: call vqhip_pq_adc_set_codes first");
    return vqhip_pq_adc_search_device(enc, enc->adc_resident.p, enc->adc_resident_n, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_pq_adc_last_redone(vqhip_pq_encoder *enc, uint32_t *queries_out) {
    VQ_API_BEGIN
    if (!enc || !queries_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(enc->sync);
    *queries_out = enc->adc_last_redone;
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_adc_search(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, const float *queries, uint32_t nq,
                        uint32_t topk, uint32_t *idx_out, float *dist_out) {
    VQ_API_BEGIN
    if (!enc || !codes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const size_t code_b = (size_t)n * enc->cs.m * code_bytes(enc->cs.k);
    VQ_TRY(enc->adc_codes.ensure(code_b));
    VQ_HIP(hipMemcpyAsync(enc->adc_codes.p, codes, code_b, hipMemcpyHostToDevice, s));
    return vqhip_pq_adc_search_device(enc, enc->adc_codes.p, n, queries, nq, topk, idx_out, dist_out);
    VQ_API_END
}

int vqhip_dequantize_f16(const uint16_t *f16_in, uint64_t count, float *out) {
    VQ_API_BEGIN
    if (count == 0) return VQHIP_OK;
    if (!f16_in || !out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    DevBuf in, o;
    VQ_TRY(in.alloc((size_t)count * 2));
    VQ_TRY(o.alloc((size_t)count * 4));
    VQ_HIP(hipMemcpyAsync(in.p, f16_in, (size_t)count * 2, hipMemcpyHostToDevice, s));
    VQ_TRY(launch_dequant_f16(in.as<uint16_t>(), count, o.as<float>(), s));
    VQ_HIP(hipMemcpyAsync(out, o.p, (size_t)count * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_pq_decode(vqhip_pq_encoder *enc, const uint8_t *codes, uint64_t n, float *out) {
    VQ_API_BEGIN
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "encoder is NULL");
    if (n == 0) return VQHIP_OK;
    if (!codes || !out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    const uint32_t m = enc->cs.m, d = enc->cs.m * enc->cs.sd;
    const size_t cw = code_bytes(enc->cs.k);
    VQ_TRY(check_codes(codes, n * m, enc->cs.k));
    VQ_TRY(enc->codes.ensure((size_t)n * m * cw));
    VQ_TRY(enc->f32buf.ensure((size_t)n * d * 4));
    VQ_HIP(hipMemcpyAsync(enc->codes.p, codes, (size_t)n * m * cw, hipMemcpyHostToDevice, s));
    VQ_TRY(launch_decode_f32(enc->cs.view(), enc->codes.as<uint8_t>(), n, enc->f32buf.as<float>(), s));
    VQ_HIP(hipMemcpyAsync(out, enc->f32buf.p, (size_t)n * d * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    in.synced();
    return VQHIP_OK;
    VQ_API_END
}

// device forms (asynchronous on the current stream, like vqhip_pq_encode_device): what a host that keeps codes / f16 rows
// resident calls, and what bench.py times.  Codes are the caller's to keep inside [0, k): an out-of-range code reads a
// wrong (in-bounds of the allocation or not) codebook row -- the host form checks, this one cannot without a read-back.
int vqhip_pq_decode_device(vqhip_pq_encoder *enc, const void *dev_codes, uint64_t n, void *dev_out) {
    VQ_API_BEGIN
    if (!enc) return fail(VQHIP_ERR_NULL_PTR, "encoder is NULL");
    if (n == 0) return VQHIP_OK;
    if (!dev_codes || !dev_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    Entry in(enc->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    return launch_decode_f32(enc->cs.view(), static_cast<const uint8_t *>(dev_codes), n, static_cast<float *>(dev_out), s);
    VQ_API_END
}

int vqhip_dequantize_f16_device(const void *dev_f16_in, uint64_t count, void *dev_out) {
    VQ_API_BEGIN
    if (count == 0) return VQHIP_OK;
    if (!dev_f16_in || !dev_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    return launch_dequant_f16(static_cast<const uint16_t *>(dev_f16_in), count, static_cast<float *>(dev_out), s);
    VQ_API_END
}

// ---------------------------------------------------------------- ScalarQuantizer / BinaryQuantizer ----
// Parameters are checked (and the tables built) before anything touches a device; see k_sqbq.hip for the arithmetic.
int vqhip_sq_check(float min, float max, uint32_t levels, float *step) {
    VQ_API_BEGIN
    return sq_check(min, max, levels, step);
    VQ_API_END
}

int vqhip_sq_thresholds(float min, float max, uint32_t levels, float *b) {
    VQ_API_BEGIN
    float step = 0;
    VQ_TRY(sq_check(min, max, levels, &step));
    if (!b) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    sq_thresholds(min, max, levels, step, b);
    return VQHIP_OK;
    VQ_API_END
}

static int sqbq_encode_host(const SqbqEncodeOp &op, const float *x, uint64_t count, uint8_t *codes) {
    if (count == 0) return VQHIP_OK;
    if (!x || !codes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    const HostBatch b{x, 4, codes, 1, nullptr, 0, count, 16};
    auto launch = [&](const void *dx, uint64_t n, void *dc, void *, hipStream_t s) {
        return launch_sqbq_encode(op, static_cast<const float *>(dx), n, static_cast<uint8_t *>(dc), s);
    };
    DevBuf dx, dc;
    return host_batch(b, nullptr, b.stage_bytes() <= kElementwiseSmallBytes, launch, launch, dx, dc, dc);
}
static int sqbq_decode_host(const SqbqDecodeLut &lut, const uint8_t *codes, uint64_t count, float *out) {
    if (count == 0) return VQHIP_OK;
    if (!codes || !out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    const HostBatch b{codes, 1, out, 4, nullptr, 0, count, 16};
    auto launch = [&](const void *dc, uint64_t n, void *dout, void *, hipStream_t s) {
        return launch_sqbq_decode(lut, static_cast<const uint8_t *>(dc), n, static_cast<float *>(dout), s);
    };
    DevBuf dc, dout;
    return host_batch(b, nullptr, b.stage_bytes() <= kElementwiseSmallBytes, launch, launch, dc, dout, dout);
}
static int sqbq_encode_dev(const SqbqEncodeOp &op, const void *dev_x, uint64_t count, void *dev_codes) {
    if (count == 0) return VQHIP_OK;
    if (!dev_x || !dev_codes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (reinterpret_cast<uintptr_t>(dev_x) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "x is not 4-byte aligned");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    return launch_sqbq_encode(op, static_cast<const float *>(dev_x), count, static_cast<uint8_t *>(dev_codes), s);
}
static int sqbq_decode_dev(const SqbqDecodeLut &lut, const void *dev_codes, uint64_t count, void *dev_out) {
    if (count == 0) return VQHIP_OK;
    if (!dev_codes || !dev_out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (reinterpret_cast<uintptr_t>(dev_out) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "out is not 4-byte aligned");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    return launch_sqbq_decode(lut, static_cast<const uint8_t *>(dev_codes), count, static_cast<float *>(dev_out), s);
}

int vqhip_sq_encode(float min, float max, uint32_t levels, const float *x, uint64_t count, uint8_t *codes) {
    VQ_API_BEGIN
    SqbqEncodeOp op;
    VQ_TRY(sq_encode_op(min, max, levels, &op));
    return sqbq_encode_host(op, x, count, codes);
    VQ_API_END
}

int vqhip_sq_encode_device(float min, float max, uint32_t levels, const void *dev_x, uint64_t count, void *dev_codes) {
    VQ_API_BEGIN
    SqbqEncodeOp op;
    VQ_TRY(sq_encode_op(min, max, levels, &op));
    return sqbq_encode_dev(op, dev_x, count, dev_codes);
    VQ_API_END
}

int vqhip_sq_decode(float min, float max, uint32_t levels, const uint8_t *codes, uint64_t count, float *out) {
    VQ_API_BEGIN
    SqbqDecodeLut lut;
    VQ_TRY(sq_decode_lut(min, max, levels, &lut));
    return sqbq_decode_host(lut, codes, count, out);
    VQ_API_END
}

int vqhip_sq_decode_device(float min, float max, uint32_t levels, const void *dev_codes, uint64_t count, void *dev_out) {
    VQ_API_BEGIN
    SqbqDecodeLut lut;
    VQ_TRY(sq_decode_lut(min, max, levels, &lut));
    return sqbq_decode_dev(lut, dev_codes, count, dev_out);
    VQ_API_END
}

int vqhip_bq_check(float threshold, uint32_t low, uint32_t high) {
    VQ_API_BEGIN
    return bq_check(threshold, low, high);
    VQ_API_END
}

int vqhip_bq_encode(float threshold, uint32_t low, uint32_t high, const float *x, uint64_t count, uint8_t *codes) {
    VQ_API_BEGIN
    SqbqEncodeOp op;
    VQ_TRY(bq_encode_op(threshold, low, high, &op));
    return sqbq_encode_host(op, x, count, codes);
    VQ_API_END
}

int vqhip_bq_encode_device(float threshold, uint32_t low, uint32_t high, const void *dev_x, uint64_t count,
                           void *dev_codes) {
    VQ_API_BEGIN
    SqbqEncodeOp op;
    VQ_TRY(bq_encode_op(threshold, low, high, &op));
    return sqbq_encode_dev(op, dev_x, count, dev_codes);
    VQ_API_END
}

int vqhip_bq_decode(float threshold, uint32_t low, uint32_t high, const uint8_t *codes, uint64_t count, float *out) {
    VQ_API_BEGIN
    SqbqDecodeLut lut;
    VQ_TRY(bq_decode_lut(threshold, low, high, &lut));
    return sqbq_decode_host(lut, codes, count, out);
    VQ_API_END
}

int vqhip_bq_decode_device(float threshold, uint32_t low, uint32_t high, const void *dev_codes, uint64_t count,
                           void *dev_out) {
    VQ_API_BEGIN
    SqbqDecodeLut lut;
    VQ_TRY(bq_decode_lut(threshold, low, high, &lut));
    return sqbq_decode_dev(lut, dev_codes, count, dev_out);
    VQ_API_END
}

int vqhip_distance_batch(int metric, const float *a, const float *b, uint64_t n, uint32_t d, float *out) {
    VQ_API_BEGIN
    if (n == 0) return VQHIP_OK;
    if (!a || !b || !out) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (metric < VQHIP_SQUARED_EUCLIDEAN || metric > VQHIP_COSINE_UNCLAMPED) return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    DevBuf da, db, dout;
    VQ_TRY(da.alloc((size_t)n * d * 4));
    VQ_TRY(db.alloc((size_t)n * d * 4));
    VQ_TRY(dout.alloc((size_t)n * 4));
    VQ_HIP(hipMemcpyAsync(da.p, a, (size_t)n * d * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipMemcpyAsync(db.p, b, (size_t)n * d * 4, hipMemcpyHostToDevice, s));
    VQ_TRY(launch_distance_batch(metric, da.as<float>(), db.as<float>(), n, d, dout.as<float>(), s));
    VQ_HIP(hipMemcpyAsync(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    VQ_HIP(hipStreamSynchronize(s));
    return VQHIP_OK;
    VQ_API_END
}

// ------------------------------------------------------------------ resident indexes: the shared host layer ----
// What vqhip_flat, vqhip_sqindex and vqhip_binary have in common: the rows stay on the device from create on, a search
// takes [nq][d] f32 queries to [nq][topk] results, and every call locks the handle and runs on the calling thread's stream.
}  // extern "C"

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

// The two indexes of exact distances.  T (vqhip_flat, vqhip_sqindex) keeps its rows and the three launcher calls that
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
static int check_mask_aligned(const void *dev_allowed) {
    if (reinterpret_cast<uintptr_t>(dev_allowed) & 3) return fail(VQHIP_ERR_INVALID_INPUT, "the row mask is not 4-byte aligned");
    return VQHIP_OK;
}

// every create takes 1 <= n < 2^32 rows and a metric of include/vqhip.h (two checks: each create has its own between them)
static int check_rows(uint64_t n) {
    if (n == 0 || n >= (1ull << 32)) return fail(VQHIP_ERR_INVALID_INPUT, "n must be in [1, 2^32)");
    return VQHIP_OK;
}
static int check_metric(int metric) {
    if (metric < VQHIP_SQUARED_EUCLIDEAN || metric > VQHIP_COSINE_UNCLAMPED) return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    return VQHIP_OK;
}

// every index's search takes 1 <= topk <= min(n, 1024)
static int check_topk(uint64_t n, uint32_t topk) {
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
static void swap_buf(DevBuf &a, DevBuf &b) {
    std::swap(a.p, b.p);
    std::swap(a.bytes, b.bytes);
}

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

// rows from host (kind = H2D) or device (D2D) memory into a new index
static int flat_create(const void *src, hipMemcpyKind kind, uint64_t n, uint32_t d, int dtype, int metric, vqhip_flat **out) {
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

static int binary_check(int kind, uint64_t n, uint32_t d, float threshold, uint32_t low, uint32_t high, int metric) {
    if (kind != VQHIP_BINARY_F32 && kind != VQHIP_BINARY_U8 && kind != VQHIP_BINARY_PACKED)
        return fail(VQHIP_ERR_INVALID_INPUT, "source kind must be 0 (f32), 1 (u8 codes) or 2 (packed words), not %d", kind);
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
    if (kind == VQHIP_BINARY_PACKED && kind_copy == hipMemcpyHostToDevice && d % 32) {
        const uint32_t *w = static_cast<const uint32_t *>(src), mask = (1u << (d % 32)) - 1u;
        for (uint64_t i = 0; i < n; ++i)
            if (w[i * W + W - 1] & ~mask) return fail(VQHIP_ERR_INVALID_INPUT, "row %llu has a pad bit set", (unsigned long long)i);
    }
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
    if (kind == VQHIP_BINARY_PACKED) {
        VQ_HIP(hipMemcpyAsync(b->words.p, src, (size_t)n * W * 4, kind_copy, s));
        if (kind_copy == hipMemcpyDeviceToDevice && d % 32) {
            DevBuf bad;
            uint32_t h_bad = 0;
            VQ_TRY(bad.alloc(4));
            VQ_HIP(hipMemsetAsync(bad.p, 0, 4, s));
            VQ_TRY(launch_bin_padcheck(b->words.as<uint32_t>(), n, d, bad.as<uint32_t>(), s));
            VQ_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
            VQ_HIP(hipStreamSynchronize(s));
            if (h_bad) return fail(VQHIP_ERR_INVALID_INPUT, "a packed row has a pad bit set");
        }
    } else if (kind_copy == hipMemcpyDeviceToDevice) {
        VQ_TRY(launch_bq_pack(src, kind, n, d, threshold, high, b->words.as<uint32_t>(), s));
    } else {  // host rows are packed a piece at a time
        VQ_TRY(staged_rows(src, n, (size_t)d * (kind == VQHIP_BINARY_U8 ? 1 : 4), s, [&](const void *piece, uint64_t r0, uint64_t rn) {
            return launch_bq_pack(piece, kind, rn, d, threshold, high, b->words.as<uint32_t>() + r0 * W, s);
        }));
    }
    VQ_HIP(hipStreamSynchronize(s));  // the caller may free or change its source once this returns
    *out = b.release();
    return VQHIP_OK;
}

// n_add rows of `kind` (vqhip_binary_create's three) behind the last, with create's checks of the source
static int binary_add(vqhip_binary *b, const void *src, hipMemcpyKind kind_copy, int kind, uint64_t n_add) {
    if (!b) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_add == 0) return VQHIP_OK;
    if (!src) return fail(VQHIP_ERR_NULL_PTR, "source is NULL");
    if (kind != VQHIP_BINARY_F32 && kind != VQHIP_BINARY_U8 && kind != VQHIP_BINARY_PACKED)
        return fail(VQHIP_ERR_INVALID_INPUT, "source kind must be 0 (f32), 1 (u8 codes) or 2 (packed words), not %d", kind);
    const bool dev = kind_copy == hipMemcpyDeviceToDevice;
    if (dev && kind != VQHIP_BINARY_U8 && (reinterpret_cast<uintptr_t>(src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, kind == VQHIP_BINARY_F32 ? "rows are not 4-byte aligned" : "words are not 4-byte aligned");
    const uint32_t d = b->d, W = b->W;  // (fixed at create)
    if (kind == VQHIP_BINARY_PACKED && !dev && d % 32) {
        const uint32_t *w = static_cast<const uint32_t *>(src), mask = (1u << (d % 32)) - 1u;
        for (uint64_t i = 0; i < n_add; ++i)
            if (w[i * W + W - 1] & ~mask) return fail(VQHIP_ERR_INVALID_INPUT, "added row %llu has a pad bit set", (unsigned long long)i);
    }
    return resident_add(b, src, n_add, [&](char *dst, hipStream_t s) -> int {
        uint32_t *words = reinterpret_cast<uint32_t *>(dst);
        if (kind == VQHIP_BINARY_PACKED) {
            VQ_HIP(hipMemcpyAsync(words, src, (size_t)n_add * W * 4, kind_copy, s));
            if (dev && d % 32) {
                DevBuf bad;
                uint32_t h_bad = 0;
                VQ_TRY(bad.alloc(4));
                VQ_HIP(hipMemsetAsync(bad.p, 0, 4, s));
                VQ_TRY(launch_bin_padcheck(words, n_add, d, bad.as<uint32_t>(), s));
                VQ_HIP(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, s));
                VQ_HIP(hipStreamSynchronize(s));
                if (h_bad) return fail(VQHIP_ERR_INVALID_INPUT, "an added packed row has a pad bit set");
            }
            return VQHIP_OK;
        }
        if (dev) return launch_bq_pack(src, kind, n_add, d, b->thr, b->high, words, s);
        return staged_rows(src, n_add, (size_t)d * (kind == VQHIP_BINARY_U8 ? 1 : 4), s, [&](const void *piece, uint64_t r0, uint64_t rn) {
            return launch_bq_pack(piece, kind, rn, d, b->thr, b->high, words + r0 * W, s);
        });
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
    if (kind == VQHIP_BINARY_F32 && (reinterpret_cast<uintptr_t>(dev_src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, "rows are not 4-byte aligned");
    if (kind == VQHIP_BINARY_PACKED && (reinterpret_cast<uintptr_t>(dev_src) & 3))
        return fail(VQHIP_ERR_INVALID_INPUT, "words are not 4-byte aligned");
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

// ------------------------------------------------------------------ inverted lists: the shared host layer ----
// What vqhip_ivfpq, vqhip_ivfflat, vqhip_ivfsq and vqhip_ivfbin have in common.  Host state: the coarse centroids and every added
// row's list id and payload (PQ codes, f32 / f16 elements, SQ codes or packed BQ words) in add order.  The device state -- a flat index
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

// ------------------------------------------------------------------ inverted-file flat and scalar (k_ivfflat.hip, k_ivfsq.hip) ----
// The two indexes of exact distances: the payload is the rows themselves (f32 or f16 elements) or their SQ codes (dim
// bytes), with the rows' norms under the cosines.  They differ in the norms kernel and the distance launcher.
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

// ---------------------------------------------------------------------------- TSVQ ----
int vqhip_tsvq_build(const vqhip_dataset *ds, uint32_t max_depth, uint32_t cap, float *centroids, int32_t *left,
                     int32_t *right, int32_t *n_nodes) {
    VQ_API_BEGIN
    if (!ds || !centroids || !left || !right || !n_nodes) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    return tsvq_build_device(ds->X, ds->n, ds->d, max_depth, cap, centroids, left, right, n_nodes, s, ds->own.p ? &ds->tsvq_policy : nullptr);
    VQ_API_END
}

int vqhip_tsvq_create(const float *centroids, const int32_t *left, const int32_t *right, uint32_t n_nodes, uint32_t d,
                      int metric, vqhip_tsvq **out) {
    VQ_API_BEGIN
    if (!out) return fail(VQHIP_ERR_NULL_PTR, "out is NULL");
    *out = nullptr;
    if (!centroids || !left || !right) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    if (n_nodes == 0 || d == 0) return fail(VQHIP_ERR_INVALID_INPUT, "empty tree");
    if (metric < VQHIP_SQUARED_EUCLIDEAN || metric > VQHIP_COSINE_UNCLAMPED) return fail(VQHIP_ERR_INVALID_INPUT, "unknown metric %d", metric);
    {
        // the arrays must describe ONE tree rooted at node 0: children point forward (pre-order, so the
        // descent terminates), a node's two children differ, no node has two parents and every node but
        // the root has one (the encoder's breadth-first images are sized by the node count)
        std::vector<uint8_t> has_parent(n_nodes, 0);
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const int32_t ch[2] = {left[i], right[i]};
            if (ch[0] >= 0 && ch[0] == ch[1]) return fail(VQHIP_ERR_INVALID_INPUT, "node %u names node %d as both children", i, ch[0]);
            for (int c = 0; c < 2; ++c) {
                if (ch[c] < 0) continue;
                if (ch[c] <= (int32_t)i || ch[c] >= (int32_t)n_nodes)
                    return fail(VQHIP_ERR_INVALID_INPUT, "node %u has an out-of-order child index", i);
                if (has_parent[ch[c]]) return fail(VQHIP_ERR_INVALID_INPUT, "node %d has two parents", ch[c]);
                has_parent[ch[c]] = 1;
            }
        }
        for (uint32_t i = 1; i < n_nodes; ++i)
            if (!has_parent[i]) return fail(VQHIP_ERR_INVALID_INPUT, "node %u is not reachable from the root", i);
    }
    VQ_TRY(require_gfx950());
    hipStream_t s;
    VQ_TRY(current_stream(&s));
    std::unique_ptr<vqhip_tsvq> t(new vqhip_tsvq());
    t->n_nodes = n_nodes;
    t->d = d;
    t->metric = metric;
    VQ_TRY(t->centroids.alloc((size_t)n_nodes * d * 4));
    VQ_TRY(t->left.alloc((size_t)n_nodes * 4));
    VQ_TRY(t->right.alloc((size_t)n_nodes * 4));
    VQ_HIP(hipMemcpyAsync(t->centroids.p, centroids, (size_t)n_nodes * d * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipMemcpyAsync(t->left.p, left, (size_t)n_nodes * 4, hipMemcpyHostToDevice, s));
    VQ_HIP(hipMemcpyAsync(t->right.p, right, (size_t)n_nodes * 4, hipMemcpyHostToDevice, s));
    VQ_TRY(t->cnorm.alloc((size_t)n_nodes * 4));
    VQ_TRY(launch_tsvq_node_norms(t->centroids.as<float>(), n_nodes, d, t->cnorm.as<float>(), s));
    VQ_TRY(t->table16.alloc((size_t)n_nodes * d * 2));
    VQ_TRY(launch_tsvq_table_f16(t->centroids.as<float>(), n_nodes, d, t->table16.as<uint16_t>(), s));
    VQ_TRY(tsvq_prepare_screen(t.get(), centroids, left, right, s));
    VQ_HIP(hipStreamSynchronize(s));
    *out = t.release();
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_tsvq_destroy(vqhip_tsvq *t) {
    delete t;
    return VQHIP_OK;
}

int vqhip_tsvq_encode_device(vqhip_tsvq *t, const void *dev_rows, uint64_t n, void *dev_leaf, void *dev_f16_out) {
    VQ_API_BEGIN
    if (!t) return fail(VQHIP_ERR_NULL_PTR, "tree is NULL");
    if (n == 0) return VQHIP_OK;
    if (!dev_rows) return fail(VQHIP_ERR_NULL_PTR, "dev_rows is NULL");
    VQ_TRY(require_gfx950());
    Entry in(t->sync);
    hipStream_t s;
    VQ_TRY(in.stream(&s));
    int32_t *leaf = reinterpret_cast<int32_t *>(dev_leaf);
    if (!leaf) {
        VQ_TRY(t->leafbuf.ensure((size_t)n * 4));
        leaf = t->leafbuf.as<int32_t>();
    }
    t->last_screened = false;
    const float *X = reinterpret_cast<const float *>(dev_rows);
    uint16_t *out = reinterpret_cast<uint16_t *>(dev_f16_out);
    const bool out_vec = out && t->d % 8 == 0 && (reinterpret_cast<uintptr_t>(dev_f16_out) & 15) == 0;
    bool out_done = false;
    if (t->use_screen && n <= 0xFFFFFFFFull && (reinterpret_cast<uintptr_t>(dev_rows) & 15) == 0) {
        t->last_screened = true;
        VQ_TRY(t->scr_wl.ensure((size_t)n * 8));
        t->scr.wl = t->scr_wl.as<uint2>();
        // the reconstruction rides on the descent when it can be written in 16-byte pieces
        VQ_TRY(launch_tsvq_screen_encode(X, n, t->d, t->centroids.as<float>(), t->cnorm.as<float>(), t->left.as<int32_t>(),
                                         t->right.as<int32_t>(), t->metric, t->scr, leaf, s,
                                         out_vec ? t->table16.as<uint16_t>() : nullptr, out_vec ? out : nullptr));
        out_done = out_vec;
    } else {
        VQ_TRY(launch_tsvq_encode(X, n, t->d, t->centroids.as<float>(), t->cnorm.as<float>(), t->left.as<int32_t>(),
                                  t->right.as<int32_t>(), t->metric, leaf, s));
    }
    if (out && !out_done) {
        if (out_vec)
            VQ_TRY(launch_tsvq_gather_table(t->table16.as<uint16_t>(), t->d, leaf, n, out, s));
        else
            VQ_TRY(launch_tsvq_gather_f16(t->centroids.as<float>(), t->d, leaf, n, out, s));
    }
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_tsvq_last_stats(vqhip_tsvq *t, int *screened, uint64_t *undecided) {
    VQ_API_BEGIN
    if (!t || !screened || !undecided) return fail(VQHIP_ERR_NULL_PTR, "NULL argument");
    Entry in(t->sync);
    *screened = t->last_screened ? 1 : 0;
    *undecided = 0;
    if (t->last_screened) {
        hipStream_t s;
        VQ_TRY(in.stream(&s));
        uint32_t c = 0;
        VQ_HIP(hipMemcpyAsync(&c, t->scr_count.as<uint32_t>() + (t->scr.turn ^ 1u), 4, hipMemcpyDeviceToHost, s));  // the last call's counter
        VQ_HIP(hipStreamSynchronize(s));
        in.synced();
        *undecided = c;
    }
    return VQHIP_OK;
    VQ_API_END
}

int vqhip_tsvq_encode(vqhip_tsvq *t, const float *rows, uint64_t n, int32_t *leaf, uint16_t *f16_out) {
    VQ_API_BEGIN
    if (!t) return fail(VQHIP_ERR_NULL_PTR, "tree is NULL");
    if (n == 0) return VQHIP_OK;
    if (!rows) return fail(VQHIP_ERR_NULL_PTR, "rows is NULL");
    VQ_TRY(require_gfx950());
    Entry in(t->sync);
    const uint32_t d = t->d;
    // per-vector calls: the kernel reads the tree only (fixed at creation, complete before the handle existed) and
    // stages through a buffer of its own, so the handle is given back before the launch (see vqhip_pq_encode)
    const bool small = n <= kSmallRows && tsvq_small_supported(d);
    if (small) t->last_screened = false;
    auto small_launch = [&](const void *di, uint64_t nr, void *dl, void *df, hipStream_t s) {
        return launch_tsvq_encode_small(static_cast<const float *>(di), (uint32_t)nr, d, t->metric, t->centroids.as<float>(),
                                        t->cnorm.as<float>(), t->left.as<int32_t>(), t->right.as<int32_t>(),
                                        static_cast<int32_t *>(dl), static_cast<uint16_t *>(df), s);
    };
    auto chunk_launch = [t](const void *di, uint64_t nr, void *dl, void *df, hipStream_t) {
        return vqhip_tsvq_encode_device(t, di, nr, dl, df);
    };
    return host_batch(HostBatch{rows, (size_t)d * 4, leaf, 4, f16_out, (size_t)d * 2, n, 1}, &in, small, small_launch,
                      chunk_launch, t->xbuf, t->leafbuf, t->f16buf);
    VQ_API_END
}

}  // extern "C"
