// api_common.hpp -- what every file of extern "C" entry points needs (api.hip, api_resident.hip, api_ivf.hip): the
// per-handle lock and stream order, the exception fence of an entry point, and the two helpers of api.hip that the
// index files call.  Internal to the library, like common.hpp.
#pragma once
#include <mutex>
#include <new>

#include "kernels.hpp"

namespace vqhip {

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

// defined in api.hip
int check_codes(const uint8_t *codes, uint64_t count, uint32_t k);
int sqbq_encode_host(const SqbqEncodeOp &op, const float *x, uint64_t count, uint8_t *codes);

}  // namespace vqhip

#define VQ_API_BEGIN try {
#define VQ_API_END                                                                  \
    }                                                                               \
    catch (const std::bad_alloc &) { return fail(VQHIP_ERR_FAILURE, "host allocation failed"); } \
    catch (...) { return fail(VQHIP_ERR_FAILURE, "unexpected C++ exception"); }
