// api_common.hpp -- what every file of extern "C" entry points needs (api.hip, api_resident.hip, api_ivf.hip): the
// per-handle lock and stream order, the exception fence of an entry point, and the two helpers of api.hip that the
// index files call.  Internal to the library, like common.hpp.
#pragma once
#include <memory>
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
//     A call whose last stream operation is a kernel records nothing: that kernel carries a pooled event as the stop
//     event of its own dispatch (LaunchStage, kernels.hpp) and hands it over with `cover`.  Such an event completes
//     with the kernel and outlives the stream like a recorded one, and it puts no marker behind the kernel.

// Events for the dispatches of kernels (stage times, a call's last kernel).  One free list per device for the whole
// process: an event goes back to it when its last holder lets go, on whichever thread that is, so no call creates or
// destroys an event once the lists are warm.
struct PooledEvent {
    hipEvent_t e = nullptr;
    int device = 0;
};
using EventRef = std::shared_ptr<PooledEvent>;
int pooled_event(EventRef *out);   // defined in api.hip
uint64_t pooled_event_count();     // events the pool has created and not destroyed

struct HandleSync {
    std::recursive_mutex mu;
    hipEvent_t ev = nullptr;
    EventRef kev;                // stop event of the last kernel of the call that left the tail, when tail_kernel
    hipStream_t tail = nullptr;  // stream holding queued work of this handle (nullptr: the last call synchronised)
    bool tail_lazy = false;      // the event for `tail` has not been recorded yet (library-owned stream)
    bool tail_kernel = false;    // the tail's event is `kev`
    bool covered = false;        // this call's last stream operation is a kernel that carries `kev`
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
            if (tail_kernel) {
                VQ_HIP(hipStreamWaitEvent(s, kev->e, 0));
            } else {
                VQ_TRY(event());
                if (tail_lazy) VQ_HIP(hipEventRecord(ev, tail));
                VQ_HIP(hipStreamWaitEvent(s, ev, 0));
            }
            tail = nullptr;
        }
        return VQHIP_OK;
    }
    // True for the outermost call of a handle: only its last kernel can be the last operation of the call.
    bool may_cover() const { return depth == 1; }
    // `e` is the stop event of the kernel just launched, and the call queues nothing behind that kernel
    void cover(const EventRef &e) {
        kev = e;
        covered = true;
    }
    void leave(hipStream_t s, bool synced) {
        const bool by_kernel = covered;
        covered = false;
        if (synced || !s) {
            if (synced) tail = nullptr;
            return;
        }
        tail = s;
        tail_kernel = by_kernel;
        tail_lazy = !by_kernel;
        if (!by_kernel && tls().user_stream_set && tls().user_stream == s) {
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
    HandleSync &handle() { return *h_; }
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
