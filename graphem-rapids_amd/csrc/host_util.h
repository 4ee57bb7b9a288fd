// Host plumbing shared by every handle behind the C ABI, the layout engine included: the HIP-call checks, gh_dev -- a device
// allocation that frees itself, the type of every buffer a handle owns -- with the process-wide count of the live ones, the
// life cycle of an analysis handle (device, stream, budget, message), the canonical edge set and its CSR (csr_build.h),
// and the level loop of a breadth-first pass.  No kernel and no policy lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "csr_build.h"   // gh_canonical_edge_keys and the CSR builder: host-only code, kept where a host compiler reads it alone

// The checks need a handle `h` in scope whose `err` takes the message "<call>: <hip error string>".
#define GH_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            h->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return GH_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

#define GH_TRY_ST(x)                                                                        \
    do {                                                                                    \
        gh_status st_ = (x);                                                                \
        if (st_ != GH_OK) return st_;                                                       \
    } while (0)

#define GH_LAUNCH_CHECK()                                                                   \
    do {                                                                                    \
        hipError_t e_ = hipGetLastError();                                                  \
        if (e_ != hipSuccess) {                                                             \
            h->err = std::string("kernel launch: ") + hipGetErrorString(e_);                \
            return GH_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

// Live gh_dev allocations of the process and their bytes (gh_debug_live_allocations): what a test of the handles' life
// cycles reads, since the card's free memory also moves with other processes.
inline std::atomic<int64_t> gh_live_count{0}, gh_live_bytes{0};

// A device allocation that frees itself.  Never smaller than 16 bytes, so an empty array still has an address to hand
// to a kernel.  Moving it, also to a buffer of another element type, hands the allocation over (and counts it once).
// No conversion to T *: a member of this type owns its memory, a raw pointer is a view of somebody else's.
template <class T> struct gh_dev {
    T *p = nullptr;
    size_t bytes = 0;   // as allocated
    gh_dev() = default;
    gh_dev(const gh_dev &) = delete;
    gh_dev &operator=(const gh_dev &) = delete;
    template <class U> gh_dev(gh_dev<U> &&o) noexcept { take(o); }
    template <class U> gh_dev &operator=(gh_dev<U> &&o) noexcept { take(o); return *this; }
    ~gh_dev() { reset(); }
    void reset() {
        if (p) { (void)hipFree(p); gh_live_count -= 1; gh_live_bytes -= (int64_t)bytes; }
        p = nullptr;
        bytes = 0;
    }
    bool alloc(size_t want) {
        reset();
        want = std::max<size_t>(want, 16);
        if (hipMalloc((void **)&p, want) != hipSuccess) { p = nullptr; return false; }
        bytes = want;
        gh_live_count += 1;
        gh_live_bytes += (int64_t)bytes;
        return true;
    }
    template <class U> U *as() const { return (U *)p; }

private:
    template <class U> void take(gh_dev<U> &o) {
        T *q = (T *)o.p;
        const size_t b = o.bytes;
        o.p = nullptr;
        o.bytes = 0;
        reset();
        p = q;
        bytes = b;
    }
};

// What every analysis handle (gh_ic, gh_cent, gh_gen, gh_corr) starts with.  device < 0: a host-path handle without a stream.
struct gh_host {
    int device = -1;
    hipStream_t stream = nullptr;
    int64_t budget = 0;
    std::string err;
};

// Selects the device and creates the handle's stream; a failure leaves its message in *msg (the module's create-time text).
inline gh_status gh_host_open(gh_host *h, int device_id, std::string *msg) {
    if (hipSetDevice(device_id) != hipSuccess) {
        (void)hipGetLastError();   // reported here; left in the thread it would fail the next HIP user's check (torch's)
        *msg = "invalid device ordinal " + std::to_string(device_id);
        return GH_ERR_RUNTIME;
    }
    h->device = device_id;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { *msg = "hipStreamCreate failed"; return GH_ERR_HIP; }
    return GH_OK;
}

// Waits for the handle's work and destroys its stream; the handle's gh_dev members free themselves when it is deleted.
inline void gh_host_close(gh_host *h) {
    if (h->device < 0) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    h->stream = nullptr;
}

// gh_*_set_memory_budget: 0 means `dflt`; *null_msg is the module's create-time text.
inline gh_status gh_host_set_budget(gh_host *h, int64_t bytes, int64_t dflt, std::string *null_msg) {
    if (!h) { *null_msg = "handle is NULL"; return GH_ERR_INVALID; }
    if (bytes < 0) { h->err = "budget must be >= 0 (0: the default)"; return GH_ERR_INVALID; }
    h->budget = bytes ? bytes : dflt;
    return GH_OK;
}

// The host loop of a breadth-first pass whose level kernel sets d_flags[L] when level L reached something (d_flags[0] is
// preset).  launch(L) enqueues level L = 1, 2, ..; a level can reach something only while L <= n - 1.  Every `every` levels
// the new flags are read back, and the loop ends at the first empty one.  *last = the last level that reached something.
template <class Launch>
gh_status gh_level_loop(gh_host *h, int64_t n, const int32_t *d_flags, int every, int32_t *last, Launch launch) {
    *last = 0;
    std::vector<int32_t> fl((size_t)every);
    for (int64_t L = 1, checked = 0; L <= n - 1; ++L) {
        GH_TRY_ST(launch((int32_t)L));
        if (L % every != 0 && L != n - 1) continue;
        const int64_t cnt = L - checked;
        GH_HIP(hipMemcpyAsync(fl.data(), d_flags + checked + 1, 4 * cnt, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        for (int64_t i = 0; i < cnt; ++i) {
            if (!fl[i]) return GH_OK;
            *last = (int32_t)(checked + 1 + i);
        }
        checked = L;
    }
    return GH_OK;
}
