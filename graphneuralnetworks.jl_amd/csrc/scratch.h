// scratch.h — the one scoped owner of device scratch on the host set-up path (plan builds, graph prep, link prediction, neighbour
// search).  A DevBuf gives its bytes back when it leaves scope, so every error exit of its function is a plain `return`.
// Two sources, chosen at construction:
//   Scratch::Malloc     hipMalloc / hipFree.  hipFree waits for the device, so a buffer may die while work that uses it is still queued.
//   Scratch::PrepCache  the per-thread cache of the per-mini-batch entry points below.  A parked block is handed out again WITHOUT a wait,
//                       so a buffer is parked only after synced() — the mark its owner sets once hipStreamSynchronize has succeeded
//                       behind the last work that touches it.  Unmarked (an error exit before the synchronisation) it is hipFree'd.
// The pool of pool.h keeps its explicit take / park: those blocks outlive the call that takes them.
// Plain C++ under g++ too: tests/c_harness/scratch_check.cpp defines GNNMP_SCRATCH_STANDIN and supplies counting stand-ins for
// hipError_t, dev_malloc, dev_free, current_device and hip_fail before it includes this file.
#pragma once
#include <stddef.h>
#include <algorithm>
#include "gnnmp.h"

#ifndef GNNMP_SCRATCH_STANDIN
#include "common.h"
namespace gnnmp {
inline hipError_t dev_malloc(void **out, size_t bytes) { return hipMalloc(out, bytes); }
inline hipError_t dev_free(void *p) { return hipFree(p); }
}  // namespace gnnmp
#endif

#pragma GCC visibility push(hidden)   // host helpers of the library, not part of its export list
namespace gnnmp {

// Scratch for the per-mini-batch entry points (sample_neighbors, unique_append, induced_subgraph): hipMalloc / hipFree cost
// ~0.1-1 ms each and a NeighborLoader batch made ~50 of them.  Freed blocks are parked in a small per-thread cache and
// handed out again (only blocks whose owner synchronised its stream are parked — DevBuf::synced — so a parked block is idle).
// A block is only handed out on the device it was allocated on (dev = common.h's current_device at allocation; alloc and free of one
// entry point run under the same current device).
struct PrepBlock { void *p; size_t cap; int dev; };
inline thread_local PrepBlock g_prep_cache[8] = {};
inline hipError_t prep_alloc(void **out, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    const int dev = current_device();
    int best = -1;
    for (int i = 0; i < 8; ++i)
        if (g_prep_cache[i].p && g_prep_cache[i].dev == dev && g_prep_cache[i].cap >= bytes &&
            (best < 0 || g_prep_cache[i].cap < g_prep_cache[best].cap))
            best = i;
    if (best >= 0 && g_prep_cache[best].cap <= 4 * bytes + (1 << 20)) {
        *out = g_prep_cache[best].p;
        g_prep_cache[best] = PrepBlock{nullptr, 0, 0};
        return hipSuccess;
    }
    return dev_malloc(out, bytes);
}
inline void prep_free(void *p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    const int dev = current_device();
    int slot = -1;
    for (int i = 0; i < 8; ++i)
        if (!g_prep_cache[i].p) { slot = i; break; }
    if (slot < 0) {   // cache full: evict the smallest block
        slot = 0;
        for (int i = 1; i < 8; ++i)
            if (g_prep_cache[i].cap < g_prep_cache[slot].cap) slot = i;
        if (g_prep_cache[slot].cap >= bytes) {
            (void)dev_free(p);
            return;
        }
        (void)dev_free(g_prep_cache[slot].p);
    }
    g_prep_cache[slot] = PrepBlock{p, bytes, dev};
}

enum class Scratch { Malloc, PrepCache };

template <class T>
class DevBuf {
public:
    explicit DevBuf(Scratch src = Scratch::Malloc) : src_(src) {}
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_), src_(o.src_), synced_(o.synced_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            give_back();
            p_ = o.p_;
            bytes_ = o.bytes_;
            src_ = o.src_;
            synced_ = o.synced_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { give_back(); }
    // n elements (whatever the buffer held before goes back first); on failure the buffer is empty
    hipError_t alloc(size_t n) {
        give_back();
        bytes_ = sizeof(T) * n;
        synced_ = false;
        void *p = nullptr;
        const hipError_t e = src_ == Scratch::PrepCache ? prep_alloc(&p, bytes_) : dev_malloc(&p, bytes_);
        if (e == hipSuccess) p_ = static_cast<T *>(p);
        return e;
    }
    T *get() const { return p_; }
    // ownership to the caller (a plan member, say): whoever holds the pointer now dev_free's it
    T *release() {
        T *p = p_;
        p_ = nullptr;
        return p;
    }
    // the stream was synchronised behind the last work that touches the buffer: a PrepCache buffer may be parked
    void synced() { synced_ = true; }

private:
    void give_back() {
        if (!p_) return;
        if (src_ == Scratch::PrepCache && synced_)
            prep_free(p_, bytes_);
        else
            (void)dev_free(p_);   // (waits for the device: safe whatever still uses the block)
        p_ = nullptr;
    }
    T *p_ = nullptr;
    size_t bytes_ = 0;
    Scratch src_;
    bool synced_ = false;
};

// n elements straight into an owner's member (the plan's arrays: gnnmp_plan_destroy frees them)
template <class T>
inline hipError_t alloc_into(T *&member, size_t n) {
    DevBuf<T> b;
    const hipError_t e = b.alloc(n);
    member = b.release();
    return e;
}

// Grow-only member of a long-lived owner (the plan's workspaces): make sure `ptr` holds at least `need` elements.  Nothing is carried
// over; hipFree waits for work that may still read the old buffer.  After a failed allocation the member is empty (nullptr, 0).
template <class T>
inline int grow(T *&ptr, size_t &cap, size_t need, const char *what) {
    if (need <= cap) return GNNMP_OK;
    if (ptr) (void)dev_free(ptr);
    ptr = nullptr;
    cap = 0;
    const hipError_t e = alloc_into(ptr, need);
    if (e != hipSuccess) return hip_fail(e, what);
    cap = need;
    return GNNMP_OK;
}

}  // namespace gnnmp
#pragma GCC visibility pop
