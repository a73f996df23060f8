// scratch_check.cpp — CPU check of csrc/scratch.h (DevBuf, the prep cache, alloc_into, grow): the SAME header the library compiles, under
// plain g++ with counting stand-ins for the device calls.  Every check prints its name; the first failing one ends the run with status 1.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <utility>
#include <vector>

// ---- the stand-ins scratch.h asks for under GNNMP_SCRATCH_STANDIN ---------------------------------------------------------------------------
namespace gnnmp {
typedef int hipError_t;
const hipError_t hipSuccess = 0;
const hipError_t hipErrorOutOfMemory = 2;
static std::vector<std::string> g_log;     // "malloc" / "free" in call order
static std::vector<void *> g_live;         // blocks handed out and not given back
static int g_mallocs = 0, g_frees = 0, g_double_frees = 0, g_fail_next = 0, g_device = 0;
static std::string g_what;
inline hipError_t dev_malloc(void **out, size_t bytes) {
    g_log.push_back("malloc");
    if (g_fail_next) {
        g_fail_next = 0;
        *out = reinterpret_cast<void *>(0xdead);   // a failed hipMalloc promises nothing about *out
        return hipErrorOutOfMemory;
    }
    *out = malloc(bytes ? bytes : 1);
    g_live.push_back(*out);
    ++g_mallocs;
    return hipSuccess;
}
inline hipError_t dev_free(void *p) {
    g_log.push_back("free");
    ++g_frees;
    for (size_t i = 0; i < g_live.size(); ++i)
        if (g_live[i] == p) {
            g_live.erase(g_live.begin() + (long)i);
            free(p);
            return hipSuccess;
        }
    ++g_double_frees;                              // not a live block: freed twice, or never allocated
    return 1;
}
inline int current_device() { return g_device; }
inline int hip_fail(hipError_t e, const char *what) {
    g_what = what;
    return e == hipErrorOutOfMemory ? -3 : -4;
}
}  // namespace gnnmp

#define GNNMP_SCRATCH_STANDIN
#include "scratch.h"

using namespace gnnmp;

static int g_checks = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int parked() {
    int n = 0;
    for (int i = 0; i < 8; ++i) n += g_prep_cache[i].p != nullptr;
    return n;
}
static void reset_counts() {
    g_log.clear();
    g_mallocs = g_frees = g_double_frees = 0;
}
static int early_return(bool leave_early) {
    DevBuf<int> a, b;
    if (a.alloc(4) != hipSuccess) return -1;
    if (leave_early) return 1;
    if (b.alloc(4) != hipSuccess) return -1;
    return 0;
}

int main() {
    // -- one give-back per alloc: normal exit, early return, after a move --------------------------------------------------------------------
    {
        DevBuf<double> a;
        CHECK(a.get() == nullptr);
        CHECK(a.alloc(10) == hipSuccess);
        CHECK(a.get() != nullptr && g_mallocs == 1 && g_frees == 0);
    }
    CHECK(g_mallocs == 1 && g_frees == 1 && g_live.empty() && g_double_frees == 0);
    reset_counts();
    CHECK(early_return(true) == 1);
    CHECK(g_mallocs == 1 && g_frees == 1 && g_live.empty());
    CHECK(early_return(false) == 0);
    CHECK(g_mallocs == 3 && g_frees == 3 && g_live.empty() && g_double_frees == 0);
    reset_counts();
    {
        DevBuf<int> a;
        CHECK(a.alloc(3) == hipSuccess);
        int *was = a.get();
        DevBuf<int> b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == was);
        DevBuf<int> c;
        CHECK(c.alloc(5) == hipSuccess);
        c = std::move(b);                          // c's own block goes back here, b's moves in
        CHECK(g_frees == 1 && c.get() == was && b.get() == nullptr);
    }
    CHECK(g_mallocs == 2 && g_frees == 2 && g_live.empty() && g_double_frees == 0);
    reset_counts();
    {   // a second alloc on the same buffer gives the first block back
        DevBuf<int> a;
        CHECK(a.alloc(3) == hipSuccess && a.alloc(7) == hipSuccess);
        CHECK(g_mallocs == 2 && g_frees == 1 && g_live.size() == 1);
    }
    CHECK(g_frees == 2 && g_live.empty());
    printf("ok  give-back on exit, early return, move\n");

    // -- release() suppresses the give-back --------------------------------------------------------------------------------------------------
    reset_counts();
    int *kept = nullptr;
    {
        DevBuf<int> a;
        CHECK(a.alloc(8) == hipSuccess);
        kept = a.release();
        CHECK(kept != nullptr && a.get() == nullptr);
    }
    CHECK(g_mallocs == 1 && g_frees == 0 && g_live.size() == 1);
    CHECK(dev_free(kept) == hipSuccess && g_live.empty());
    reset_counts();
    float *member = nullptr;
    CHECK(alloc_into(member, 16) == hipSuccess && member != nullptr && g_mallocs == 1 && g_frees == 0);
    CHECK(dev_free(member) == hipSuccess);
    g_fail_next = 1;
    member = reinterpret_cast<float *>(0x10);
    CHECK(alloc_into(member, 16) == hipErrorOutOfMemory && member == nullptr);
    printf("ok  release / alloc_into\n");

    // -- a failed alloc leaves the buffer empty, destruction does nothing --------------------------------------------------------------------
    reset_counts();
    {
        DevBuf<int> a;
        g_fail_next = 1;
        CHECK(a.alloc(8) == hipErrorOutOfMemory);
        CHECK(a.get() == nullptr);
    }
    CHECK(g_frees == 0 && g_live.empty());
    {
        DevBuf<int> a(Scratch::PrepCache);
        g_fail_next = 1;
        CHECK(a.alloc(8) == hipErrorOutOfMemory && a.get() == nullptr);
        a.synced();
    }
    CHECK(g_frees == 0 && parked() == 0);
    printf("ok  failed alloc\n");

    // -- the prep cache: freed without synced(), parked with it, the next fitting request gets the same block ----------------------------------
    reset_counts();
    {
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(1000) == hipSuccess);
    }
    CHECK(g_mallocs == 1 && g_frees == 1 && parked() == 0 && g_live.empty());   // no synced(): an error exit before the synchronisation
    void *block = nullptr;
    {
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(1000) == hipSuccess);
        block = a.get();
        a.synced();
    }
    CHECK(g_mallocs == 2 && g_frees == 1 && parked() == 1 && g_live.size() == 1);
    {
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(900) == hipSuccess);                                      // fits the parked block
        CHECK(a.get() == block && g_mallocs == 2 && parked() == 0);
        a.synced();
        CHECK(a.alloc(900) == hipSuccess);                                      // parks the block and takes it again
        CHECK(a.get() == block && g_mallocs == 2 && g_frees == 1 && parked() == 0);
        // an alloc starts unmarked again: without a new synced() the block is freed, not parked
    }
    CHECK(g_frees == 2 && parked() == 0 && g_live.empty());
    {   // a parked block of another device is not handed out
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(1000) == hipSuccess);
        block = a.get();
        a.synced();
    }
    CHECK(parked() == 1);
    g_device = 1;
    {
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(1000) == hipSuccess && a.get() != block && parked() == 1);
    }
    g_device = 0;
    {   // a plain buffer never parks, marked or not
        DevBuf<long> a;
        CHECK(a.alloc(1000) == hipSuccess && a.get() != block);
        a.synced();
    }
    CHECK(parked() == 1);
    {   // drain the cache so that the run ends with nothing live
        DevBuf<long> a(Scratch::PrepCache);
        CHECK(a.alloc(1000) == hipSuccess && a.get() == block);
    }
    CHECK(parked() == 0 && g_live.empty() && g_double_frees == 0);
    printf("ok  prep cache parks only after synced()\n");

    // -- grow ---------------------------------------------------------------------------------------------------------------------------------
    reset_counts();
    float *ws = nullptr;
    size_t cap = 0;
    CHECK(grow(ws, cap, 100, "first") == 0 && ws != nullptr && cap == 100);
    CHECK(g_log == std::vector<std::string>({"malloc"}));                       // nothing to free the first time
    float *old = ws;
    CHECK(grow(ws, cap, 100, "same") == 0 && grow(ws, cap, 40, "smaller") == 0);
    CHECK(ws == old && cap == 100 && g_mallocs == 1 && g_frees == 0);           // need <= cap: the old buffer stays
    g_log.clear();
    CHECK(grow(ws, cap, 101, "larger") == 0 && cap == 101 && ws != nullptr);
    CHECK(g_log == std::vector<std::string>({"free", "malloc"}));               // frees BEFORE it allocates
    CHECK(g_live.size() == 1);
    g_fail_next = 1;
    g_what.clear();
    CHECK(grow(ws, cap, 500, "plan workspace") == -3);
    CHECK(ws == nullptr && cap == 0 && g_live.empty() && g_what == "plan workspace");
    CHECK(grow(ws, cap, 8, "again") == 0 && ws != nullptr && cap == 8);         // and the member recovers
    CHECK(dev_free(ws) == hipSuccess && g_live.empty() && g_double_frees == 0);
    printf("ok  grow\n");

    printf("scratch.h: all %d checks passed\n", g_checks);
    return 0;
}
