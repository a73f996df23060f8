// runtime.hip — the library's process-wide plumbing: the error string, the tuning knobs (knobs.h), the current device and its
// compute-unit count, the environment switch that is read once, and the version / tune / debug exports.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>

#include "common.h"
#include "pool.h"

namespace gnnmp {

static thread_local char g_err[512] = "";
// the table of knobs.h as arrays; its entries are in index order (checked below), so entry i is knob i
#define GNNMP_KNOB_INDEX(name, index, def, doc) index,
#define GNNMP_KNOB_DEFAULT(name, index, def, doc) def,
#define GNNMP_KNOB_NAME(name, index, def, doc) #name,
static constexpr int g_knob_index[KNOB_COUNT] = {GNNMP_KNOB_TABLE(GNNMP_KNOB_INDEX)};
static constexpr int g_knob_defaults[KNOB_COUNT] = {GNNMP_KNOB_TABLE(GNNMP_KNOB_DEFAULT)};
[[maybe_unused]] static const char *const g_knob_names[KNOB_COUNT] = {GNNMP_KNOB_TABLE(GNNMP_KNOB_NAME)};
static int g_knobs[KNOB_COUNT] = {GNNMP_KNOB_TABLE(GNNMP_KNOB_DEFAULT)};
#undef GNNMP_KNOB_INDEX
#undef GNNMP_KNOB_DEFAULT
#undef GNNMP_KNOB_NAME
constexpr bool knob_table_is_dense() {
    for (int i = 0; i < KNOB_COUNT; ++i)
        if (g_knob_index[i] != i) return false;
    return true;
}
static_assert(knob_table_is_dense(), "knobs.h: the X(...) entries must be listed in index order, 0 .. KNOB_COUNT - 1, without gaps");

int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return status;
}
int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    return e == hipErrorOutOfMemory ? GNNMP_EALLOC : GNNMP_ELAUNCH;
}
int knob(int k) { return (k >= 0 && k < KNOB_COUNT) ? g_knobs[k] : 0; }
static thread_local int g_mock_device = -1;
int current_device() {
    if (g_mock_device >= 0) return g_mock_device < GNNMP_MAX_DEVICES ? g_mock_device : GNNMP_MAX_DEVICES - 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev < GNNMP_MAX_DEVICES ? dev : GNNMP_MAX_DEVICES - 1;
}
int device_cus() {
    static std::atomic<int> cached[GNNMP_MAX_DEVICES] = {};
    const int dev = current_device();
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        cus = 256;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

bool fold_disabled_by_env() {
    static const bool off = [] {
        const char *e = getenv("GNNMP_NO_FOLD");
        return e && *e && *e != '0';
    }();
    return off;
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_version(void) { return GNNMP_VERSION; }
const char *gnnmp_last_error(void) { return g_err; }

// perf-experiment hooks over the table of knobs.h (not part of the drop-in surface)
int gnnmp_tune(int k, int value) {
    if (k < 0 || k >= KNOB_COUNT) return fail(GNNMP_EINVAL, "gnnmp_tune: bad knob %d", k);
#ifndef GNNMP_EXPERIMENTS
    if (k == KNOB_T16_DEBUG && value != 0)
        return fail(GNNMP_EUNSUPPORTED, "gnnmp_tune: knob %d (%s) selects experiment code that this build does not contain; build the library with "
                                        "-DGNNMP_EXPERIMENTS (make EXPERIMENTS=1)", k, g_knob_names[k]);
#endif
    g_knobs[k] = value;
    return GNNMP_OK;
}
int gnnmp_tune_get(int k, int *value, int *default_value) {
    if (k < 0 || k >= KNOB_COUNT) return fail(GNNMP_EINVAL, "gnnmp_tune_get: bad knob %d", k);
    if (value) *value = g_knobs[k];
    if (default_value) *default_value = g_knob_defaults[k];
    return GNNMP_OK;
}

// test hooks (like gnnmp_tune: exported, not part of the drop-in surface).  gnnmp_debug_mock_device(d >= 0) makes `d` the calling
// thread's "current device" for every per-device table of the library (common.h: current_device), d < 0 restores hipGetDevice.
int gnnmp_debug_mock_device(int dev) {
    g_mock_device = dev;
    return current_device();
}
// Runs the per-device machinery with a counting stand-in for hipFuncSetAttribute and returns how often it ran: the sequence of mocked
// devices devs[0..n) must run it once per DISTINCT device (tests/test_multi_device_cpu.py).  fail_on >= 0: the stand-in fails on that
// device; *n_failed = calls that reported the failure (every call on that device must, not only the first).
int gnnmp_debug_device_once(const int *devs, int n, int fail_on, int *n_failed) {
    DeviceOnce once;
    int ran = 0, failed = 0;
    const int keep = g_mock_device;
    for (int k = 0; k < n; ++k) {
        g_mock_device = devs[k];
        const hipError_t e = device_once(once, [&] {
            ++ran;
            return current_device() == fail_on ? hipErrorInvalidValue : hipSuccess;
        });
        if (e != hipSuccess) ++failed;
    }
    g_mock_device = keep;
    if (n_failed) *n_failed = failed;
    return ran;
}
// the pooled block of a plan made by gnnmp_plan_concat / gnnmp_plan_select (NULL for other plans): lets a test see WHICH block a plan got
void *gnnmp_debug_plan_block(const gnnmp_graph_t *p) { return p ? p->block : nullptr; }
// pool.h's slot choice on host arrays
int gnnmp_debug_pool_pick(const uint64_t *caps, int n, uint64_t bytes) {
    size_t c[64];
    if (n < 0 || n > 64) return -2;
    for (int i = 0; i < n; ++i) c[i] = (size_t)caps[i];
    return pool_pick(c, n, (size_t)bytes);
}

}  // extern "C"
