// Library-wide host runtime: thread-local error string, tuning knobs, device probe.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ss_common.h"

namespace ss {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return SS_OK;
    set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    return SS_EHIP;
}

std::atomic<int> g_knobs[K_COUNT] = {
#define X(name, dflt, doc) {dflt},
    SS_KNOB_LIST(X)
#undef X
};

// the only lookup by name: the two C entry points below
static int knob_find(const char* key) {
    for (int k = 0; key && k < K_COUNT; ++k)
        if (!strcmp(kKnobs[k].name, key)) return k;
    return -1;
}

}  // namespace ss

extern "C" {

const char* ss_last_error(void) { return ss::g_err; }
int ss_abi_version(void) { return SS_ABI_VERSION; }

int ss_set_tuning(const char* key, int value) {
    const int k = ss::knob_find(key);
    SS_REQUIRE(k >= 0, "ss_set_tuning: unknown tuning key '%s' (the list is csrc/ss_knobs.h)", key ? key : "(null)");
    ss::g_knobs[k].store(value, std::memory_order_relaxed);
    return SS_OK;
}
int ss_get_tuning(const char* key, int dflt) {
    const int k = ss::knob_find(key);
    return k < 0 ? dflt : ss::knob_or((ss::Knob)k, dflt);
}

int ss_device_info(int32_t out[4]) {
    int dev = 0;
    SS_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    SS_HIP(hipGetDeviceProperties(&p, dev));
    out[0] = p.multiProcessorCount;
    out[1] = strstr(p.gcnArchName, "gfx950") != nullptr;
    out[2] = (int32_t)(p.totalGlobalMem >> 20);
    out[3] = p.warpSize;
    return SS_OK;
}

}  // extern "C"
