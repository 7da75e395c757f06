// fir_kernel_launch.cpp -- see fir_kernel_launch.h.  HIP runtime API, no kernels.
#include "fir_kernel_launch.h"

#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "errors.h"

namespace rsmp {

uint32_t device_cus(int device) {
    static std::mutex mu;
    static std::map<int, uint32_t> count;
    std::lock_guard<std::mutex> lock(mu);
    uint32_t& c = count[device];
    if (c == 0) {
        int v = 0;
        (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device);
        c = static_cast<uint32_t>(v > 0 ? v : 256);
    }
    return c;
}

hipError_t grant_dynamic_lds(int device, const void* fn, uint32_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, bool> granted;
    std::lock_guard<std::mutex> lock(mu);
    bool& have = granted[{device, fn}];
    if (!have) {
        if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)); e != hipSuccess) return e;
        have = true;
    }
    return hipSuccess;
}

uint32_t fir_debug_knob() {
    static const uint32_t debug = [] {
        const char* e = rsmp::knob("RSMP_FIR_DEBUG");
        return e ? static_cast<uint32_t>(atoi(e)) : 0u;
    }();
    return debug;
}

hipError_t TraceBuffer::renew(size_t n_words) {
    if (d) (void)hipFree(d);
    d = nullptr;
    words = n_words;
    return hipMalloc(&d, n_words * 8) == hipSuccess ? hipSuccess : hipErrorOutOfMemory;
}

}  // namespace rsmp
