// fir_kernel_launch.h -- what the launchers of the periodic kernels (fir_periodic.hip, fir_split.hip) share: the CU count
// of a device, the grant of dynamic LDS to a kernel, the debug word, the buffers of the diagnostic traces.  HIP runtime
// API, no kernels (fir_kernel_launch.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

namespace rsmp {

// Compute units of `device` (asked once per device; 256 if the runtime does not say).
uint32_t device_cus(int device);

// Dynamic LDS above 64 KiB must be opted into, once per kernel and device.
hipError_t grant_dynamic_lds(int device, const void* fn, uint32_t bytes);

// RSMP_FIR_DEBUG: the kernels' debug word (bit0 skip staging, bit1 skip the tap loops ...: timing only).
uint32_t fir_debug_knob();

// A diagnostic trace of one launch (RSMP_FIR_TRACE, RSMP_FIR_WTRACE): `words` 64-bit words on the device, the buffer of
// the previous launch given back.  The caller zeroes it, hands it to the kernel, and afterwards has its lines written:
// trace_dump waits for `stream`, fetches the words and calls write(file, words) on the opened file.
struct TraceBuffer {
    unsigned long long* d = nullptr;
    size_t words = 0;
    hipError_t renew(size_t n_words);
    template <class Write>
    void dump(const char* path, hipStream_t stream, Write write) const {
        (void)hipStreamSynchronize(stream);
        std::vector<unsigned long long> h(words);
        (void)hipMemcpy(h.data(), d, words * 8, hipMemcpyDeviceToHost);
        if (FILE* f = fopen(path, "w")) {
            write(f, h);
            fclose(f);
        }
    }
};

}  // namespace rsmp
