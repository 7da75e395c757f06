// fir_periodic_plan.h -- what the host planner (fir_hostplan.cpp) asks about the periodic kernels: no HIP header.
// Defined beside the kernels they describe, in fir_periodic.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fir_plan.h"

namespace rsmp {

bool periodic_supported(const FirMirror& m, size_t channels, size_t taps, int kernel_mode);
bool periodic_worthwhile(const FirMirror& planned, size_t produced_frames, int kernel_mode);

// Bitmap of wrapped outputs for one launch: bit K <-> the output with absolute index
// (abs_out / den + K) * den.  Returns the number of 32-bit words.
size_t periodic_wrap_words(uint64_t abs_out, uint32_t n_out, uint64_t den);
void periodic_fill_wrap_bits(const std::vector<uint32_t>& wraps, uint64_t abs_out, uint64_t den,
                             uint32_t* words, size_t n_words);

}  // namespace rsmp
