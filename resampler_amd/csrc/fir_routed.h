// fir_routed.h -- bulk batches in many different states, planned on the device behind the host entry (fir_routed.cpp).
#pragma once

#include <cstddef>

struct rsmp_fir;

namespace rsmp {

// The launch through the device planner, if the batch is one for it.  *took = 1: done (rc is the call's result); *took = 0: not
// one for it -- the host planner's, and no error of this call's has been set.
int batch_bulk_routed(rsmp_fir* const* rs, size_t n, const float* const* d_in, const size_t* in_lens, size_t chunk_len,
                      float* const* d_out, const size_t* out_caps, size_t* consumed, size_t* produced, void* stream, int planner, int* took);

// Throws away (without a write-back) every cached batch that lists `r`: the handle is about to be destroyed.
void routed_forget(const rsmp_fir* r);

}  // namespace rsmp
