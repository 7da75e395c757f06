// pcm_batch_plan.cpp -- the host half of the batched PCM converters' plan (pcm_batch_plan.h): the prefix of tile counts.
#include "pcm_batch_plan.h"

namespace rsmp {

bool pcm_batch_prefix(const uint64_t* n_values, size_t n, uint32_t* prefix) {
    uint64_t total = 0;
    for (size_t s = 0; s < n; ++s) {
        prefix[s] = static_cast<uint32_t>(total);
        const uint64_t t = pcm_batch_stream_tiles(n_values[s]);
        if (t > 0xFFFFFFFFull || total + t > 0xFFFFFFFFull) return false;
        total += t;
    }
    prefix[n] = static_cast<uint32_t>(total);
    return true;
}

}  // namespace rsmp
