// fir_routed.cpp -- see fir_routed.h.
//
// The lock-step batch a routed launch runs on is kept per list of handles, from launch to launch: its plan stream, its class tables and
// the run it plans ahead are what make the second and later launches cheap.  Its states are written back into the handles before a
// routed call returns, so the handles are always current and the batch can be thrown away at any time WITHOUT a write-back
// (rsmp_fir_lockstep_discard) -- which is what happens when a handle has been touched through another entry since, when the cache is
// full, and when one of its handles is destroyed.
#include "fir_routed.h"

#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "fir_handle.h"
#include "fir_launch.h"

namespace rsmp {
namespace {

struct RoutedBatch {
    rsmp_fir_lockstep* ls = nullptr;
    size_t frames = 0;                     // max_step_frames it was made for
    std::vector<const void*> bound;        // d_in / d_out it is bound to
    uint64_t used = 0;
};
using RoutedCache = std::map<std::vector<rsmp_fir*>, RoutedBatch>;
std::mutex& routed_mu() { static std::mutex* m = new std::mutex; return *m; }
RoutedCache& routed_cache() { static auto* c = new RoutedCache; return *c; }
uint64_t routed_clock = 0;
constexpr size_t kRoutedCacheSize = 8;
constexpr size_t kRoutedMinStates = 16;    // fewer different states than this (and than streams): the host's shared plans are cheaper
constexpr size_t kRoutedMaxCallFrames = 2048, kRoutedMinCalls = 8;

bool route_trace() {
    static const bool trace = knob("RSMP_ROUTE_TRACE") != nullptr;
    return trace;
}

// Is this batch one for the device planner?  Pure: takes no lock, makes no HIP call, sets no error.  *ragged: the buffer lengths
// differ; *length: the longest stream's, in values.
bool routed_eligible(rsmp_fir* const* rs, size_t n, const size_t* in_lens, size_t chunk_len, const size_t* out_caps, int planner,
                     bool* ragged_out, size_t* length_out) {
    if (planner == 0 || n < 2) return false;
    // A batch whose buffer lengths differ goes through rsmp_fir_lockstep_run_bulk_v -- where the caller asked for the device planner
    // (planner = 1); the default (planner = -1) keeps its conditions: one buffer length.  `length`: the longest stream's.
    bool ragged = false;
    size_t longest = in_lens[0];
    for (size_t i = 1; i < n; ++i) {
        ragged = ragged || in_lens[i] != in_lens[0];
        longest = std::max(longest, in_lens[i]);
    }
    if (ragged && planner != 1) return false;
    const size_t ch = rs[0]->channels, length = ragged ? longest : in_lens[0];
    if (ch == 0 || chunk_len % ch != 0 || length % ch != 0) return false;
    const size_t frames = chunk_len / ch;
    // calls every stream accepts whole (rsmp_fir_lockstep_run_bulk), at least a handful of them, the same buffer length for all
    // (ragged: at least a handful for the longest stream, whole calls only for every stream)
    if (frames > kRoutedMaxCallFrames || length / ch < kRoutedMinCalls * frames) return false;
    if (batch_handles_fault(rs, n) != BatchFault::None) return false;  // (the host path says which)
    for (size_t i = 0; i < n; ++i) {
        if (rs[i]->channels != ch) return false;
        if (ragged) {
            if (in_lens[i] % chunk_len != 0) return false;
            // a stream with so many frames buffered that a call could accept less than it is offered (resampler_fir.rs:524-528): the
            // device planner would flag the run afterwards (kLsStatusPartialAccept) -- the host planner's, before anything is launched
            if (in_lens[i] != 0 && rs[i]->mirror.state().available + frames > kMirrorInputCapacity) return false;
            if (in_lens[i] == 0) continue;   // (makes no call: needs no room)
        }
        // room for what the launch will produce: the outputs below the limit once `length` more values are accepted, in exact arithmetic
        // (fir_mirror_fast.h: mirror_predict's m1), + 2 for an output that f64 puts a hair below it.  (rsmp_fir_bulk_output_bound is
        // no test here: it grows with the frames a stream has buffered, and a buffer sized by it before the stream's first launch
        // would fail it ever after.)  Anything else: the host path, which checks the room exactly and says so.
        const FirMirrorState st = rs[i]->mirror.state();
        const uint64_t a_now = st.abs_consumed + st.available + in_lens[i] / ch;
        if (st.num == 0 || st.den == 0 || st.den >= (1ull << 21) || st.num >= (1ull << 21) || a_now >= (1ull << 40)) return false;
        // ceil(x den / num): the outputs m >= 0 with m num / den < x
        const uint64_t m1 = a_now + 1 > st.taps ? ((a_now + 1 - st.taps) * st.den + st.num - 1) / st.num : 0;
        const uint64_t made = (m1 > st.abs_out ? m1 - st.abs_out : 0) + 2;
        if (out_caps[i] / ch < made) return false;
    }
    if (planner < 0) {
        size_t distinct = 0;
        if (rsmp_fir_batch_distinct_states(rs, n, &distinct) != RSMP_OK || distinct < std::min(kRoutedMinStates, n)) return false;
    }
    *ragged_out = ragged;
    *length_out = length;
    return true;
}

// The cached batch for this list of handles, made if there is none that still matches them (under routed_mu).  cache.end(): a
// batch the lock-step entry refuses -- the host planner's, remembered.
RoutedCache::iterator routed_find_or_make(RoutedCache& cache, rsmp_fir* const* rs, size_t n, size_t frames) {
    const std::vector<rsmp_fir*> key(rs, rs + n);
    auto it = cache.find(key);
    if (it != cache.end() && it->second.ls == nullptr) {   // (a batch the lock-step entry has refused before: the host planner's)
        it->second.used = ++routed_clock;
        return cache.end();
    }
    if (it != cache.end()) {
        int in_sync = 0;
        const int rc_sync = rsmp_fir_lockstep_in_sync(it->second.ls, &in_sync);
        if (route_trace()) fprintf(stderr, "[rsmp] routed batch: in_sync rc %d -> %d, frames %zu / %zu\n", rc_sync, in_sync, it->second.frames, frames);
        if (rc_sync != RSMP_OK || !in_sync || it->second.frames < frames) {
            rsmp_fir_lockstep_discard(it->second.ls);   // (the handles have moved on: they hold the newer state)
            cache.erase(it);
            it = cache.end();
        }
    }
    if (it != cache.end()) return it;
    // (a handle of this batch in ANOTHER cached batch: that one's device states go stale with this launch, which its own next use
    // finds out -- rsmp_fir_lockstep_in_sync --, nothing to do here)
    if (cache.size() >= kRoutedCacheSize) {
        auto oldest = cache.begin();
        for (auto jt = cache.begin(); jt != cache.end(); ++jt)
            if (jt->second.used < oldest->second.used) oldest = jt;
        rsmp_fir_lockstep_discard(oldest->second.ls);
        cache.erase(oldest);
    }
    RoutedBatch rb;
    rb.ls = rsmp_fir_lockstep_new(rs, n, frames);
    if (!rb.ls) {   // (streams a lock-step batch does not take: the host planner's, without an error of this call's -- and remembered)
        last_error_slot().clear();
        rb.used = ++routed_clock;
        cache.emplace(key, std::move(rb));
        return cache.end();
    }
    rb.frames = frames;
    return cache.emplace(key, std::move(rb)).first;
}

// Binds the batch to this launch's buffers, unless it is bound to them already.
int routed_bind(RoutedBatch& rb, rsmp_fir* const* rs, size_t n, const float* const* d_in, float* const* d_out, void* stream) {
    std::vector<const void*> bound;
    bound.reserve(2 * n);
    for (size_t i = 0; i < n; ++i) bound.push_back(d_in[i]);
    for (size_t i = 0; i < n; ++i) bound.push_back(d_out[i]);
    if (route_trace()) fprintf(stderr, "[rsmp] routed batch: %s\n", bound != rb.bound ? "bind" : "bound already");
    if (bound == rb.bound) return RSMP_OK;
    if (rb.bound.empty()) {
        std::vector<size_t> caps(n);
        for (size_t i = 0; i < n; ++i) caps[i] = rsmp_fir_buffer_size_output(rs[i]);   // per CALL, as the reference sizes a call's buffer
        if (int rc = rsmp_fir_lockstep_bind(rb.ls, d_in, d_out, caps.data())) return rc;
    } else {   // (fresh buffers for this launch: the run planned ahead for it stays)
        if (int rc = rsmp_fir_lockstep_rebind_buffers(rb.ls, d_in, d_out, stream)) return rc;
    }
    rb.bound = bound;
    return RSMP_OK;
}

// Runs the bound batch over the buffers and waits for its totals (the states are back in the handles then).
int routed_run(RoutedBatch& rb, size_t n, const size_t* in_lens, size_t ch, size_t frames, bool ragged, size_t length, size_t* consumed,
               size_t* produced, void* stream) {
    if (ragged) {
        std::vector<size_t> totals(n);
        for (size_t i = 0; i < n; ++i) totals[i] = in_lens[i] / ch;
        if (int rc = rsmp_fir_lockstep_run_bulk_v(rb.ls, totals.data(), frames, 0, 0, stream)) return rc;
    } else if (int rc = rsmp_fir_lockstep_run_bulk(rb.ls, length / ch, frames, 0, 0, stream)) return rc;
    uint32_t flags = 0;
    std::vector<size_t> acc(n), made(n);
    if (int rc = rsmp_fir_lockstep_sync_totals(rb.ls, acc.data(), made.data(), &flags)) return rc;
    if (flags & (1u | 8u | 16u))
        return fail(RSMP_ERR_INVALID_ARGUMENT, "bulk batch planned on the device: status flags %u", flags);
    for (size_t i = 0; i < n; ++i) {
        if (consumed) consumed[i] = acc[i];
        if (produced) produced[i] = made[i];
    }
    return RSMP_OK;
}

}  // namespace

void routed_forget(const rsmp_fir* r) {
    std::lock_guard<std::mutex> lock(routed_mu());
    auto& cache = routed_cache();
    for (auto it = cache.begin(); it != cache.end();) {
        if (std::find(it->first.begin(), it->first.end(), r) != it->first.end()) {
            rsmp_fir_lockstep_discard(it->second.ls);
            it = cache.erase(it);
        } else {
            ++it;
        }
    }
}

int batch_bulk_routed(rsmp_fir* const* rs, size_t n, const float* const* d_in, const size_t* in_lens, size_t chunk_len,
                      float* const* d_out, const size_t* out_caps, size_t* consumed, size_t* produced, void* stream, int planner, int* took) {
    *took = 0;
    bool ragged = false;
    size_t length = 0;
    if (!routed_eligible(rs, n, in_lens, chunk_len, out_caps, planner, &ragged, &length)) return RSMP_OK;
    const size_t ch = rs[0]->channels, frames = chunk_len / ch;
    std::lock_guard<std::mutex> lock(routed_mu());
    auto& cache = routed_cache();
    const auto it = routed_find_or_make(cache, rs, n, frames);
    if (it == cache.end()) return RSMP_OK;
    RoutedBatch& rb = it->second;
    rb.used = ++routed_clock;
    *took = 1;
    int rc = routed_bind(rb, rs, n, d_in, d_out, stream);
    if (rc == RSMP_OK) rc = routed_run(rb, n, in_lens, ch, frames, ragged, length, consumed, produced, stream);
    if (rc != RSMP_OK) {   // (whatever state the batch is in now: not one to keep)
        const std::string msg = last_error_slot();
        rsmp_fir_lockstep_discard(rb.ls);
        cache.erase(it);
        last_error_slot() = msg;
    }
    return rc;
}

}  // namespace rsmp
