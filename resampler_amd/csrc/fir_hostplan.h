// fir_hostplan.h -- the host planner of ResamplerFir: replays the reference's call sequence on a copy of a stream's
// mirror and keeps what a launch needs of it (counts, position runs or wrapped outputs, the state behind it).
// Plain values in, a shared immutable Plan out: no handle, no device, no HIP header.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "fir_plan.h"

namespace rsmp {

// The host-side result of replaying a reference call sequence: shared between the streams of a
// batch that are in the same state and are fed the same amount of input (their control flow is
// data independent, so one replay serves all of them).
struct Plan {
    FirMirror planned;                      // mirror state after the launch
    std::vector<rsmp_fir_segment> segs;     // generic kernel: exact position runs
    std::vector<uint32_t> wraps;            // periodic kernel: row-1023 fix-ups
    std::vector<uint32_t> wrap_bits;        // ... as the bitmap the kernels with inline wraps read (built with the plan, by its worker)
    std::vector<size_t> calls;              // (accepted, produced) per reference call, in frames
    size_t accepted_frames = 0;
    size_t produced_frames = 0;
    size_t consumed_frames = 0;
    size_t hist_frames = 0;
    bool periodic = false;
    explicit Plan(const FirMirror& m) : planned(m) {}
};

// What one stream asks of the planner.  in_len / out_cap / chunk_len are f32 values; chunk_len 0: one reference call
// with output capacity out_cap, else the bulk driver loop.
struct PlanRequest {
    const FirMirror& mirror;
    size_t channels, taps;
    uint32_t in_hz, out_hz;
    int kernel_mode;
    size_t in_len, out_cap, chunk_len;
};

struct PlanKey {
    uint32_t in_hz, out_hz;
    size_t taps, channels, read_position, available;
    uint64_t position_bits, abs_out, abs_consumed;
    size_t in_len, out_cap_or_zero, chunk_len;
    int kernel_mode;
    bool operator==(const PlanKey& o) const { return std::memcmp(this, &o, sizeof o) == 0; }
};
PlanKey make_key(const PlanRequest& q);

// Replays the call sequence on a copy of the mirror; a bulk request is looked up in the process-wide cache first.
int plan_job(const PlanRequest& q, std::shared_ptr<Plan>* out);

// The reference's bulk driver loop (resample/src/main.rs:226-254) on a mirror: every call offers min(chunk, remaining)
// frames and the full output capacity; stops after max_calls calls (0 = no limit), when the input is used up or when a
// call accepts nothing.  segs / wraps / calls: what to keep of it (each may be null).  `overflow`: a caller that keeps
// runs or wraps indexes outputs with 32 bits; the loop stops BEFORE the call that could pass 2^31 of them.
struct BulkTotals {
    size_t accepted = 0, produced = 0, consumed = 0, calls = 0;   // frames
    bool overflow = false;
};
BulkTotals drive_bulk(FirMirror& m, size_t in_frames, size_t chunk_frames, size_t max_calls, std::vector<rsmp_fir_segment>* segs,
                      std::vector<uint32_t>* wraps, std::vector<size_t>* calls);

// A launch's coefficient rows are mixed for ONE drift, the stream's f64 drift moves by ~1e-14 of a frame per output: a
// bulk call of more than kMaxLaunchOutputs outputs is cut into launches of at most that many (at call boundaries: the
// reference's loop, resample/src/main.rs:226-254, does not know the difference), each with the table of its own middle --
// 2e-7 of a frame from either end, 3e-7 of a full-scale sample.  (Config 5's 26.5 M outputs stay one launch.)
constexpr uint64_t kMaxLaunchOutputs = 46000000ull;
// ... as input: the f32 values one launch takes, whole chunks, at least one.  chunk_len: a multiple of channels, not 0.
inline size_t launch_input_values(double ratio, size_t channels, size_t chunk_len) {
    const size_t chunks = static_cast<size_t>(static_cast<double>(kMaxLaunchOutputs) * ratio / static_cast<double>(chunk_len / channels));
    return (chunks ? chunks : 1) * chunk_len;
}

}  // namespace rsmp
