// fir_launch.h -- one launch of ResamplerFir: planned jobs in, kernels enqueued on one stream, handles committed.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "fir_format.h"
#include "fir_handle.h"
#include "fir_hostplan.h"

namespace rsmp {

// One stream's part of a launch.
struct FirJob {
    rsmp_fir* r;
    const float* d_in;
    size_t in_len;     // f32 values offered
    float* d_out;      // (PCM output: the bytes' address)
    size_t out_cap;    // values (samples) of room
    size_t chunk_len;  // 0: one reference call with output capacity out_cap; else bulk loop
    std::shared_ptr<Plan> plan;
    size_t consumed() const { return plan->accepted_frames * r->channels; }
    size_t produced() const { return plan->produced_frames * r->channels; }
    PlanRequest request() const {
        return PlanRequest{r->mirror, r->channels, r->taps, r->in_hz, r->out_hz, r->kernel_mode, in_len, out_cap, chunk_len};
    }
};

// The event `leader` records behind what it enqueues (the launch it leads, a seek's copy).
int launch_event(rsmp_fir* leader);
// ... recorded behind everything `leader` has just enqueued on `stream` (`attached`: the last launch completes it already).
int record_launch(rsmp_fir* leader, hipStream_t stream, bool attached = false);

// Launches that touch a handle (its buffered frames, its plan slots, the leader's item queue) are
// ordered: the ABI lets every call name a stream, so a handle that was last used on another stream
// makes this stream wait for the event of its last launch (rare; a caller that keeps one stream per
// handle never waits here).  An event, not the previous stream: the caller may have destroyed that one.
// `waited`: the event `stream` was last made to wait for (null at first), so that the handles of one batch wait once.
int order_behind_handle(rsmp_fir* h, hipStream_t stream, const FirLaunchEvent*& waited);

// Assembles and enqueues the launches for a set of planned jobs on one device / stream.
// `leader` owns the launch workspace.
// format (fir_format.h): what every job's d_in and d_out hold and how PCM output is stored -- the entry has built it from the widths and the handles'
// settings and held every handle to it; the periodic groups are held to it here (format_group_fault): RSMP_ERR_INVALID_ARGUMENT before anything is launched or changed.
int launch_jobs(rsmp_fir* leader, std::vector<FirJob>& jobs, hipStream_t stream, const FirFormat& format = FirFormat{});

}  // namespace rsmp
