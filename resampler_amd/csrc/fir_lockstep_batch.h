// fir_lockstep_batch.h -- the lock-step batch as its host files see it (fir_lockstep_api.cpp: the C ABI; fir_lockstep_drift.cpp:
// drift classes and their tables; fir_lockstep_runpath.cpp: rsmp_fir_lockstep_run and the bulk entries).  One member per
// concern, each with the functions that work on it declared beside it.  Host only: no .hip file includes this.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <vector>

#include "common.h"
#include "device_util.h"
#include "fir_handle.h"
#include "fir_lockstep.h"
#include "fir_table_refresher.h"

struct rsmp_fir_lockstep;

namespace rsmp {

inline bool ls_verbose() { static const bool v = knob("RSMP_FIR_VERBOSE") != nullptr; return v; }

// The class tables follow the streams' f64 drift.  The reference's position (src/resampler_fir.rs:589) moves away from
// the exact rational one by ~1e-14 of a frame per output for as long as a stream runs (every add rounds on the grid of
// its binade): 1e-6 of a frame after half an hour of audio -- 2e-6 of a full-scale sample with coefficient rows mixed
// for another drift.  Streams of one key whose drifts lie together form a class; the class's tables are built for the
// drift of its first stream, which is read back from the device now and then (asynchronously: a tiny kernel, a copy
// into pinned memory, an event looked at when the next step or run is enqueued); when it has moved by more than
// kLsDriftTolerance, the tables are replaced (class_table_for: cached per device, built on the host otherwise).
struct DriftClass {
    uint32_t rep = 0;                 // internal index of the stream that stands for the class
    size_t first = 0, count = 0;      // its streams, internal order
    double table_drift = 0.0;         // what the bound tables were built for
    const rsmp_fir* r0 = nullptr;
    bool has_step = false, has_run = false;
    rsmp::PeriodicGeometry step_geo, run_geo;
    rsmp::ClassTable step_table, run_table;
    // Tables of the process-wide cache this class has bound (creation, reset: the host knows the states and may
    // wait) stay held until nothing enqueued or planned ahead can read them (bind / reset, behind their waits) --
    // the cache is bounded, and a table it has evicted lives by its holders alone.
    std::vector<std::shared_ptr<void>> holds;
    // The NEXT tables: owned double-buffered device images that the batch's worker thread fills when the drift has
    // covered most of the way to the tolerance (TableRefresher: host arithmetic, allocation, upload and the wait
    // for it all happen there); the crossing swaps pointers.
    rsmp::TableRefresher::Table* step_next = nullptr;
    rsmp::TableRefresher::Table* run_next = nullptr;
    bool next_pending = false;        // a request is out (or its result is waiting to be taken)
    double next_drift = 0.0;
    double seen_drift = 0.0;          // the class's drift as last read back ...
    double rate = 0.0;                // ... and how fast it moves per input frame (from the last two readings)
    bool late = false;                // past the tolerance, the next tables not there yet
};

// Drift classes and the replacement of their tables (fir_lockstep_drift.cpp).  Holds no stream of the caller's.
struct Drift {
    std::vector<DriftClass> classes;
    std::unique_ptr<rsmp::TableRefresher> refresher;
    double tolerance = 0.0;               // (set at creation: kLsDriftTolerance; rsmp_fir_lockstep_set_drift_policy)
    uint64_t check_frames = 0;
    size_t n_late = 0;                    // classes currently `late`
    // A reading tells where the DEVICE was when the gather kernel ran; what the host enqueues now runs later -- by as much
    // as the host is ahead of the device (a caller that never waits: thousands of launches, tens of millions of frames per
    // stream: several tolerances of drift).  Decisions are made for the drift a launch enqueued NOW will see: the last
    // reading + the measured rate x the frames enqueued since that reading was asked for.
    uint64_t frames_total = 0;            // input frames per stream enqueued through this batch so far
    uint64_t frames_at_inflight = 0;      // ... when the reading in flight was asked for
    uint64_t frames_at_seen = 0;          // ... when the latest completed reading was asked for
    bool have_seen = false;
    uint64_t frames_at_eval = 0;          // (when the classes were last looked at)
    uint64_t frames_since = 0;            // ... since a reading was last asked for
    std::vector<rsmp::TableRefresher::Table*> guards_due;   // images unbound by this call's replacements (record_guards)
    DeviceBuffer d_reps;
    rsmp::PinnedBuffer h_drift, h_stage;            // the drifts read back; staging of the group / stream tables when they change
    EventHolder ev, stage_ev;
    bool inflight = false, stage_inflight = false, groups_dirty = false, rs_dirty = false;
    // diagnostics (rsmp_fir_lockstep_stats)
    size_t table_rebinds = 0;             // times a class got new tables
    uint64_t table_ops = 0;               // patch launches + table uploads enqueued on a caller's stream (poll_drift, flush_tables)
    uint64_t late_polls = 0, table_waits = 0;
};
double quantized_drift(double d);
int rebind_class_blocking(rsmp_fir_lockstep* ls, size_t c, double d);
int poll_drift(rsmp_fir_lockstep* ls, hipStream_t s);
int flush_tables(rsmp_fir_lockstep* ls, hipStream_t s);
int request_drift(rsmp_fir_lockstep* ls, hipStream_t s, uint64_t frames);
int rebind_from_host_states(rsmp_fir_lockstep* ls);
int set_drift_policy(rsmp_fir_lockstep* ls, double tolerance_frames, size_t check_frames);
void init_drift(rsmp_fir_lockstep* ls);   // (creation: the default policy, the refresher)
long long drift_class_of(double drift);   // streams of one key whose drifts give the same value share a class

// rsmp_fir_lockstep_run (k calls per stream and launch): the bulk kernels' geometry per rate pair, the run's
// descriptors and what the device-side planner leaves for them (fir_lockstep_run.hip)
struct RunGroup { rsmp::PeriodicGeometry geo; size_t first = 0, count = 0; uint32_t max_out_step = 0; };
// The run's descriptors, bitmaps, per-call counts and call records exist twice ("slots", used alternately): the NEXT run
// is planned ahead on a stream of its own while the current one computes (PlanAhead below) and must not overwrite
// what the current run's kernels and the caller (run_counts) still read.
struct RunSlot { DeviceBuffer descs, bits, counts, recs; EventHolder compute_done; hipStream_t compute_stream = nullptr; bool used = false, compute_recorded = false;
                 // the split kernel's item tables of the run planned ahead into this slot, built on the plan stream behind its plan
                 DeviceBuffer items; uint64_t items_seq = 0, items_ops = 0; bool items_valid = false; };
// A slot's `compute_stream` may be a caller's stream.
struct RunSlots {
    int state = 0;              // 0: not looked at yet, 1: every rate pair has a bulk kernel, -1: runs are loops of steps
    std::vector<RunGroup> groups;
    RunSlot slot[2];
    int next_slot = 0, last_slot = 0;
    std::vector<rsmp::LsRunStream> h_rs;
    DeviceBuffer d_rs, d_nf, d_work, d_preds, d_states0;
    // planned ahead: states / append positions / last counts / status flags of the run AFTER the current one, in scratch
    // copies until the run is really asked for (then committed by one small kernel), or dropped
    DeviceBuffer sp_states, sp_cursor, sp_last, sp_status;
    uint64_t seq = 0;
    uint32_t wrap_words = 0, k = 0, nf_tag = 0;
    bool planned = false;       // the most recent run went through the device planner
    size_t counts_k = 0;        // calls of the most recent run whose counts are in slot[last_slot].counts
    std::vector<uint32_t> h_counts;
    void forget_caller_streams(hipStream_t own) {
        for (auto& sl : slot)
            if (sl.compute_stream != own) { sl.used = false; sl.compute_stream = nullptr; }
    }
};

struct RunKey { uint32_t k = 0, in_frames = 0, append = 0, parity = 0; uint64_t in_offset = 0, seq = 0; int slot = 0; bool valid = false; };
// `waited_on` may be a caller's stream (only compared, never used).
struct PlanAhead {
    RunKey ahead;               // what the plan stream was asked to plan
    bool inflight = false;      // ... and has not been waited for since
    RunKey prev;                // the previous run (the pattern the next one is guessed from)
    bool rebased = false;       // the buffers changed under a run planned ahead (rsmp_fir_lockstep_rebind_buffers): its descriptors are patched when it is taken over
    EventHolder ev_ready, done, ev_commit;
    hipStream_t q = nullptr;             // the plan stream the run planned ahead was enqueued on
    bool waited = false;                 // the caller's stream `waited_on` already waits for `done` (rsmp_fir_lockstep_run)
    hipStream_t waited_on = nullptr;
    uint64_t hits = 0, misses = 0, commits_on_plan_stream = 0;   // diagnostics (rsmp_fir_lockstep_stats)
    void forget_caller_streams() { waited = false; waited_on = nullptr; }
};
int drop_plan_ahead(rsmp_fir_lockstep* ls, hipStream_t s);

// caller's stream -> the candidate that runs beside it, found out by a probe that the DEVICE decides and the host
// never waits for (launch_fir_lockstep_probe_wait): until it is known, runs on that stream are not planned ahead.
// `probe_owner` and the map's keys are streams of the caller's; the keys are only compared.
struct PlanStreamPick {
    hipStream_t stream = nullptr;   // the candidate picked for the caller's stream of the last run (pick_plan_stream)
    StreamHolder candidates[2];
    struct Pick { int pick = -1; bool decided = false, probing = false; int cand = 0, tries = 0; };
    std::map<hipStream_t, Pick> by_stream;
    DeviceBuffer d_probe;                // the probes' flag word
    rsmp::PinnedBuffer h_probe;          // ... and their result
    EventHolder probe_ev;
    hipStream_t probe_owner = nullptr;   // the caller's stream whose probe is in flight (one at a time)
    uint32_t probe_token = 0;
    uint64_t probes = 0;                 // diagnostic (rsmp_fir_lockstep_stats)
    void take_probe_answer();
    void forget_caller_streams();
};

// rsmp_fir_lockstep_run_bulk_v: the streams' frame totals (internal order) on the device, uploaded in stream order from a small
// ring of pinned staging buffers (the caller's array is free when the call returns; a launch enqueued behind launches that
// have not run yet does not wait for them); a loop of steps also keeps what every stream is offered per step and the counts
// of its latest real call
struct RaggedTotals {
    static constexpr int kRing = 4;
    DeviceBuffer d_totals, d_offer, d_keep;
    rsmp::PinnedBuffer h[kRing];
    EventHolder ev[kRing];
    bool inflight[kRing] = {};
    int next = 0;
};

// optional timing of the step launches (rsmp_fir_lockstep_set_profiling): ring of event pairs
struct StepProfiler {
    static constexpr int kRing = 256;
    bool on = false;
    EventHolder start[kRing], stop[kRing];
    size_t count = 0;
    hipError_t begin(hipStream_t s) { return on ? event_record(start[count % kRing], s) : hipSuccess; }
    hipError_t end(hipStream_t s) { return on ? event_record(stop[count++ % kRing], s) : hipSuccess; }
};

int lockstep_run(rsmp_fir_lockstep* ls, size_t k_steps, size_t in_frames, size_t in_offset_frames, int append, void* stream,
                 const uint32_t* d_totals);

}  // namespace rsmp

struct rsmp_fir_lockstep {
    // the step kernel's tables, and what every entry point shares
    int device = 0;
    uint32_t step_frames = 0;
    size_t max_taps = 0;              // the longest stream's
    std::vector<rsmp_fir*> rs;        // caller order
    std::vector<uint32_t> order;      // internal index -> caller index
    std::vector<rsmp::LockstepGroup> groups;
    std::vector<rsmp::LockstepStream> streams;   // internal order
    std::vector<uint32_t> channels;        // internal order
    bool in_aligned8 = false;
    rsmp::DeviceBuffer d_groups, d_streams, d_states, d_cursor, d_counts, d_status, d_order, d_recs, d_peaks;
    uint32_t rec_stride = 0, epoch = 1, step = 0;   // plan-ahead records (fir_lockstep.h)
    uint32_t max_lds = 0;
    bool bound = false;
    hipStream_t last_stream = nullptr;   // may be a caller's stream
    rsmp::StreamHolder own_stream;
    std::vector<uint64_t> h_counts;
    std::vector<rsmp::FirMirrorState> h_states;
    uint32_t hist_parity = 0;   // 0: the next step / run reads `hist` of LockstepStream and leaves its tail in `hist_alt`
    rsmp::Drift drift;
    rsmp::RunSlots run;
    rsmp::PlanAhead plan;
    rsmp::PlanStreamPick pick;
    rsmp::RaggedTotals totals;
    rsmp::StepProfiler prof;

    // A run's or a bulk entry's calls of `frames` frames are ones every stream accepts whole: a stream buffers at most
    // kMirrorInputCapacity frames and keeps up to taps + 1 of them between calls.
    bool accepts_whole(size_t frames) const { return frames + max_taps + 8 <= rsmp::kMirrorInputCapacity; }
    // "order this launch behind the batch's previous stream": steps and runs of one batch are ordered, a change of stream
    // waits for the previous launch
    hipError_t order_behind_last(hipStream_t s) { return last_stream && last_stream != s ? hipStreamSynchronize(last_stream) : hipSuccess; }
    hipError_t wait_last_launch() { return last_stream ? hipStreamSynchronize(last_stream) : hipSuccess; }
};
