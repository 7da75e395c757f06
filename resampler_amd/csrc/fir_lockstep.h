// fir_lockstep.h -- lock-step batch of ResamplerFir streams with DEVICE-resident state.
//
// BASELINE config 4 (a thousand independent streams of mixed rate pairs, each fed one 512-frame
// chunk per step) is microseconds of GPU work per step: any per-stream host work -- replaying the
// state machine, assembling descriptors, uploading them -- costs more than the arithmetic.  A lock-step
// batch therefore keeps everything a step needs in HBM: the streams' reference state
// (read_position / available_frames / position, resampler_fir.rs:189-192), their buffered frames, their
// buffer pointers.  One step is ONE kernel launch with constant arguments; the kernel runs the
// reference's control flow itself (fir_mirror_core.h, one lane per stream), stages every stream's
// [buffered | new] frames in LDS, computes the outputs on the matrix cores with "row = stream"
// (the 16 columns of a tile are (stream, period) pairs, so short steps of many streams fill the
// tiles), retires the consumed frames and writes (consumed, produced) per stream to HBM.
// Two-channel streams use the arithmetic of fir_split.hip (operands cut into two fp16 planes, three
// v_mfma_f32_16x16x32_f16 products per term, f32 accumulation): 5x less matrix-pipe time than exact f32
// products, which stay available (rsmp_fir_set_kernel(.., RSMP_FIR_KERNEL_PERIODIC_F32), other channel counts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "fir_mirror_core.h"
#include "fir_mirror_fast.h"
#include "fir_kernels.h"
#include "fir_lockstep_plan.h"
#include "fir_periodic.h"

namespace rsmp {

struct LockstepStream {        // per bound stream, constant between binds (HBM)
    const float* in;           // a step reads in + in_offset, in_frames frames
    float* out;
    float* hist;               // frames buffered between steps (interleaved): a step with an even index reads
    float* hist_alt;           // `hist` and leaves its tail in `hist_alt`, an odd one the other way round
    const float* coeffs;       // [1024][taps] polyphase table
    uint64_t out_cap_frames;   // room of `out` per step, in frames
};

struct LockstepArgs {
    const LockstepGroup* groups;
    const LockstepStream* streams;
    FirMirrorState* states;
    uint64_t* out_cursor;                 // f32 values appended so far per stream (append mode)
    uint64_t* counts;                     // [n][2]: (consumed, produced) of the step, in f32 values
    uint32_t* status;                     // sticky per-stream flags (kLsStatus*)
    const uint32_t* order;                // internal stream index -> index in the caller's order
    const uint32_t* in_frames_per_stream; // optional: frames offered per stream, in the caller's order
    uint64_t in_offset;                   // frames added to every stream's `in`
    uint32_t in_frames;                   // frames offered to every stream (when the array is null)
    uint32_t append;                      // 1: a step's output goes to out + out_cursor; 0: to out
    uint32_t in_aligned8;                 // every two-channel stream's `in` is 8-byte aligned (split variant: 8-byte loads)
    unsigned long long* trace;            // diagnostic instantiation only (RSMP_LS_TRACE), else null
    // Plans are computed one step AHEAD: while the other waves of a workgroup compute step k, its first
    // wave runs the state machine for step k + 1 (assuming the same number of frames will be offered) and
    // leaves the result in the stream's plan record; step k + 1 then starts from the record instead of
    // ~20 k cycles of serial f64 arithmetic.  A record is used only if its epoch, step and frame count
    // match; otherwise the step plans in line as before.
    uint32_t* peaks;                      // [n_streams][4]: epoch, step it is a prediction for, bits of the stream's latest peak, -
    char* recs;                           // [2][n_streams] records of rec_stride bytes (parity = step & 1)
    uint32_t rec_stride, n_streams;
    uint32_t epoch, step;
    uint32_t hist_parity;                 // 0: this step reads `hist` and leaves its tail in `hist_alt`; 1: the other way round
};

struct LsPlanHeader {          // head of a plan record; followed by kLsSegCap runs (24 B each), then the wrap list
    uint32_t epoch, step, in_frames, n_out;
    uint32_t hist_frames, accepted, consumed, tail_frames;
    uint32_t n_segs, n_wraps, flags, pad0;
    uint64_t abs_out, abs_consumed;
    FirMirrorState after;      // the stream's state after the step
    uint64_t pad1;
};
static_assert(sizeof(LsPlanHeader) == kLsRecSegs, "plan record layout (fir_lockstep_plan.h: lockstep_rec_stride)");

constexpr uint32_t kLsStatusRunOverflow = 1;   // more than kLsSegCap position runs in one step
constexpr uint32_t kLsStatusNonFinite = 2;     // a step saw non-finite samples (reference-form path taken)
constexpr uint32_t kLsStatusAperiodic = 4;     // the f64 drift left the class tables' tolerance
constexpr uint32_t kLsStatusPartialAccept = 8; // rsmp_fir_lockstep_run: a call accepted fewer frames than it was offered
constexpr uint32_t kLsStatusPlannerCheck = 16; // rsmp_fir_lockstep_run: the replay of a call found a premise of the planner's closed form violated (never observed)

hipError_t launch_fir_lockstep(const LockstepArgs& args, uint32_t n_groups, uint32_t max_lds_bytes,
                               hipStream_t stream);

// ---- rsmp_fir_lockstep_run: k calls per stream, planned on the device, computed by the bulk kernels ------------
struct LsRunStream {           // per stream (internal order), constant for the batch
    uint32_t wrap_unit;        // the bitmap of wrapped outputs starts at output (abs_out / wrap_unit) * wrap_unit: the bulk
                               // geometry's b (= den unless a super period of an exact ratio, whose outputs never wrap)
    uint32_t den, channels;
    uint32_t caller;           // the stream's index in the caller's order
    // the class tables of the bulk kernels and the drift they were built for: replaced as the stream's f64 drift moves on
    // (fir_lockstep_api.cpp, DriftClass); the planner copies them into every run's descriptor
    const float* class_coef;
    const float* class_wrap_coef;
    const TileMeta* class_meta;
    double drift;
};
struct LsRunArgs {
    const LockstepStream* streams;
    const LsRunStream* rs;
    const FirMirrorState* states_in;
    FirMirrorState* states_out;
    FirMirrorState* states_before;   // [n]: copy of the states the run started from
    MirrorPred* preds;         // [n][k]: the predicted structure of every call (fir_mirror_fast.h)
    void* call_recs;           // [n][k] x 24 bytes: what the chain leaves per call for the replay
    const uint64_t* cursor_in;
    uint64_t* cursor_out;
    FirStreamDesc* descs;      // [n]: the run's descriptors (the constant fields are the host's)
    uint32_t* wrap_bits;       // [n][wrap_words]
    uint32_t* counts;          // [k][n][2] in the caller's order: (consumed, produced) per call in f32 values
    uint64_t* last_counts;     // [n][2], internal order: the last call's (rsmp_fir_lockstep_counts)
    uint32_t* status;          // per-stream flags: ORed into
    uint32_t* zero_status;     // non-null: `status` is a scratch copy of a run planned AHEAD -- cleared here first (the commit ORs it in)
    uint64_t in_offset;        // frames added to every stream's `in`
    uint32_t n_streams, k, in_frames, wrap_words, append, hist_parity;
    uint32_t parallel_chain;   // K2: chunks of lean calls by the parallel chain (set by launch_fir_lockstep_plan; RSMP_LS_PCHAIN=0, debug: never)
    // A RAGGED run (rsmp_fir_lockstep_run_bulk_v): frames per stream, internal order; null: every stream makes k calls of in_frames.
    // Stream i makes totals[i] / in_frames calls of in_frames frames and, where that leaves a remainder, one more of that many;
    // k is then the batch's largest number of calls (the short one included) and stays the stride of preds / call_recs / counts.
    const uint32_t* totals;
};
struct LsCommitArgs {
    FirMirrorState* states; const FirMirrorState* sp_states;
    uint64_t* cursor; const uint64_t* sp_cursor;
    uint64_t* last_counts; const uint64_t* sp_last_counts;
    uint32_t* status; const uint32_t* sp_status;
    uint32_t n_streams;
};
// parts: 1 = K1 (the predictions), 2 = K2 + K3 (chain, replay); 3 = all three in `stream`
// What is launched -- grids, blocks, the chain's build -- is fir_lockstep_plan.h's lockstep_plan_shape(n_streams, k).
// (commit, with part 1: K1 also does what launch_fir_lockstep_commit does -- the first thread of a stream's calls copies the
// stream's scratch results into place -- and reads the states it predicts from out of the scratch copies: one launch less in
// front of a run planned ahead)
// (k1_done, with part 1: an event the K1 launch itself completes -- hipExtLaunchKernel's stop event --, no packet of its own
// behind it as hipEventRecord would put there)
hipError_t launch_fir_lockstep_plan(const LsRunArgs& args, hipStream_t stream, int parts = 3, const LsCommitArgs* commit = nullptr,
                                    hipEvent_t k1_done = nullptr);
// out[c] = states[reps[c]].drift: the drifts the batch's classes are watched by (one thread per class).
hipError_t launch_fir_lockstep_gather_drift(const FirMirrorState* states, const uint32_t* reps, double* out, uint32_t n,
                                            hipStream_t stream);
// Do two streams run side by side?  (HIP deals a handful of hardware queues to its streams in turn; two streams on one
// queue run their kernels strictly one after the other.)  `wait` goes to the one stream: a single wave that polls *flag
// until it reads `token` or `timeout_ticks` of the 100 MHz clock have passed, and stores 1 / 0 to *result (mapped host
// memory).  `set` goes to the other stream and stores `token` to *flag.  On one queue `set` cannot start before `wait`
// has given up: the result is decided by the DEVICE, whatever the host's threads are doing meanwhile (round 4 timed the
// pair with the host's clock against a 200 us threshold, which a busy host fails both ways).
hipError_t launch_fir_lockstep_probe_wait(uint32_t* flag, uint32_t token, uint32_t timeout_ticks, uint32_t* result, hipStream_t stream);
hipError_t launch_fir_lockstep_probe_set(uint32_t* flag, uint32_t token, hipStream_t stream);
// New class tables for up to kLsMaxPatches drift classes, written into the device copies of the group table (step
// kernel: the groups whose `pad0` names the class) and the run planner's stream table (streams [first, first + count))
// by ONE small kernel in stream order -- no copy-engine operation, no staging buffer to wait for.
constexpr uint32_t kLsMaxPatches = 8;
struct LsTablePatch {
    uint32_t cls, first, count, flags;     // flags: 1 = step table, 2 = run table
    const float* step_coef; const TileMeta* step_meta;
    const float* run_coef; const float* run_wrap_coef; const TileMeta* run_meta;
    double drift;
};
struct LsPatchArgs {
    LockstepGroup* groups; LsRunStream* rs;   // (rs: null before the batch's first run)
    uint32_t n_groups, n_streams, n_patches, pad;
    LsTablePatch p[kLsMaxPatches];
};
hipError_t launch_fir_lockstep_patch_tables(const LsPatchArgs& args, hipStream_t stream);
// A run planned ahead (on a stream of its own, while the previous run computes) left its results in scratch copies:
// states, append positions, the last call's counts, status flags -> the batch's own, when the run is really asked for.
hipError_t launch_fir_lockstep_commit(const LsCommitArgs& args, hipStream_t stream);
// A run planned ahead names the buffers the batch was bound to when it was planned: descs[gs].in / .out again from the stream table as
// it is now (rsmp_fir_lockstep_rebind_buffers; a run that starts at the front of `out`: no `append`).
hipError_t launch_fir_lockstep_rebase(FirStreamDesc* descs, const LockstepStream* streams, const LsRunStream* rs, uint64_t in_offset,
                                      uint32_t n_streams, hipStream_t stream);
hipError_t launch_fir_lockstep_gather_counts(const uint64_t* last_counts, const LsRunStream* rs, uint32_t* counts, uint32_t n,
                                             hipStream_t stream);
// A ragged run as a loop of steps (rate pairs no bulk kernel serves).  In front of step `step`: what every stream is offered,
// clamp(totals[gs] - step * chunk, 0, chunk) frames, into offer[caller index] (rsmp_fir_lockstep_step's d_in_frames), and the
// counts of the stream's latest call into `keep`; cursor_to_front (the run's first step, no `append`; else null): the append
// positions of the streams that make a call go back to 0.  Behind the step: the step's counts into the row of the run's table -- or, for a
// stream that is through (its call was an empty one, which the driver loop never makes), zeros into the row and `keep` back into
// last_counts.
hipError_t launch_fir_lockstep_ragged_offer(const uint32_t* totals, const LsRunStream* rs, uint32_t* offer, const uint64_t* last_counts,
                                            uint64_t* keep, uint64_t* cursor_to_front, uint32_t step, uint32_t chunk, uint32_t n,
                                            hipStream_t stream);
hipError_t launch_fir_lockstep_ragged_gather(const uint32_t* totals, const LsRunStream* rs, uint64_t* last_counts, const uint64_t* keep,
                                             uint32_t* counts, uint32_t step, uint32_t chunk, uint32_t n, hipStream_t stream);

}  // namespace rsmp
