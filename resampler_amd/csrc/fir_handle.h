// fir_handle.h -- the ResamplerFir handle behind the C ABI (shared by the files of its front-end,
// DESIGN.md 4.3b, and fir_lockstep_api.cpp; not part of the public interface).
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "device_util.h"
#include "fir_periodic.h"
#include "fir_plan.h"

// An event recorded behind a launch on its stream, shared by the handles of a batch launch (the leader re-records its own
// for every launch it leads: each handle's launches are ordered, so the later recording completes after the earlier one).
struct FirLaunchEvent {
    hipEvent_t ev = nullptr;
    ~FirLaunchEvent() { if (ev) (void)hipEventDestroy(ev); }
};

struct rsmp_fir {
    int device = 0;
    size_t channels = 0;
    size_t taps = 0;
    int attenuation = 0;
    uint32_t in_hz = 0, out_hz = 0;
    int kernel_mode = RSMP_FIR_KERNEL_AUTO;
    rsmp::FirMirror mirror;
    std::shared_ptr<const std::vector<float>> table;
    float* d_coeffs = nullptr;
    float* d_hist[2] = {nullptr, nullptr};  // kInputCapacity * channels floats each
    int cur = 0;
    hipStream_t stream = nullptr;
    // Launch plans travel through a small ring of pinned buffers so the host can enqueue several
    // launches ahead of the GPU (a slot is reused only after its upload has left host memory).
    static constexpr int kPlanSlots = 4;
    rsmp::EventHolder plan_copied[kPlanSlots];
    bool plan_pending[kPlanSlots] = {false, false, false, false};
    int plan_slot = 0;
    // launch workspace (descs + runs + tile index), host-pinned and device
    rsmp::PinnedBuffer h_plan[kPlanSlots];
    rsmp::DeviceBuffer d_plan[kPlanSlots];
    std::vector<char> plan_image[kPlanSlots];   // what each slot's HBM buffer currently holds
    std::vector<char> plan_scratch;
    // staging for the host-pointer entry points
    rsmp::DeviceBuffer d_stage_in, d_stage_out;
    rsmp::PinnedBuffer h_stage_in, h_stage_out;   // small calls: the kernels read / write mapped host memory, no copy engine
    rsmp::PeriodicState periodic;
    bool last_periodic = false;   // the handle's last launch went through a periodic kernel
    unsigned long long* d_work_counter = nullptr;   // periodic kernel's item queue (leader only), zero between launches
    rsmp::DeviceBuffer d_nf;                        // non-finite marks of the periodic launches (leader only)
    uint32_t nf_tag = 0;
    hipStream_t last_stream = nullptr;              // the stream of the handle's most recent launch (compared, never used:
    bool last_stream_valid = false;                 // the caller may have destroyed it by the next call)
    // ... and the event behind that launch: a call on another stream waits for it there (fft_api.cpp does the same)
    std::shared_ptr<FirLaunchEvent> last_launch, launch_ev;   // (launch_ev: the one this handle records when it leads a launch)
    // optional timing of the main convolution launch(es) (rsmp_fir_set_profiling)
    bool profiling = false;
    // ring of event pairs: launches made while profiling is on are timed without any host sync
    static constexpr int kProfRing = 64;
    rsmp::EventHolder prof_start[kProfRing], prof_stop[kProfRing];
    size_t prof_count = 0;
    // PCM output (rsmp_fir_batch_resample_bulk_pcm_out_device): RSMP_DITHER_* and the stream's seed (rsmp_fir_set_pcm_dither).
    // A setting, not state: reset and seek leave it alone; the noise counter is the mirror's abs_out.
    int pcm_dither = RSMP_DITHER_NONE;
    uint64_t pcm_dither_seed = 0;
    int pcm_dither_shape = RSMP_DITHER_SHAPE_WHITE;   // (rsmp_fir_set_pcm_dither_shape; read only under RSMP_DITHER_TPDF)
    // ... and the stream's output gain (rsmp_fir_set_pcm_gain): only the PCM-output entry reads it
    float pcm_gain = 1.0f;
    // ... and its statistics (rsmp_fir_set_pcm_stats): the setting -- reset and seek leave it -- and the handle's totals, one
    // rsmp_pcm_stats in device memory that the fold kernel behind every counting launch merges into.  pcm_stats_cleared: the totals
    // are zero whatever the memory holds (a new handle, reset, rsmp_fir_pcm_stats_clear): the next counting launch replaces them.
    // Nothing is enqueued by a clear, and a handle with the setting off has neither buffer.
    bool pcm_stats = false;
    bool pcm_stats_cleared = true;
    rsmp::DeviceBuffer d_pcm_stats;
    rsmp::DeviceBuffer d_stat_table;   // a counting launch's per-chunk table (FirStatArgs, fir_kernels.h; leader only)

    rsmp_fir(uint32_t i, uint32_t o, size_t t) : mirror(i, o, t) {}
};

namespace rsmp {

// What is wrong with a batch's list of handles: the first fault in list order.  (Says nothing and sets no error: the host path
// answers each with a message of its own, the routed path falls through to it.)
enum class BatchFault { None, NullOrOtherDevice, Duplicate };
inline BatchFault batch_handles_fault(rsmp_fir* const* rs, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!rs[i] || rs[i]->device != rs[0]->device) return BatchFault::NullOrOtherDevice;
        for (size_t k = 0; k < i; ++k)
            if (rs[k] == rs[i]) return BatchFault::Duplicate;
    }
    return BatchFault::None;
}

}  // namespace rsmp

