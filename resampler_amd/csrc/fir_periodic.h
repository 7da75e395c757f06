// fir_periodic.h -- the periodic (rational-ratio) FIR throughput kernels as the rest of the library sees them: device
// class tables, a handle's periodic state and the launch wrappers.  This is the header with HIP types; what is decided on
// the host without a device -- geometry, kernel build, class-table image -- is in fir_periodic_plan.h.
//
// For in_hz/out_hz = num/den the exact position of output m is m*num/den: the phase pattern
// repeats every `den` outputs and the reference's f64 position stays within ~1e-9 of it
// (measured per launch by FirMirror).  The kernels exploit that:
//   * outputs are grouped in *classes* j = m mod b and classes in tiles; b = r*den outputs consume a = r*num input
//     frames;
//   * per class the two phase rows are pre-mixed with the class's frac (the reference's lerp,
//     resampler_fir.rs:562-565 + fir/avx.rs:41-45, hoisted out of the per-sample loop -> `taps`
//     FMAs per value instead of 2*taps), shifted by the class's offset inside its tile and
//     zero padded, so all classes of a tile read the SAME input samples;
//   * the only outputs whose discrete choices depend on the sign of the f64 drift are those with
//     m*num/den integer: position just below the integer picks the previous frame and row 1023
//     (:562-564).  FirMirror lists them (`wraps`); the kernels compute that variant beside the ordinary one and select
//     per output from a bitmap, or (vector kernel, den < 8) a fix-up kernel recomputes them.
// Three kernel families (periodic_geometry picks one per rate pair and channel count):
//   * the vector kernel (fir_periodic.hip): tiles of 8 classes, r the smallest multiplier with a >= the padded row
//     length (a window never spans more than two period rows in LDS); the 64 lanes of a wave are 64 periods, the 8
//     coefficients of a tap wave-uniform through the scalar cache while the samples come from LDS: a register-tiled
//     8 x channels outer product per tap, a 9th accumulator for the wrap variant.  Any channel count;
//   * the exact-f32 matrix-core kernel (fir_periodic.hip): tiles of 16 classes on v_mfma_f32_16x16x4_f32, two LDS
//     images per workgroup, producer waves that only stage.  Two channels;
//   * the split kernel (fir_split.hip): tiles of 16 classes on the 16-bit matrix cores, every f32 operand cut into two
//     fp16 or three bf16 planes, a ring of two to four LDS images.  Up to 16 channels, 16 .. 320 classes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "fir_kernels.h"
#include "fir_periodic_plan.h"
#include "fir_plan.h"

namespace rsmp {

// Device image of one class table (HostClassTable, fir_periodic_plan.h): coefficients, wrap-variant coefficients,
// [tile] TileMeta.
// `hold` keeps the device allocation alive: the cache is bounded (a stream's drift moves on for as long as it runs, and
// every drift step is a new table), and a table that has left it is freed once nobody holds it any more AND the device
// has been waited for (kernels already enqueued may still read it): class_table_for.
struct ClassTable {
    const float* d_coef = nullptr;
    const float* d_wrap_coef = nullptr;
    const TileMeta* d_meta = nullptr;
    std::shared_ptr<void> hold;
};

// Per-handle periodic state: the class table currently bound to the stream.
struct PeriodicState {
    PeriodicGeometry geo;
    bool geo_valid = false;
    int geo_mode = -1;           // kernel mode the geometry was derived for
    ClassTable table;
    bool table_valid = false;
    double table_drift = 0.0;
};

// Makes sure `st` holds the geometry and the device class table matching the stream's rate pair
// and its current f64 drift (host build + one upload, cached per device and shared by every
// stream with the same polyphase table, rate pair and drift).
// `drift`: what the launch's coefficient rows are mixed for -- the middle between the stream's drift before the launch and
// behind it (the drift moves by ~1e-14 of a frame per output: a launch is half as far from its table that way).
int periodic_bind(PeriodicState& st, int device, const std::vector<float>& table, int kernel_mode,
                  const FirMirror& planned, double drift, uint32_t channels, hipStream_t stream);

// Device class table for a geometry and drift (built on the host once, cached per device).  `prebuilt`: the host image
// for exactly these arguments, from build_class_table run ahead of time (on another thread: it touches no device): only
// the allocation and the upload, 0.06 ms, are left for the caller.
int class_table_for(int device, const std::vector<float>& table, const PeriodicGeometry& g, double drift,
                    ClassTable* out, const HostClassTable* prebuilt = nullptr);

// One launch per geometry: d_descs[0..n_streams) all use `geo`; grid = (max_blocks, n_streams).
// `d_work_counter` is a zero-initialised 64-bit device word owned by the caller; the kernel leaves it
// at zero again (launches sharing it must be ordered, which launch_jobs enforces per handle).
// `nf`: where non-finite sums are marked (fir_nonfinite.h); the caller follows up with launch_fir_repair.
// items_key: a hash of everything the split kernel's item table depends on (the streams' counters in launch order; 0 =
// none): a launch with the key of the table already in the stream's workspace does not rebuild it.
// format: the launch's (fir_format.h; the descriptors' in_bits / out_bits / dither say the same).  PCM in or out: the split kernel's builds for it; hipErrorNotSupported
// where format_group_fault names a fault.  st, for a counting format: the table the builds count what they store into (FirStatArgs, fir_kernels.h; stream s of d_descs has row s).
hipError_t launch_fir_periodic(const FirStreamDesc* d_descs, uint32_t n_streams,
                               const PeriodicGeometry& geo, uint32_t max_blocks,
                               unsigned long long* d_work_counter, const NfArgs& nf, hipStream_t stream,
                               bool fuse_tail = false, uint64_t items_key = 0, const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});
// Recomputes the outputs listed in each stream's `wraps` with row 1023 / previous frame
// (only for geometries without inline wraps).
// (done / done_attached: as in launch_fir_repair_multi, fir_kernels.h)
hipError_t launch_fir_wrap_fixup(const FirStreamDesc* d_descs, uint32_t n_streams,
                                 uint32_t max_wraps, hipStream_t stream, hipEvent_t done = nullptr, bool* done_attached = nullptr);
// Split kernel (fir_split.hip) for a geometry with mfma == 3; `cus`: workgroups at most (device_cus, fir_kernel_launch.h).
// fuse_tail: the kernel also copies every stream's still-buffered tail into hist_next (no tail-copy launch)
hipError_t launch_fir_split(const FirStreamDesc* d_descs, uint32_t n_streams, const PeriodicGeometry& geo,
                            uint32_t max_blocks, uint32_t cus, bool fuse_tail, const NfArgs& nf, hipStream_t stream,
                            uint64_t items_key = 0, const FirFormat& format = FirFormat{}, const FirStatArgs& st = {});

// Several rate pairs in as few launches as their geometries allow (one item-table launch for all of them, then one
// launch of the kernel per window length among them): `jobs[j]` = the streams d_descs[0 .. n_streams) of geometry
// `geo`, as for launch_fir_split.  Jobs whose geometry the multi-job build does not cover (other than two channels)
// get a launch of their own.  The caller follows up with launch_fir_repair_multi over the same jobs' `nf`.
struct SplitJob {
    const FirStreamDesc* d_descs;
    uint32_t n_streams;
    const PeriodicGeometry* geo;
    uint32_t max_blocks;
    NfArgs nf;
};
// (items_prebuilt: the covered jobs' item tables, one behind the other, built before by a call with items_only = the stream to build
// them on -- which launches nothing else; fir_split_multi_item_words: how many words they take)
hipError_t launch_fir_split_multi(const SplitJob* jobs, size_t n_jobs, hipStream_t stream, uint32_t reserve_cus = 0,
                                  const uint32_t* items_prebuilt = nullptr, hipStream_t items_only = nullptr);
size_t fir_split_multi_item_words(const SplitJob* jobs, size_t n_jobs);

// Gives back the split kernel's item-table workspace of a stream that is about to be destroyed.
void split_release_stream(int device, hipStream_t stream);

}  // namespace rsmp
